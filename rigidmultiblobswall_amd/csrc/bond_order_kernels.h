// bond_order_kernels.h -- bond-orientational order of point frames (gfx950, fp64): the neighbour sums behind psi_m(i) and
// the pair correlation of a quantised per-point field behind g_m(r).  Two policies of frames that exist: BondOrderOp of the
// one-sided sweep (onesided_kernels.h) and PairFieldOp of the pair-once sweep (pair_once_kernels.h), and the kernels around
// the calls.  The time correlation C_m(t) needs no kernel: it is the lag sweep of rmb_scattering.hip over (Re psi, Im psi).
//
// Pass 1, BondOrderOp.  Targets and sources are the points of ONE frame; the frame is blockIdx.z (the kernels shift the
// frame's pointers and hand the frame a copy of the arguments), so many frames of few points are one launch.  For target i
// and source j: the separation in the minimal image of every direction with a positive period (wrap_nearest, the formula of
// pair_hist_kernels.h, any number of periods away), rho^2 = dx^2 + dy^2, d^2 = rho^2 (plane xy) or rho^2 + dz^2 (xyz).
// j is a neighbour when d^2 < r_cut^2 and rho^2 > 0: the point itself and points stacked on it have no bond angle and are
// left out of the sums AND of the count, so no index test is needed.  z = (dx + i dy) rsqrt_f64(rho^2) -- no trigonometric
// function -- and z^m by left-to-right binary powering (bond_power: at most 2 floor(log2 m) complex products), for up to 4
// wave-uniform runtime orders m <= 16.  Sums: [N_i, Re sum z^m1, Im sum z^m1, ...]; NOUT = 9 registers, of which only 1 + 2 K
// are stored.  A source that is nobody's neighbour in the wave is skipped by one wave-uniform branch (it would add zeros).
// The order of the sum over j is the frame's: fixed for a given chunk count, so the same call gives the same bits.
//
// Pass 2, PairFieldOp (BATCH layout, as PairHistOp<., true>).  The field of a point is two int32 (a, b) = rint(psi 2^30); it
// travels in .w of the pair-once record as the BITS of a double and is only ever moved (__longlong_as_double and back, loads,
// stores, selects): no floating-point operation touches it.  PAD_W = 0.0 is the field (0, 0), and a padded pair fails
// r < r_max anyway.  Per unordered pair with r < r_max (binning exactly hist_pair's): counts[bin] += 1 (uint32 in LDS) and
// sums[bin] += (a_i a_j + b_i b_j + 2^29) >> 30 (int64 in LDS, arithmetic shift); every workgroup flushes its non-empty
// bins once with integer atomics.  Integer sums commute: the same bits for every launch plan, permutation and cut of the
// trajectory.  |term| <= 2^30 + 1 for |psi| <= 1 (2^31 + 1 at the corner (-2^30, -2^30)) and a workgroup meets fewer than 2^31
// pairs (the host's plan), so |LDS sum| < 2^62 (2^63 at the corner).
#pragma once
#include "onesided_kernels.h"
#include "pair_once_kernels.h"

namespace rmb {

constexpr int kBondMaxOrders = 4;       // orders per call
constexpr int kBondMaxOrder = 16;       // 1 <= m <= 16
constexpr int kPairFieldMaxBins = 4096; // 12 bytes of LDS counters per bin: 48 KB

struct BondOrderArgs : OneSidedArgs {   // n_src = points per frame; targets [0, n_src); out / partial / frames: of frame 0
  const double* frames;                 // (n_frames, n, 3)
  double rc2;                           // r_cut^2
  double Lx, Ly, Lz, iLx, iLy, iLz;     // Lz = 0 under plane xy
  long out_stride, partial_stride;      // doubles per frame of out (n (1 + 2 K)) and of partial (n_chunks NOUT n_tgt_pad)
  int xy;                               // 1: d is the in-plane distance
  int n_orders;
  int orders[kBondMaxOrders];
};

// (zx + i zy)^m, m >= 1, left to right over the bits of m below the leading one: square, and multiply by z where the bit is
// set.  m is wave-uniform: the loop is scalar.
__device__ __forceinline__ void bond_power(double zx, double zy, int m, double& px, double& py) {
  px = zx; py = zy;
  for (int b = 30 - __builtin_clz(m); b >= 0; --b) {
    const double sx = __builtin_fma(px, px, -(py * py)), sy = 2.0 * (px * py);
    px = sx; py = sy;
    if ((m >> b) & 1) {
      const double mx = __builtin_fma(px, zx, -(py * zy)), my = __builtin_fma(px, zy, py * zx);
      px = mx; py = my;
    }
  }
}

template <bool PERIODIC> struct BondOrderOp {
  typedef BondOrderArgs Args;
  struct Target { double x, y, z; };
  static constexpr int NOUT = 1 + 2 * kBondMaxOrders, REC2 = 2;
  static constexpr bool SHARDED = false, SKIP_OWN_TILE = false;      // the point itself has rho^2 = 0

  static __device__ __forceinline__ Target load_target(const Args& a, long t) {
    const double* p = a.frames + 3 * t;
    return {p[0], p[1], p[2]};
  }

  static __device__ __forceinline__ void stage(const Args& a, long j, double2* rec) {
    const double* p = a.frames + 3 * j;
    rec[0] = make_double2(p[0], p[1]);
    rec[1] = make_double2(p[2], 0.0);
  }

  template <bool>
  static __device__ __forceinline__ void tile_pairs(const Args& a, const double2* tile, int n, int wave, long, long, const Target& tg,
                                                    double* acc) {
    for (int s = wave; s < n; s += kWaves) {
      const double2 q0 = tile[s * 2 + 0], q1 = tile[s * 2 + 1];
      double dx = tg.x - q0.x, dy = tg.y - q0.y, dz = tg.z - q1.x;
      if constexpr (PERIODIC) {
        if (a.Lx > 0) dx = wrap_nearest(dx, a.Lx, a.iLx);
        if (a.Ly > 0) dy = wrap_nearest(dy, a.Ly, a.iLy);
        if (a.Lz > 0) dz = wrap_nearest(dz, a.Lz, a.iLz);
      }
      const double rho2 = __builtin_fma(dy, dy, dx * dx);
      const double d2 = a.xy ? rho2 : __builtin_fma(dz, dz, rho2);
      const bool nb = d2 < a.rc2 && rho2 > 0.0;
      if (__any(nb)) {
        const double ir = rsqrt_f64(nb ? rho2 : 1.0);
        const double zx = nb ? dx * ir : 0.0, zy = nb ? dy * ir : 0.0;      // not a neighbour: z = 0, every power 0
        acc[0] += nb ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < kBondMaxOrders; ++k) {
          if (k < a.n_orders) {
            double px, py;
            bond_power(zx, zy, a.orders[k], px, py);
            acc[1 + 2 * k] += px; acc[2 + 2 * k] += py;
          }
        }
      }
    }
  }

  static __device__ __forceinline__ void store(const Args& a, long t, const Target&, const double* acc) {
    const int w = 1 + 2 * a.n_orders;
    double* o = a.out + w * t;
#pragma unroll
    for (int c = 0; c < NOUT; ++c)
      if (c < w) o[c] = acc[c];
  }
};

// the arguments as frame blockIdx.z (sweep) / blockIdx.y (finishing launch) sees them
__device__ __forceinline__ BondOrderArgs bond_order_frame(const BondOrderArgs& a0, long frame) {
  BondOrderArgs a = a0;
  a.frames += 3 * a.n_src * frame;
  a.out += a.out_stride * frame;
  if (a.n_chunks > 1) a.partial += a.partial_stride * frame;
  return a;
}

template <bool PERIODIC>
__global__ __launch_bounds__(kBlock) void bond_order_kernel(const BondOrderArgs a0) {
  const BondOrderArgs a = bond_order_frame(a0, blockIdx.z);
  one_sided_sweep<BondOrderOp<PERIODIC>>(a);
}

__global__ __launch_bounds__(256) void bond_order_finalize_kernel(const BondOrderArgs a0) {
  const BondOrderArgs a = bond_order_frame(a0, blockIdx.y);
  one_sided_finalize<BondOrderOp<false>>(a);
}

struct PairFieldArgs : PairOnceArgs {      // pos, bounds, cull2, order, xcd: unused (BATCH layout)
  double r_max2, inv_dr;      // r_max^2 (below the padding's 1e200) and n_bins / r_max
  int n_bins;
  int xy;                     // 1: r is the in-plane distance
  unsigned long long* counts; // [n_bins], added to
  long long* sums;            // [n_bins], added to
  const double* frames;       // (n_frames, n, 3)
  const long long* field;     // (n_frames, n): two int32 (a, b) per point, a in the low half
  long units_per_frame;       // n_tiles (n_tiles + 1) / 2;  step_end = n_frames * units_per_frame * 64
};

template <bool PERIODIC>
struct PairFieldOp {
  typedef PairFieldArgs Args;
  struct Lane { unsigned* counts; long long* sums; };      // the workgroup's LDS accumulators
  static constexpr bool FRAMES = true;
  static constexpr double PAD_W = 0.0;      // the field (0, 0)
  static __device__ __forceinline__ double4 fetch(const Args& a, long frame, long i) {
    const long k = frame * a.n + i;
    const double* p = a.frames + 3 * k;
    return make_double4(p[0], p[1], p[2], __longlong_as_double(a.field[k]));      // bits only
  }
  static __device__ __forceinline__ bool culled(const Args&, int, int) { return false; }      // no bounds
  static __device__ __forceinline__ void diag_start(const Args&, Lane&, const double4&, bool) {}
  static __device__ __forceinline__ bool guarded(const Args&, int, int) { return false; }
  template <bool GUARDED>
  static __device__ __forceinline__ void pair(const Args& a, Lane& st, const double4& self, const double4& q, bool take) {
    const double dx = image<PERIODIC>(a.Lx, a.iLx, self.x - q.x);
    const double dy = image<PERIODIC>(a.Ly, a.iLy, self.y - q.y);
    const double dz = a.xy ? 0.0 : image<PERIODIC>(a.Lz, a.iLz, self.z - q.z);
    const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
    if (take && r2 < a.r_max2) {
      const double r = r2 * rsqrt_f64(fmax(r2, 1e-300));      // hist_pair's arithmetic: the same bin
      int bin = (int)(r * a.inv_dr);
      bin = bin < a.n_bins ? bin : a.n_bins - 1;
      const long long fi = __double_as_longlong(self.w), fj = __double_as_longlong(q.w);
      const long long term = ((long long)(int)fi * (long long)(int)fj + (long long)(int)(fi >> 32) * (long long)(int)(fj >> 32) + (1LL << 29)) >> 30;
      atomicAdd(&st.counts[bin], 1u);
      atomicAdd((unsigned long long*)&st.sums[bin], (unsigned long long)term);      // two's complement: the signed sum
    }
  }
};

template <bool PERIODIC>
__global__ __launch_bounds__(64 * kSymWaves) void pair_field_kernel(const PairFieldArgs a) {
  typedef PairFieldOp<PERIODIC> OP;
  __shared__ double4 rec_all[kSymWaves][64];
  extern __shared__ long long field_lds[];      // sums [n_bins], then counts [n_bins]
  long long* sums = field_lds;
  unsigned* counts = (unsigned*)(field_lds + a.n_bins);
  for (int b = threadIdx.x; b < a.n_bins; b += 64 * kSymWaves) { sums[b] = 0; counts[b] = 0u; }
  __syncthreads();
  typename OP::Lane st{counts, sums};
  pair_once_sweep<OP>(a, st, rec_all[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
  __syncthreads();
  for (int b = threadIdx.x; b < a.n_bins; b += 64 * kSymWaves) {
    const unsigned v = counts[b];
    if (v) {
      atomicAdd(&a.counts[b], (unsigned long long)v);
      atomicAdd((unsigned long long*)&a.sums[b], (unsigned long long)sums[b]);
    }
  }
}

}  // namespace rmb
