// van_hove_kernels.h -- lag histograms behind the van Hove correlation functions G_s(r, t) and G_d(r, t) of point
// trajectories (gfx950, fp64).
//
// Frames f = 0 .. F-1 of n points, (F, n, 3) doubles straight from the caller and possibly unwrapped; origins o in
// [o_begin, o_end), lags l in [0, n_lags), a pair (o, l) only where o + l < F (the convention of msd_kernels.h).
//
//   self      Hs[l, b] = #{(o, j) : bin(|x_j(o + l) - x_j(o)|) = b}, the displacement as it is (no image, as the MSD), and the
//             moments M[l, 0] = sum |D|^2, M[l, 1] = sum |D|^4 over ALL terms, those at and beyond r_max included.
//   distinct  Hd[l, b] = #{(o, i, j), i != j : bin(|image(x_i(o + l) - x_j(o))|) = b}, ORDERED pairs, the minimal image of
//             pair_once_kernels.h (vh_image, the bits of wrap_nearest_pad_safe: valid for separations of any number of periods).
//
// Binning is hist_pair's (pair_hist_kernels.h), shared as vh_bin: gate r^2 < r_max^2, r = r^2 rsqrt(max(r^2, 1e-300)), bin =
// min((int)(r n_bins / r_max), n_bins - 1); r = 0 is bin 0.  XY: the z component of every separation is ignored.
// Counters are uint32 in the workgroup's LDS (ds_add_u32), flushed once to the caller's uint64 bins with integer atomics:
// the same bits for every launch plan; the host (rmb_van_hove.hip) sizes the launch so that no workgroup meets 2^31 terms.
//
//   van_hove_distinct_kernel  THE WORKGROUP OWNS A LAG.  A work unit is (origin, target tile I, source tile J) over the FULL
//             T x T tile grid of the lag (ordered pairs: not the upper triangle) and takes the 64 rotation steps of
//             pair_once_sweep: lane = point of tile I in frame o + l (registers), tile J of frame o in the wave's LDS slab,
//             step k meets slot (lane + k) & 63; on a diagonal unit step 0 is the i = j term and is skipped.  Workgroup
//             (lag, p) takes the p-th of P contiguous runs of the lag's units, its four waves stride inside the run; ONE
//             histogram of n_bins counters serves the workgroup and is flushed once.  Padding lanes are the +-1e100
//             sentinels: the image leaves them alone, x and y alone give r^2 >= 1e200, which fails the gate under both
//             planes (the host keeps r_max^2 below 1e199).
//   van_hove_self_kernel  A LANE OWNS A POINT.  A workgroup serves 256 points, a tile of up to kVhLagTile lags and a
//             contiguous range of origins: x_j(o) is loaded once per origin and kept in registers, x_j(o + l) is loaded per
//             lag (coalesced across lanes, L2-hot across neighbouring origins).  LDS holds (lags of the tile) x n_bins
//             counters.  At small lags nearly every term of a wave lands in one bin: where all counted lanes of a wave
//             agree, one lane adds the population count (vh_count) instead of 64 same-address adds.  The moments are kept
//             per lane and lag in registers, reduced per wave by a fixed butterfly, the four waves added in wave order,
//             written as the workgroup's partial;
//   van_hove_moments_finish_kernel  adds the partials of a lag in block order INTO the caller's (n_lags, 2): no
//             floating-point atomic anywhere, the same call gives the same bits.
#pragma once
#include "pair_hist_kernels.h"

namespace rmb {

constexpr int kVhWaves = 4;
constexpr int kVhBlock = 64 * kVhWaves;
constexpr int kVhLagTile = 8;               // lags per tile of the self sweep: 2 x 8 moment sums in registers per lane
constexpr int kVhSelfCounters = 8192;       // LDS counters of a self workgroup (32 KB: four to five workgroups per CU)
constexpr long kVhMaxUnitsPerWg = 1L << 18; // distinct: 2^18 units of 4096 terms = 2^30 terms per workgroup
constexpr long kVhMaxOriginsPerWg = 1L << 22;  // self: 256 points x 2^22 origins = 2^30 terms per counter

struct VanHoveArgs {
  const double* frames;   // (F, n, 3)
  long F, n;
  long n_lags, o_begin, o_end;
  double r_max2, inv_dr;  // r_max^2 (at most 1e199) and n_bins / r_max
  int n_bins;
  unsigned long long* hist;   // (n_lags, n_bins), added to
  // distinct
  double Lx, Ly, Lz, iLx, iLy, iLz;
  long T, P;              // tiles per frame, workgroups per lag
  // self
  int lt;                 // lags per tile
  long lag_tiles, point_blocks, S;   // S: origin ranges; workgroup ((tile S + s) point_blocks + pb)
  double* part;           // [workgroups][kVhLagTile][2]
  double* moments;        // (n_lags, 2), added to
};

// hist_pair's bin of a squared distance, -1 where the term is dropped
__device__ __forceinline__ int vh_bin(const VanHoveArgs& a, double r2) {
  if (!(r2 < a.r_max2)) return -1;
  // r = r2 rsqrt(r2); the floor keeps rsqrt finite at r = 0 (r = 0 * 1e150 = 0) and changes no other r
  const double r = r2 * rsqrt_f64(fmax(r2, 1e-300));
  const int bin = (int)(r * a.inv_dr);
  return bin < a.n_bins ? bin : a.n_bins - 1;      // r < r_max up to the last rounding: never past the counters
}

// image<> of pair_once_kernels.h for the rotation loop, the same r^2 to the bit with fewer instructions (measured: the loop is
// VALU-bound).  A select instead of a uniform branch per direction, which puts a wait between the slab reads; and the half
// that wrap_nearest_sym adds before truncating taken as copysign(0.5, d): at d = +-0, the only place the two differ, both
// give a zero.  The product and the sum are written as there, so that the compiler fuses them as there.
template <bool PERIODIC>
__device__ __forceinline__ double vh_image(double L, double iL, double d) {
  if constexpr (PERIODIC) {
    const double q = d * iL;
    const double w = __builtin_fma(-__builtin_trunc(q + __builtin_copysign(0.5, d)), L, d);
    d = (L > 0 && __builtin_fabs(d) < 1e50) ? w : d;
  }
  return d;
}

// the p-th of P contiguous runs of [0, total): without the product total * p
__device__ __forceinline__ void vh_run(long total, long p, long P, long& begin, long& end) {
  const long q = total / P, r = total - q * P;
  begin = q * p + (p < r ? p : r);
  end = begin + q + (p < r ? 1 : 0);
}

// PERIODIC: some direction has a period; PZ: z has one (under XY it is never looked at)
template <bool PERIODIC, bool XY, bool PZ>
__global__ __launch_bounds__(kVhBlock) void van_hove_distinct_kernel(const VanHoveArgs a) {
  __shared__ double rec_all[kVhWaves][3][64];
  extern __shared__ unsigned vh_hist[];      // [n_bins]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long lag = blockIdx.x / a.P, p = blockIdx.x - lag * a.P;
  const long o_last = a.F - lag < a.o_end ? a.F - lag : a.o_end;      // origins [o_begin, o_last) have this lag
  if (o_last <= a.o_begin) return;      // the whole workgroup
  const long TT = a.T * a.T;
  long u0, u1;
  vh_run((o_last - a.o_begin) * TT, p, a.P, u0, u1);
  if (u0 == u1) return;
  for (int b = threadIdx.x; b < a.n_bins; b += kVhBlock) vh_hist[b] = 0u;
  __syncthreads();

  double* rx = rec_all[wave][0];
  double* ry = rec_all[wave][1];
  double* rz = rec_all[wave][2];
  long row_cur = -1;
  double sx = 1e100, sy = 1e100, sz = 1e100;
  for (long u = u0 + wave; u < u1; u += kVhWaves) {
    const long oi = u / TT, rem = u - oi * TT;
    const long I = rem / a.T, J = rem - I * a.T;
    const long o = a.o_begin + oi;
    if (oi * a.T + I != row_cur) {      // the lane's own point: tile I of frame o + lag
      row_cur = oi * a.T + I;
      const long i = 64 * I + lane;
      sx = sy = sz = 1e100;
      if (i < a.n) {
        const double* s = a.frames + 3 * ((o + lag) * a.n + i);
        sx = s[0]; sy = s[1]; sz = s[2];
      }
    }
    const long j = 64 * J + lane;      // tile J of frame o into the slab
    double px = -1e100, py = -1e100, pz = -1e100;
    if (j < a.n) {
      const double* q = a.frames + 3 * (o * a.n + j);
      px = q[0]; py = q[1]; pz = q[2];
    }
    rx[lane] = px; ry[lane] = py;
    if constexpr (!XY) rz[lane] = pz;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int k = (I == J) ? 1 : 0; k < 64; ++k) {      // step 0 of a diagonal unit is i = j
      const int slot = (lane + k) & 63;
      const double qx = rx[slot], qy = ry[slot];
      double qz = 0.0;
      if constexpr (!XY) qz = rz[slot];
      const double dx = vh_image<PERIODIC>(a.Lx, a.iLx, sx - qx);
      const double dy = vh_image<PERIODIC>(a.Ly, a.iLy, sy - qy);
      double r2 = __builtin_fma(dy, dy, dx * dx);
      if constexpr (!XY) {
        const double dz = vh_image<PZ>(a.Lz, a.iLz, sz - qz);
        r2 = __builtin_fma(dz, dz, r2);
      }
      const int bin = vh_bin(a, r2);
      if (bin >= 0) atomicAdd(&vh_hist[bin], 1u);
    }
    __builtin_amdgcn_wave_barrier();   // the slab is rewritten by the next unit
  }
  __syncthreads();
  unsigned long long* out = a.hist + lag * a.n_bins;
  for (int b = threadIdx.x; b < a.n_bins; b += kVhBlock) {
    const unsigned v = vh_hist[b];
    if (v) atomicAdd(&out[b], (unsigned long long)v);
  }
}

// One term per lane into the counters `h`, bin < 0: none.  Where every counted lane of the wave has the same bin, one lane adds
// their number.
__device__ __forceinline__ void vh_count(unsigned* h, int bin, int lane) {
  if (bin >= 0) {
    const int b0 = __builtin_amdgcn_readfirstlane(bin);
    const unsigned long long counted = __ballot(1), same = __ballot(bin == b0);
    if (same == counted) {
      if (lane == __ffsll((long long)counted) - 1) atomicAdd(&h[b0], (unsigned)__popcll(counted));
    } else {
      atomicAdd(&h[bin], 1u);
    }
  }
}

template <bool XY>
__global__ __launch_bounds__(kVhBlock) void van_hove_self_kernel(const VanHoveArgs a) {
  __shared__ double red[kVhWaves][2 * kVhLagTile];
  extern __shared__ unsigned vh_hist[];      // [lt][n_bins]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long pb = blockIdx.x % a.point_blocks, rest = blockIdx.x / a.point_blocks;
  const long s = rest % a.S, tile = rest / a.S;
  const long l0 = tile * a.lt;
  const int nl = (int)(a.n_lags - l0 < a.lt ? a.n_lags - l0 : a.lt);
  long oa, ob;
  vh_run(a.o_end - a.o_begin, s, a.S, oa, ob);
  oa += a.o_begin; ob += a.o_begin;
  const int n_counters = nl * a.n_bins;
  for (int b = threadIdx.x; b < n_counters; b += kVhBlock) vh_hist[b] = 0u;
  __syncthreads();

  const long j = pb * kVhBlock + threadIdx.x;
  const bool valid = j < a.n;
  double m2[kVhLagTile], m4[kVhLagTile];
#pragma unroll
  for (int t = 0; t < kVhLagTile; ++t) m2[t] = m4[t] = 0.0;
  for (long o = oa; o < ob; ++o) {
    double x0 = 0.0, y0 = 0.0, z0 = 0.0;
    if (valid) {
      const double* q = a.frames + 3 * (o * a.n + j);
      x0 = q[0]; y0 = q[1]; z0 = q[2];
    }
#pragma unroll
    for (int t = 0; t < kVhLagTile; ++t) {
      if (t < nl && o + l0 + t < a.F) {      // workgroup-uniform
        int bin = -1;
        if (valid) {
          const double* q = a.frames + 3 * ((o + l0 + t) * a.n + j);
          const double dx = q[0] - x0, dy = q[1] - y0;
          double r2 = __builtin_fma(dy, dy, dx * dx);
          if constexpr (!XY) {
            const double dz = q[2] - z0;
            r2 = __builtin_fma(dz, dz, r2);
          }
          m2[t] += r2;
          m4[t] = __builtin_fma(r2, r2, m4[t]);
          bin = vh_bin(a, r2);
        }
        vh_count(vh_hist + t * a.n_bins, bin, lane);
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_counters; b += kVhBlock) {
    const unsigned v = vh_hist[b];
    if (v) atomicAdd(&a.hist[l0 * a.n_bins + b], (unsigned long long)v);
  }
  // moments: butterfly over the wave, then the four waves in wave order
#pragma unroll
  for (int t = 0; t < kVhLagTile; ++t) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      m2[t] += __shfl_xor(m2[t], m);
      m4[t] += __shfl_xor(m4[t], m);
    }
    if (lane == 0) { red[wave][2 * t] = m2[t]; red[wave][2 * t + 1] = m4[t]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * kVhLagTile) {
    double sum = red[0][threadIdx.x];
    for (int w = 1; w < kVhWaves; ++w) sum += red[w][threadIdx.x];
    a.part[(size_t)blockIdx.x * (2 * kVhLagTile) + threadIdx.x] = sum;
  }
}

// one thread per (lag, moment): the partials of the lag's tile, origin ranges and point blocks in block order
__global__ __launch_bounds__(256) void van_hove_moments_finish_kernel(const VanHoveArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * a.n_lags) return;
  const long lag = i >> 1, tile = lag / a.lt;
  const int slot = (int)(2 * (lag - tile * a.lt) + (i & 1));
  const long per_tile = a.S * a.point_blocks;
  const double* part = a.part + (size_t)tile * per_tile * (2 * kVhLagTile) + slot;
  double sum = 0.0;
  for (long b = 0; b < per_tile; ++b) sum += part[(size_t)b * (2 * kVhLagTile)];
  a.moments[i] += sum;
}

}  // namespace rmb
