// hydro_function_kernels.h -- the hydrodynamic function H(k) of a point configuration (gfx950, fp64): the quadratic form of
// the translational pair mobility with plane waves,
//
//   H(k; e) = (1 / (N mu0)) sum_i sum_j  e^T M_ij e  cos(k . (x_i - x_j)),
//
// what joins the mobility half of the library (pair_blocks.h) to its trajectory analyses.  HydroOp is a policy of the
// pair-once frame (pair_once_kernels.h), the first one with SLOTS: next to the position records a wave keeps the phase
// factors of tile J's points in a second LDS slab.
//
// M is the matrix of the context's tt product: the RPY block with its overlap patch; above a wall the Swan-Brady block on
// heights clamped to z <= a -> a, every block damped by b_i b_j, b = z / a for z < a (pack_positions_kernel's rule,
// matvec_kernels.h); with periodic lengths the 3^d images around the nearest one (sym_kernels.h's loop).  The i = j term
// is self_term (pair_ops.h) plus, in a box, the point's own images by the pair formula.
//
// The pair block does not depend on the wavevector.  With e6 = (e_x^2, e_y^2, e_z^2, 2 e_x e_y, e_x e_z, e_y e_z) and
// M6 = (M_xx, M_yy, M_zz, M_xy, M_xz + M_zx, M_yz + M_zy) summed over the images, e^T M e = M6 . e6: the block -- some 80
// instructions and two reciprocal square roots per image -- is built ONCE per pair and contracted with the kHydroKC
// wavevectors of the wave's chunk at nine instructions each:
//
//   q = M6 . e6[m]                           one multiply, five fused steps, e6 wave-uniform
//   t = c_i c_j + s_i s_j                    cos(theta_i - theta_j); (c_j, s_j) is ONE 16-byte LDS read
//   sum[m] = fma(q, t, sum[m])
//
// The phase theta = k . x goes through scat_phase (scat_phase.h, the scattering sweeps' route: reduced in turns before the multiplication by
// 2 pi), on the RAW coordinates: a lane computes (c, s) of its own point when its tile changes and of the point it stages
// when tile J is staged -- 64 points per 64 x 64 pairs -- so no (N, K) table of phases exists anywhere.  Where the
// mobility is periodic in a direction its period is the wavevector's length (the host refuses anything else), so the
// phase factor is the same for every image.
//
// Launch: grid (walk workgroups, ceil(K / kHydroKC)); blockIdx.y picks the chunk of wavevectors, the x direction walks the
// (frame, tile pair) units exactly as every other pair-once sweep.  No tile is culled: the mobility is long-ranged.
//
// kHydroKC = 8.  A lane holds 2 x 8 phase factors and 8 sums (48 VGPRs) for the whole walk, the pair's M6 and the block build
// on top: 139 ... 153 VGPRs, three waves per SIMD (the wall block inside a box's image loop 187, two waves); no scratch.
// The slabs take 8 + 32 KB of LDS per workgroup.  Per pair and wavevector one ds_read_b128 (1 KB per wave: 8 cycles of the
// CU's 128 bytes per clock) stands against nine fp64 instructions (36 cycles of a SIMD); four SIMDs ask for 32 of every 36
// LDS cycles, so the LDS just keeps up.  A chunk of 16 would save half of the block builds that are left -- a sixteenth of
// a pair's cost -- for 48 more registers per lane, one wave per SIMD fewer, and the same LDS traffic per wavevector; a chunk
// of 4 doubles the block builds per wavevector.  (profiles/r32_hydro_function_kernel_resources.txt.)
//
// Reduction, no floating-point atomic.  The steps of a frame are cut into chunks of spw steps (the last one short), the same
// cut for every frame whatever the number of frames of the call: a chunk never reaches into the next frame.  A lane adds its
// terms in walk order; at the end of a chunk (flush) the wave adds its 64 lanes by a fixed butterfly and stores ONE record
// of kHydroKC sums in the chunk's slot.  hydro_finish_kernel, one thread per (frame, wavevector), adds the records of the
// frame's chunks in chunk order, contracts the six self sums (hydro_self_kernel: one workgroup per frame, fixed order) with
// e6, scales by 1 / (8 pi eta) and OVERWRITES out[f, m, 0:2] = (S_self, S_dist).  A term passes through at most spw <= 64 U
// additions in its lane (U = units per frame), 6 in the butterfly and ceil(64 U / spw) in the finishing launch: never more
// than 64 U + 9.  The same call gives the same bits, and a frame's sums do not depend on the frames it is handed over with.
#pragma once
#include "pair_blocks.h"
#include "pair_once_kernels.h"
#include "scat_phase.h"

namespace rmb {

constexpr int kHydroKC = 8;            // wavevectors per wave
// register budget of the sweep: three waves per SIMD (168 VGPRs); the wall block inside the image loop of a box needs
// more than that and takes two (the nine block builds per pair hide the LDS latency by themselves)
constexpr int hydro_waves_per_eu(bool wall, bool periodic) { return wall && periodic ? 2 : 3; }
constexpr int kHydroCoefBatch = 64;    // wavevectors per hydro_coef_kernel launch: 2.25 KB of kernel arguments

struct HydroCoefArgs {
  int n[3 * kHydroCoefBatch];
  double e[3 * kHydroCoefBatch];
  double L[3];
  long count;
  double* coef;      // (count, 3): n_d / L_d
  double* e6;        // (count, 6)
};

// pos, bounds: resident only (bounds unused: nothing is culled).  Lx .. iLz: the MOBILITY's periods.
struct HydroArgs : PairOnceArgs {
  const double* frames;      // BATCH: (n_frames, n, 3) raw coordinates
  long units_per_frame;      // n_tiles (n_tiles + 1) / 2
  long n_frames;             // resident: 1
  double radius;             // a
  double prefactor;          // 1 / (8 pi eta)
  PairConsts k;
  const double* coef;        // (K padded to kHydroKC, 3), zeros past K
  const double* e6;          // (K padded, 6), zeros past K
  long K;
  long spw;                  // steps per chunk of the walk
  long chunks_per_frame;     // ceil(64 units_per_frame / spw): the chunks are cut per frame (pair_once_kernels.h, SLOTS)
  long n_seg;                // n_frames * chunks_per_frame records per chunk of wavevectors
  double* part;              // [K chunks][n_seg][kHydroKC]
  double* self6;             // [n_frames][6]: sum_i b_i^2 M6_ii
  double* out;               // (n_frames, K, 2)
};

__global__ __launch_bounds__(kHydroCoefBatch) void hydro_coef_kernel(const HydroCoefArgs a) {
  const long i = threadIdx.x;
  if (i >= a.count) return;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int n = a.n[3 * i + d];
    a.coef[3 * i + d] = n != 0 ? (double)n / a.L[d] : 0.0;      // scat_coef_kernel's rule
  }
  const double ex = a.e[3 * i], ey = a.e[3 * i + 1], ez = a.e[3 * i + 2];
  double* o = a.e6 + 6 * i;
  o[0] = ex * ex; o[1] = ey * ey; o[2] = ez * ez;
  o[3] = 2.0 * (ex * ey); o[4] = ex * ez; o[5] = ey * ez;
}

// M6 += the tt block of one separation (an image of the pair, or of the point itself)
template <bool WALL>
__device__ __forceinline__ void hydro_block(const PairConsts& k, double dx, double dy, double dz, double zi, double zj, double (&m)[6]) {
  const Geom g = make_geom<WALL>(dx, dy, dz, zi, zj);
  const TTc c = tt_coeffs<WALL>(k, g, zi, zj);
  const double Pdx = c.P * dx, Pdy = c.P * dy;
  m[0] += __builtin_fma(Pdx, dx, c.F);
  m[1] += __builtin_fma(Pdy, dy, c.F);
  m[3] = __builtin_fma(Pdx, dy, m[3]);
  if constexpr (WALL) {
    const double Q = c.Q3 + c.Q4;
    m[2] += c.Szz;
    m[4] = __builtin_fma(Q, dx, m[4]);
    m[5] = __builtin_fma(Q, dy, m[5]);
  } else {
    const double Pdz = c.P * dz;
    m[2] += __builtin_fma(Pdz, dz, c.F);
    m[4] = __builtin_fma(Pdx + Pdx, dz, m[4]);
    m[5] = __builtin_fma(Pdy + Pdy, dz, m[5]);
  }
}

template <bool WALL, bool PERIODIC, bool BATCH>
struct HydroOp {
  typedef HydroArgs Args;
  struct Lane {
    double c[kHydroKC], s[kHydroKC];      // phase factors of the lane's own point
    double sum[kHydroKC];                 // distinct-pair sums of the wave's wavevectors
    double zi;                            // clamped height of the lane's own point
    double2* ph;                          // the wave's second slab: (c, s) of slot l for wavevector m at [64 m + l]
  };
  static constexpr bool FRAMES = BATCH;
  static constexpr bool SLOTS = true;
  static constexpr double PAD_W = 0.0;      // b = 0: a padding record weighs nothing (its block is finite: 2e100 away)

  // record: x, y, RAW z, b
  static __device__ __forceinline__ double4 fetch(const Args& a, long frame, long i) {
    if constexpr (BATCH) {
      const double* p = a.frames + 3 * (frame * a.n + i);
      const double z = p[2];
      return make_double4(p[0], p[1], z, (WALL && z < a.radius) ? z / a.radius : 1.0);
    } else {
      const double4 p = a.pos[i];      // packed: (x, y, clamped z, b)
      return make_double4(p.x, p.y, (WALL && p.w < 1.0) ? p.w * a.radius : p.z, p.w);
    }
  }
  static __device__ __forceinline__ double height(const Args& a, double z) { return (WALL && z <= a.radius) ? a.radius : z; }
  static __device__ __forceinline__ bool culled(const Args&, int, int) { return false; }
  static __device__ __forceinline__ bool guarded(const Args&, int, int) { return false; }

  // (c, s) of point p for the wave's wavevectors into slot `lane` of the slab.  One wavevector at a time on purpose: eight
  // interleaved sincospi expansions cost a hundred registers that the pair loop then has to spill.
  static __device__ __forceinline__ void phases(const Args& a, const double4& p, double2* ph, int lane) {
    const double* coef = a.coef + 3L * kHydroKC * blockIdx.y;
#pragma unroll 1
    for (int m = 0; m < kHydroKC; ++m) {
      double s, c;
      scat_phase(p.x, p.y, p.z, coef[3 * m], coef[3 * m + 1], coef[3 * m + 2], &s, &c);
      ph[64 * m + lane] = make_double2(c, s);
    }
  }
  // the lane's own phases go through its slot of the slab (free between two units; a lane reads back what it wrote itself)
  static __device__ __forceinline__ void row(const Args& a, Lane& st, const double4& self, bool) {
    const int lane = threadIdx.x & 63;
    st.zi = height(a, self.z);
    phases(a, self, st.ph, lane);
#pragma unroll
    for (int m = 0; m < kHydroKC; ++m) {
      const double2 v = st.ph[64 * m + lane];
      st.c[m] = v.x; st.s[m] = v.y;
    }
  }
  static __device__ __forceinline__ void stage(const Args& a, Lane& st, const double4& p, int lane, bool diag) {
    if (diag) {
#pragma unroll
      for (int m = 0; m < kHydroKC; ++m) st.ph[64 * m + lane] = make_double2(st.c[m], st.s[m]);
    } else {
      phases(a, p, st.ph, lane);
    }
  }

  // the images of one separation (already the nearest image), central box included unless SELF
  template <bool SELF>
  static __device__ __forceinline__ void images(const Args& a, double dx, double dy, double dz, double zi, double zj, double (&m)[6]) {
    if constexpr (!PERIODIC) {
      if constexpr (!SELF) hydro_block<WALL>(a.k, dx, dy, dz, zi, zj, m);
    } else {
      const int px = a.Lx > 0, py = a.Ly > 0, pz = a.Lz > 0;
      for (int bx = -px; bx <= px; ++bx)
        for (int by = -py; by <= py; ++by)
          for (int bz = -pz; bz <= pz; ++bz) {
            if (SELF && bx == 0 && by == 0 && bz == 0) continue;
            hydro_block<WALL>(a.k, dx + bx * a.Lx, dy + by * a.Ly, dz + bz * a.Lz, zi, zj, m);
          }
    }
  }

  // the self term carries no phase and is not a pair's: hydro_self_kernel takes it, step 0 of the diagonal units stays empty
  static __device__ __forceinline__ void diag_start(const Args&, Lane&, const double4&, bool) {}
  // b_i^2 M6_ii of one point: self_term plus, in a box, the point's own images by the pair formula
  static __device__ __forceinline__ void self_block(const Args& a, const double4& p, double (&m)[6]) {
    const double zi = height(a, p.z);
    Vec3 u = {0.0, 0.0, 0.0};
    self_term<KIND_TT, WALL>(a.k, zi, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, u);      // the diagonal (s_xx, s_xx, s_zz)
    m[0] = u.x; m[1] = u.y; m[2] = u.z; m[3] = 0.0; m[4] = 0.0; m[5] = 0.0;
    images<true>(a, 0.0, 0.0, 0.0, zi, zi, m);
    const double w = p.w * p.w;
#pragma unroll
    for (int t = 0; t < 6; ++t) m[t] *= w;
  }

  template <bool GUARDED>
  static __device__ __forceinline__ void pair(const Args& a, Lane& st, const double4& self, const double4& q, bool take, int slot) {
    const double zj = height(a, q.z);
    const double dx = image<PERIODIC>(a.Lx, a.iLx, self.x - q.x);
    const double dy = image<PERIODIC>(a.Ly, a.iLy, self.y - q.y);
    const double dz = image<PERIODIC>(a.Lz, a.iLz, st.zi - zj);
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    images<false>(a, dx, dy, dz, st.zi, zj, m);
    const double w = take ? self.w * q.w : 0.0;
#pragma unroll
    for (int t = 0; t < 6; ++t) m[t] *= w;
    // The 48 doubles of e6 are wave-uniform and belong in the scalar file -- which cannot hold them across the whole walk
    // next to everything else.  Left alone the compiler hoists them out of the pair loop into 96 VGPRs and spills the lane's
    // sums instead; the pointer is laundered once per pair so that they stay scalar loads (scalar cache hits) inside the loop.
    // (An asm result counts as divergent and, turned back into a pointer, as a flat address: read back through readfirstlane
    // and into the constant address space it is uniform read-only memory again and the loads are s_load, not 24 vector
    // loads of one address per pair.)
    typedef const double __attribute__((address_space(4))) * UniformDoubles;
    unsigned long e6_bits = reinterpret_cast<unsigned long>(a.e6 + 6L * kHydroKC * blockIdx.y);
    asm volatile("" : "+s"(e6_bits));
    // readfirstlane returns a signed int: both halves go through unsigned, or the low half's sign would fill the high one
    const unsigned e6_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(e6_bits >> 32));
    const unsigned e6_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)e6_bits);
    const UniformDoubles e6 = (UniformDoubles)(((unsigned long)e6_hi << 32) | (unsigned long)e6_lo);
#pragma unroll
    for (int k = 0; k < kHydroKC; ++k) {
      const double2 ph = st.ph[64 * k + slot];
      const UniformDoubles e = e6 + 6 * k;
      const double qf = __builtin_fma(m[0], e[0], __builtin_fma(m[1], e[1], __builtin_fma(m[2], e[2],
                        __builtin_fma(m[3], e[3], __builtin_fma(m[4], e[4], m[5] * e[5])))));
      const double t = __builtin_fma(st.c[k], ph.x, st.s[k] * ph.y);
      st.sum[k] = __builtin_fma(qf, t, st.sum[k]);
    }
  }

  // one record per chunk: fixed butterfly over the lanes, lane 0 stores, the sums start again
  static __device__ __forceinline__ void flush(const Args& a, Lane& st, long seg) {
#pragma unroll
    for (int k = 0; k < kHydroKC; ++k) {
      double v = st.sum[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if ((threadIdx.x & 63) == 0) a.part[((long)blockIdx.y * a.n_seg + seg) * kHydroKC + k] = v;
      st.sum[k] = 0.0;
    }
  }
};

template <bool WALL, bool PERIODIC, bool BATCH>
__global__ __launch_bounds__(64 * kSymWaves)
__attribute__((amdgpu_waves_per_eu(hydro_waves_per_eu(WALL, PERIODIC), hydro_waves_per_eu(WALL, PERIODIC)))) void hydro_function_kernel(const HydroArgs a) {
  typedef HydroOp<WALL, PERIODIC, BATCH> OP;
  __shared__ double4 rec_all[kSymWaves][64];
  __shared__ double2 ph_all[kSymWaves][64 * kHydroKC];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typename OP::Lane st{};
  st.ph = ph_all[wave];
  pair_once_sweep<OP>(a, st, rec_all[wave]);
}

// The self sums of a frame: self6[f] = sum_i b_i^2 M6_ii.  One workgroup per frame; thread t adds the points t, t + 256, ...
// in that order, then a fixed tree over the 256 threads.
template <bool WALL, bool PERIODIC, bool BATCH>
__global__ __launch_bounds__(256) void hydro_self_kernel(const HydroArgs a) {
  typedef HydroOp<WALL, PERIODIC, BATCH> OP;
  __shared__ double red[6][256];
  const long f = blockIdx.x;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long i = threadIdx.x; i < a.n; i += 256) {
    double m[6];
    OP::self_block(a, OP::fetch(a, f, i), m);
#pragma unroll
    for (int t = 0; t < 6; ++t) acc[t] += m[t];
  }
#pragma unroll
  for (int t = 0; t < 6; ++t) red[t][threadIdx.x] = acc[t];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
#pragma unroll
      for (int t = 0; t < 6; ++t) red[t][threadIdx.x] += red[t][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < 6) a.self6[6 * f + threadIdx.x] = red[threadIdx.x][0];
}

// one thread per (frame, wavevector): the records of the chunks that touch the frame, in chunk order
__global__ __launch_bounds__(256) void hydro_finish_kernel(const HydroArgs a) {
  const long i = 256L * blockIdx.x + threadIdx.x;
  if (i >= a.n_frames * a.K) return;
  const long f = i / a.K, m = i - f * a.K;
  const long y = m / kHydroKC, k = m - y * kHydroKC;
  double dist = 0.0;
  for (long c = f * a.chunks_per_frame; c < (f + 1) * a.chunks_per_frame; ++c) dist += a.part[(y * a.n_seg + c) * kHydroKC + k];
  const double* e = a.e6 + 6 * m;
  const double* s6 = a.self6 + 6 * f;
  const double self = __builtin_fma(s6[0], e[0], __builtin_fma(s6[1], e[1], __builtin_fma(s6[2], e[2],
                      __builtin_fma(s6[3], e[3], __builtin_fma(s6[4], e[4], s6[5] * e[5])))));
  a.out[2 * i] = a.prefactor * self;
  a.out[2 * i + 1] = a.prefactor * (dist + dist);
}

}  // namespace rmb
