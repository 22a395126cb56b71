// pair_hist_kernels.h -- histogram of the pair distances of a point configuration (gfx950, fp64): the counts behind the
// radial distribution function g(r).
//
// The reference's g(r) program (multi_bodies/examples/Radial_Dist_Test/gr_pseudo2D_single_blob.cpp) is a single-threaded
// loop over frames and pairs i < j: minimal image, r = sqrt(dx^2 + dy^2 + dz^2), bin = int(r / dr), hist[bin] += 2 while
// bin < n_bins.  Here every unordered pair is met once by the pair-once frame (pair_once_kernels.h), of which this file
// holds the histogram's policy and the kernel around the call.  A pair with r < r_max adds ONE count (the unordered pair) to bin
// (int)(r n_bins / r_max) of a uint32 histogram in the workgroup's LDS (ds_add_u32); at the end the workgroup adds its
// non-empty bins to the caller's uint64 histogram with integer atomics.  Integer sums commute: the result is the same
// bits for every launch plan, permutation and culling choice; no finishing kernel, no floating-point atomic.  The host
// (rmb_pair_hist.hip) sizes the launch so that a workgroup meets fewer than 2^31 pairs: no LDS counter can wrap.
//
//   * minimal image in every direction with a positive period, z included, by wrap_nearest_sym (the reference program's
//     formula, valid for separations of any number of periods: unwrapped trajectories need nothing special);
//   * the padding sentinels (+-1e100) are left alone by the image (wrap_nearest_pad_safe), so a padded pair has
//     r^2 >= 1e200 and fails r < r_max before anything is converted to an integer;
//   * coincident points (r = 0) count in bin 0; no wall gate, no one-point term.
//
// BATCH: many frames of few points, packed (n_frames, n, 3) doubles straight from the caller.  Units run over
// (frame, tile pair), the frame being the slow index; row-major unit order, no bounds, no culling, no sort.
#pragma once
#include "pair_once_kernels.h"

namespace rmb {

constexpr int kPairHistMaxBins = 8192;      // 32 KB of LDS counters

struct PairHistArgs : PairOnceArgs {      // pos, bounds, cull2 (r_max^2, +inf = no culling): resident only
  double r_max2, inv_dr;   // r_max^2 and n_bins / r_max
  int n_bins;
  unsigned long long* hist;   // [n_bins], added to
  // BATCH only (step_end = n_frames * units_per_frame * 64)
  const double* frames; // (n_frames, n, 3)
  long units_per_frame; // n_tiles (n_tiles + 1) / 2
};

template <bool PERIODIC>
__device__ __forceinline__ void hist_pair(const PairHistArgs& a, unsigned* hist, double dx, double dy, double dz, bool mine) {
  dx = image<PERIODIC>(a.Lx, a.iLx, dx);
  dy = image<PERIODIC>(a.Ly, a.iLy, dy);
  dz = image<PERIODIC>(a.Lz, a.iLz, dz);
  const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
  if (mine && r2 < a.r_max2) {
    // r = r2 rsqrt(r2); the floor keeps rsqrt finite at coincident points (r = 0 * 1e150 = 0) and changes no other r
    const double r = r2 * rsqrt_f64(fmax(r2, 1e-300));
    int bin = (int)(r * a.inv_dr);
    bin = bin < a.n_bins ? bin : a.n_bins - 1;      // r < r_max up to the last rounding: never past the counters
    atomicAdd(&hist[bin], 1u);
  }
}

// The histogram as a policy of the pair-once frame (pair_once_kernels.h): no step-0 term, one pair body
template <bool PERIODIC, bool BATCH>
struct PairHistOp {
  typedef PairHistArgs Args;
  struct Lane { unsigned* hist; };      // the workgroup's LDS counters
  static constexpr bool FRAMES = BATCH;
  static constexpr double PAD_W = 0.0;      // record .w is not used
  static __device__ __forceinline__ double4 fetch(const Args& a, long frame, long i) {
    if constexpr (BATCH) {
      const double* p = a.frames + 3 * (frame * a.n + i);
      return make_double4(p[0], p[1], p[2], 0.0);
    } else {
      const double4 p = a.pos[i];
      return make_double4(p.x, p.y, p.z, 0.0);
    }
  }
  static __device__ __forceinline__ bool culled(const Args& a, int I, int J) {
    if constexpr (BATCH) return false;      // no bounds
    else return tile_gap2(a.bounds, I, J, PERIODIC ? a.Lx : 0.0, PERIODIC ? a.Ly : 0.0, PERIODIC ? a.Lz : 0.0) > a.cull2;
  }
  static __device__ __forceinline__ void diag_start(const Args&, Lane&, const double4&, bool) {}
  static __device__ __forceinline__ bool guarded(const Args&, int, int) { return false; }
  template <bool GUARDED>
  static __device__ __forceinline__ void pair(const Args& a, Lane& st, const double4& self, const double4& q, bool take) {
    hist_pair<PERIODIC>(a, st.hist, self.x - q.x, self.y - q.y, self.z - q.z, take);
  }
};

template <bool PERIODIC, bool BATCH>
__global__ __launch_bounds__(64 * kSymWaves) void pair_hist_kernel(const PairHistArgs a) {
  typedef PairHistOp<PERIODIC, BATCH> OP;
  __shared__ double4 rec_all[kSymWaves][64];
  extern __shared__ unsigned hist[];      // [n_bins]
  for (int b = threadIdx.x; b < a.n_bins; b += 64 * kSymWaves) hist[b] = 0u;
  __syncthreads();
  typename OP::Lane st{hist};
  pair_once_sweep<OP>(a, st, rec_all[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
  __syncthreads();
  for (int b = threadIdx.x; b < a.n_bins; b += 64 * kSymWaves) {
    const unsigned v = hist[b];
    if (v) atomicAdd(&a.hist[b], (unsigned long long)v);
  }
}

}  // namespace rmb
