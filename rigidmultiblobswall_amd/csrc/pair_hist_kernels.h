// pair_hist_kernels.h -- histogram of the pair distances of a point configuration (gfx950, fp64): the counts behind the
// radial distribution function g(r).
//
// The reference's g(r) program (multi_bodies/examples/Radial_Dist_Test/gr_pseudo2D_single_blob.cpp) is a single-threaded
// loop over frames and pairs i < j: minimal image, r = sqrt(dx^2 + dy^2 + dz^2), bin = int(r / dr), hist[bin] += 2 while
// bin < n_bins.  Here every unordered pair is met once on the schedule of potential_kernel (potential_kernels.h): a work
// unit is a tile pair I <= J, lane = point of tile I, tile J staged in the wave's LDS slab and read by rotation; the same
// unit_seek / unit_next (sym_schedule.h), strided chunks and tile_gap2 culling; on a diagonal unit steps 1..32, step 32
// taken by the lower half.  Instead of summing, a pair with r < r_max adds ONE count (the unordered pair) to bin
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
#include "pair_ops.h"
#include "sym_schedule.h"

namespace rmb {

constexpr int kPairHistMaxBins = 8192;      // 32 KB of LDS counters

struct PairHistArgs {
  const double4* pos;   // resident: packed raw positions (caller's order, or the Morton-sorted copy)
  const double* bounds; // resident: [n_tiles][6] tile bounding boxes of `pos`
  double cull2;         // resident: r_max^2, +inf = no culling
  long n;               // points (per frame)
  int n_tiles;
  int order, xcd;
  long chunk_steps;     // > 0: steps per strided chunk of a wave; 0: one contiguous range per wave
  long step_end;        // n_units * 64 (BATCH: n_frames * units_per_frame * 64)
  double Lx, Ly, iLx, iLy, Lz, iLz;
  double r_max2, inv_dr;   // r_max^2 and n_bins / r_max
  int n_bins;
  unsigned long long* hist;   // [n_bins], added to
  // BATCH only
  const double* frames; // (n_frames, n, 3)
  long units_per_frame; // n_tiles (n_tiles + 1) / 2
};

// minimal image of one separation component (L <= 0: open direction); sentinels pass through
template <bool PERIODIC>
__device__ __forceinline__ double hist_image(double L, double iL, double d) {
  if constexpr (PERIODIC) {
    if (L > 0) d = wrap_nearest_pad_safe(d, L, iL);
  }
  return d;
}

template <bool PERIODIC>
__device__ __forceinline__ void hist_pair(const PairHistArgs& a, unsigned* hist, double dx, double dy, double dz, bool mine) {
  dx = hist_image<PERIODIC>(a.Lx, a.iLx, dx);
  dy = hist_image<PERIODIC>(a.Ly, a.iLy, dy);
  dz = hist_image<PERIODIC>(a.Lz, a.iLz, dz);
  const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
  if (mine && r2 < a.r_max2) {
    // r = r2 rsqrt(r2); the floor keeps rsqrt finite at coincident points (r = 0 * 1e150 = 0) and changes no other r
    const double r = r2 * rsqrt_f64(fmax(r2, 1e-300));
    int bin = (int)(r * a.inv_dr);
    bin = bin < a.n_bins ? bin : a.n_bins - 1;      // r < r_max up to the last rounding: never past the counters
    atomicAdd(&hist[bin], 1u);
  }
}

template <bool PERIODIC, bool BATCH>
__global__ __launch_bounds__(64 * kSymWaves) void pair_hist_kernel(const PairHistArgs a) {
  __shared__ double4 rec_all[kSymWaves][64];
  extern __shared__ unsigned hist[];      // [n_bins]
  for (int b = threadIdx.x; b < a.n_bins; b += 64 * kSymWaves) hist[b] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double4* rec = rec_all[wave];
  const long n_waves = (long)gridDim.x * kSymWaves;
  const long w = (a.xcd ? xcd_swizzle(blockIdx.x, gridDim.x) : (long)blockIdx.x) * kSymWaves + wave;
  const long spw = a.chunk_steps > 0 ? a.chunk_steps : (a.step_end + n_waves - 1) / n_waves;
  for (long chunk = w;; chunk += n_waves) {
    long s = chunk * spw;
    if (s >= a.step_end) break;
    long s_end = s + spw;
    if (s_end > a.step_end) s_end = a.step_end;
    int I = 0, J = 0;
    long frame = 0;
    if constexpr (BATCH) {
      frame = (s >> 6) / a.units_per_frame;
      unit_seek(0, (s >> 6) - frame * a.units_per_frame, a.n_tiles, I, J);
    } else {
      unit_seek(a.order, s >> 6, a.n_tiles, I, J);
    }
    int I_cur = -1;
    double xi = 0, yi = 0, zi = 0;
    bool vi_ok = false;
    while (s < s_end) {
      const int k0 = (int)(s & 63);
      const long left = s_end - s;
      const int k1 = (left < 64 - k0) ? (int)(k0 + left) : 64;
      s += k1 - k0;
      const bool diag = (I == J);
      // diagonal unit: steps 1..32 = every unordered pair of the tile once (lane l meets l + k; at k = 32 both lanes of
      // a pair would meet: the lower half takes it), 0 and 33..63 empty
      bool idle = diag && k0 > 32;
      if constexpr (!BATCH) {
        if (!diag) idle = tile_gap2(a.bounds, I, J, PERIODIC ? a.Lx : 0.0, PERIODIC ? a.Ly : 0.0, PERIODIC ? a.Lz : 0.0) > a.cull2;
      }
      if (!idle) {
        if (I != I_cur) {
          I_cur = I;
          const long i = 64L * I + lane;
          vi_ok = i < a.n;
          xi = 1e100; yi = 1e100; zi = 1e100;
          if (vi_ok) {
            if constexpr (BATCH) {
              const double* p = a.frames + 3 * (frame * a.n + i);
              xi = p[0]; yi = p[1]; zi = p[2];
            } else {
              const double4 p = a.pos[i];
              xi = p.x; yi = p.y; zi = p.z;
            }
          }
        }
        if (!diag) {
          const long j = 64L * J + lane;
          double4 p = make_double4(-1e100, -1e100, -1e100, 0.0);
          if (j < a.n) {
            if constexpr (BATCH) {
              const double* q = a.frames + 3 * (frame * a.n + j);
              p.x = q[0]; p.y = q[1]; p.z = q[2];
            } else {
              p = a.pos[j];
            }
          }
          rec[lane] = p;
        } else {
          rec[lane] = make_double4(vi_ok ? xi : -1e100, vi_ok ? yi : -1e100, vi_ok ? zi : -1e100, 0.0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int kb = (diag && k0 < 1) ? 1 : k0;
        const int ke = (diag && k1 > 33) ? 33 : k1;
        // step 32 of a diagonal unit is met from both of its lanes: it is peeled off the loop and taken by the lower half
        const bool peel = diag && kb <= 32 && ke > 32;
        const int kl = peel ? 32 : ke;
        for (int k = kb; k < kl; ++k) {
          const double4 q = rec[(lane + k) & 63];
          hist_pair<PERIODIC>(a, hist, xi - q.x, yi - q.y, zi - q.z, true);
        }
        if (peel) {
          const double4 q = rec[(lane + 32) & 63];
          hist_pair<PERIODIC>(a, hist, xi - q.x, yi - q.y, zi - q.z, lane < 32);
        }
        __builtin_amdgcn_wave_barrier();   // rec is rewritten by the next unit
      }
      if (k1 == 64) {
        unit_next(BATCH ? 0 : a.order, a.n_tiles, I, J);
        if constexpr (BATCH) {
          if (I == a.n_tiles) { I = 0; J = 0; ++frame; I_cur = -1; }      // first unit of the next frame
        }
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < a.n_bins; b += 64 * kSymWaves) {
    const unsigned v = hist[b];
    if (v) atomicAdd(&a.hist[b], (unsigned long long)v);
  }
}

}  // namespace rmb
