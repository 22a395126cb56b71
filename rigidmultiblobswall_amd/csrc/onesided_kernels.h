// onesided_kernels.h -- the frame of every one-sided sweep (gfx950): mobility, blob-blob forces, source -> target with
// radii, pressure / Stokes double layer, Laplace layer operators.  Written once here; an operator is a policy class.
//
// Decomposition (MI355X-first, not the reference's "one CUDA thread per target reading every source from global
// memory", mobility/mobility_pycuda.py:150-254):
//   * a workgroup = 256 threads = 4 wave64 = one wave per SIMD of a CU;
//   * lane l of EVERY wave owns target  i = tgt_begin + 64*blockIdx.x + l  (its state lives in registers);
//   * blockIdx.y selects a contiguous chunk of sources; the chunk is streamed through an LDS tile of 512 records
//     staged with coalesced loads (whatever can be folded into a record is folded there, once per source);
//   * the 4 waves split each tile's sources 4-ways (wave w takes records w, w+4, ...), read them as wave-uniform
//     (broadcast) ds_read_b128, and accumulate in registers;
//   * the 4 partial sums are combined through LDS in a fixed order; with one chunk the result is finished in place
//     (OP::store: self term, prefactor, ...), otherwise partials go to a workspace [n_chunks][NOUT][n_tgt_pad] and a
//     small second kernel sums the chunks in fixed order and runs the same OP::store -> deterministic, atomic-free,
//     bit-reproducible for a given chunk count.
// So N=1e4 still yields ~2000 workgroups (157 target tiles x 13 chunks) instead of 157 waves.
//
// The policy OP supplies (all static, every function __device__ __forceinline__):
//   Args            kernel argument struct, derived from OneSidedArgs
//   NOUT, REC2      doubles per target of the result; double2 per source record of the tile
//   SHARDED         targets are [tgt_begin, tgt_end) of the sources' own array (multi-GPU shard); else tgt_begin is 0
//   SKIP_OWN_TILE   the pair t == s is left out BY INDEX, and the test runs only in the one source tile that overlaps
//                   the workgroup's own 64 targets: tile_pairs<true> there, tile_pairs<false> (no test) everywhere else.
//                   Operators that test every pair (by distance, or by index as the force sweep) or none leave it false.
//   Target          what a lane keeps of its target;  load_target(a, t)
//   stage(a, j, rec)                                      source j -> its record
//   tile_pairs<OWN>(a, tile, n, wave, j0, ti, tg, acc)    this wave's records of a tile of n (first source j0) onto acc
//   store(a, ti, tg, acc)                                 epilogue + store of target ti from the summed acc
#pragma once
#include "pair_ops.h"

namespace rmb {

constexpr int kTile = 512;  // source records per LDS tile

struct OneSidedArgs {
  double* out;              // [NOUT (tgt_end - tgt_begin)] final output (AoS)
  double* partial;          // [n_chunks][NOUT][n_tgt_pad] chunk partials, used when n_chunks > 1
  long n_src;
  long tgt_begin, tgt_end;  // target index range (0, n_tgt unless OP::SHARDED)
  long n_tgt_pad;           // 64 * gridDim.x
  long chunk_len;           // sources per chunk (multiple of kWaves)
  int n_chunks;
};

template <class OP>
__device__ __forceinline__ void one_sided_sweep(const typename OP::Args& a) {
  constexpr int NOUT = OP::NOUT, R2 = OP::REC2;
  __shared__ double2 tile[kTile * R2];
  __shared__ double red[(kWaves - 1) * NOUT * 64];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the source loop index stays scalar
  const long tb = (OP::SHARDED ? a.tgt_begin : 0) + 64L * blockIdx.x;
  const long ti = tb + lane;
  const bool valid = ti < a.tgt_end;
  const typename OP::Target tg = OP::load_target(a, valid ? ti : a.tgt_end - 1);

  const long c0 = (long)blockIdx.y * a.chunk_len;
  long c1 = c0 + a.chunk_len;
  if (c1 > a.n_src) c1 = a.n_src;

  double acc[NOUT];
#pragma unroll
  for (int c = 0; c < NOUT; ++c) acc[c] = 0.0;
  for (long j0 = c0; j0 < c1; j0 += kTile) {
    const int n = (int)((c1 - j0 < kTile) ? (c1 - j0) : kTile);
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += kBlock) OP::stage(a, j0 + t, tile + t * R2);
    __syncthreads();
    if constexpr (OP::SKIP_OWN_TILE) {
      if (j0 < tb + 64 && tb < j0 + n) OP::template tile_pairs<true>(a, tile, n, wave, j0, ti, tg, acc);
      else                             OP::template tile_pairs<false>(a, tile, n, wave, j0, ti, tg, acc);
    } else {
      OP::template tile_pairs<false>(a, tile, n, wave, j0, ti, tg, acc);
    }
  }

  // combine the 4 waves (fixed order 0+1+2+3)
  if (wave > 0) {
    double* r = red + (wave - 1) * NOUT * 64;
#pragma unroll
    for (int c = 0; c < NOUT; ++c) r[c * 64 + lane] = acc[c];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 0; w < kWaves - 1; ++w) {
    const double* r = red + w * NOUT * 64;
#pragma unroll
    for (int c = 0; c < NOUT; ++c) acc[c] += r[c * 64 + lane];
  }
  if (a.n_chunks == 1) {
    if (valid) OP::store(a, ti, tg, acc);
  } else {
    double* p = a.partial + (long)blockIdx.y * NOUT * a.n_tgt_pad + (64L * blockIdx.x + lane);
#pragma unroll
    for (int c = 0; c < NOUT; ++c) p[c * a.n_tgt_pad] = acc[c];
  }
}

// Second pass when the sources were split into chunks (256 threads, one per target): fixed-order sum over the chunks,
// then the operator's epilogue.
template <class OP>
__device__ __forceinline__ void one_sided_finalize(const typename OP::Args& a) {
  constexpr int NOUT = OP::NOUT;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long ti = (OP::SHARDED ? a.tgt_begin : 0) + t;
  if (ti >= a.tgt_end) return;
  double s[NOUT];
#pragma unroll
  for (int c = 0; c < NOUT; ++c) s[c] = 0.0;
  for (int k = 0; k < a.n_chunks; ++k) {
    const double* p = a.partial + (long)k * NOUT * a.n_tgt_pad + t;
#pragma unroll
    for (int c = 0; c < NOUT; ++c) s[c] += p[c * a.n_tgt_pad];
  }
  OP::store(a, ti, OP::load_target(a, ti), s);
}

__device__ __forceinline__ double wrap_nearest(double r, double L, double invL) {
  // r - trunc(r/L + 0.5 sgn(r)) L          (mobility/mobility_numba.py:184-192)
  const double q = r * invL;
  const double h = (r > 0.0) ? 0.5 : ((r < 0.0) ? -0.5 : 0.0);
  return __builtin_fma(-__builtin_trunc(q + h), L, r);
}

// The 3^d images of one pair under pseudo-periodic boundaries (a.Lx, a.Ly, a.Lz > 0 on the periodic axes, a.iL* = 1/L):
// nearest image on every periodic axis, then one box either way.  f(dx, dy, dz, central); central = the nearest image.
template <class A, class F>
__device__ __forceinline__ void periodic_images(const A& a, double dx, double dy, double dz, F f) {
  const int px = a.Lx > 0, py = a.Ly > 0, pz = a.Lz > 0;
  if (px) dx = wrap_nearest(dx, a.Lx, a.iLx);
  if (py) dy = wrap_nearest(dy, a.Ly, a.iLy);
  if (pz) dz = wrap_nearest(dz, a.Lz, a.iLz);
  for (int bx = -px; bx <= px; ++bx)
    for (int by = -py; by <= py; ++by)
      for (int bz = -pz; bz <= pz; ++bz) f(dx + bx * a.Lx, dy + by * a.Ly, dz + bz * a.Lz, bx == 0 && by == 0 && bz == 0);
}

}  // namespace rmb
