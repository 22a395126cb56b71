// sym_schedule.h -- the schedule of the symmetric (each unordered pair once) sweeps, and only the schedule: which tile
// pair a wave works on (unit_seek / unit_next on the tile triangle, unit2_seek / unit2_next on the row-pair grid of the
// two-targets-per-lane kernels; row-major and blocked order), the XCD-aware workgroup numbering, the nearest-image helpers
// and the tile bounds / tile gap of the culling sweeps (forces, potential).  No sweep kernel is defined here.
//
// Everything above the __HIPCC__ block is plain arithmetic and also compiles for the host (g++ with __device__,
// __host__ and __forceinline__ defined away): tests/test_unit_order_host.py checks the unit orders exhaustively that
// way, and the launchers take units2_total from here.
#pragma once
#include <cmath>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace rmb {

__device__ __forceinline__ double wrap_nearest_sym(double r, double L, double invL) {
  const double q = r * invL;
  const double h = (r > 0.0) ? 0.5 : ((r < 0.0) ? -0.5 : 0.0);
  return __builtin_fma(-__builtin_trunc(q + h), L, r);
}

// Nearest image that leaves the padding sentinels (+-1e100) alone: wrapped, a sentinel can land exactly on a real
// blob (fma(-trunc(1e100/L), L, 1e100) == 0 for power-of-two L) and 1/r = inf would reach the accumulators.
__device__ __forceinline__ double wrap_nearest_pad_safe(double r, double L, double invL) {
  const double w = wrap_nearest_sym(r, L, invL);
  return (__builtin_fabs(r) < 1e50) ? w : r;
}

__device__ __forceinline__ void unit_to_tiles(long u, int T, int& I, int& J) {
  // row-major over the upper triangle: row I holds (T - I) units
  const double tt = 2.0 * T + 1.0;
  long i = (long)((tt - sqrt(tt * tt - 8.0 * (double)u)) * 0.5);
  if (i < 0) i = 0;
  if (i > T - 1) i = T - 1;
  while (i > 0 && i * T - i * (i - 1) / 2 > u) --i;
  while ((i + 1) * T - (i + 1) * i / 2 <= u) ++i;
  I = (int)i;
  J = (int)(u - (i * T - i * (i - 1) / 2) + i);
}

// ---- unit order and workgroup placement (round 4) ------------------------------------------------------------
// order 0: row-major over the tile triangle (what the deterministic mode's ordered reduction assumes).
// order 1: BLOCKED -- the triangle is cut into super-blocks of 32 x 32 tiles; super-blocks in row-major order, and
//   inside a super-block the units in row-major order (the triangle I <= J inside a diagonal one).  Waves that work on
//   neighbouring step ranges then touch the same 64 tiles for ~1000 units instead of sweeping a whole row of the
//   triangle, and with the XCD-aware numbering below those waves sit behind ONE L2: the tile-J loads (3.6 KB per 4096
//   pairs, all of them L2 misses at >= 1e5 blobs in row-major order) mostly hit.
constexpr int kOrdShift = 5;
constexpr int kOrdB = 1 << kOrdShift;

__device__ __forceinline__ long blk_units_before_row(long P, long T) {   // super-rows before P are all kOrdB tall
  const long B = kOrdB;
  return P * (B * (B + 1) / 2) + B * (P * T - B * (P * (P + 1) / 2));
}

__device__ __forceinline__ void unit_seek(int order, long u, int T, int& I, int& J) {
  if (order == 0) { unit_to_tiles(u, T, I, J); return; }
  const int SB = (T + kOrdB - 1) >> kOrdShift;
  int lo = 0, hi = SB - 1;
  while (lo < hi) {                       // largest super-row whose first unit is <= u
    const int mid = (lo + hi + 1) >> 1;
    if (blk_units_before_row(mid, T) <= u) lo = mid; else hi = mid - 1;
  }
  const int P = lo;
  long rem = u - blk_units_before_row(P, T);
  const int sP = (T - (P << kOrdShift)) < kOrdB ? (T - (P << kOrdShift)) : kOrdB;
  const long triP = (long)sP * (sP + 1) / 2;
  if (rem < triP) {                       // diagonal super-block: row-major triangle of sP tiles
    int li, lj;
    unit_to_tiles(rem, sP, li, lj);
    I = (P << kOrdShift) + li; J = (P << kOrdShift) + lj;
    return;
  }
  rem -= triP;
  const long per = (long)sP * kOrdB;      // every super-block right of the diagonal but the last is kOrdB wide
  const int q = (int)(rem / per);
  const int Q = P + 1 + q;
  const int wQ = (T - (Q << kOrdShift)) < kOrdB ? (T - (Q << kOrdShift)) : kOrdB;
  const long rem2 = rem - (long)q * per;
  const int li = (int)(rem2 / wQ);
  I = (P << kOrdShift) + li;
  J = (Q << kOrdShift) + (int)(rem2 - (long)li * wQ);
}

__device__ __forceinline__ void unit_next(int order, int T, int& I, int& J) {
  if (order == 0) {
    if (++J == T) { ++I; J = I; }
    return;
  }
  const int P = I >> kOrdShift, Q = J >> kOrdShift;
  const int row_end = ((P + 1) << kOrdShift) < T ? ((P + 1) << kOrdShift) : T;
  const int col_end = ((Q + 1) << kOrdShift) < T ? ((Q + 1) << kOrdShift) : T;
  if (++J < col_end) return;                                     // same row of the same super-block
  if (++I < row_end) { J = (P == Q) ? I : (Q << kOrdShift); return; }   // next row of the same super-block
  if (((Q + 1) << kOrdShift) < T) { I = P << kOrdShift; J = (Q + 1) << kOrdShift; return; }   // next super-block of the super-row
  I = (P + 1) << kOrdShift; J = I;                                // diagonal super-block of the next super-row
}

// XCD-aware numbering of the workgroups (cdna_hip_programming.md, T1): blocks are dealt round-robin over the 8 XCDs,
// so blocks b and b + 8 share an L2; this bijection gives every XCD one CONTIGUOUS eighth of the numbering, i.e. of the
// step range.  A speed choice only: any placement is correct.
__device__ __forceinline__ long xcd_swizzle(long bid, long nwg) {
  const long q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// ---- unit order of the row-pair grid (two target blobs per lane: sym2t_kernels.h, symx2t_kernels.h) ----------------------
// units of the row-pair grid: sum over pairs p of (T - 2p)
__host__ __device__ inline long units2_before_pair(long p, long T) { return p * T - p * (p - 1); }
__host__ __device__ inline long units2_total(long T) { return units2_before_pair((T + 1) / 2, T); }

// order 0: pair by pair, J ascending.  order 1: the blocked order above on this grid -- super-blocks of
// 16 row pairs (32 tile rows) x 32 tile columns, walked super-row by super-row, pair by pair inside a super-block (the
// diagonal super-block is the staircase J >= 2p), so that waves which run at the same time share tiles in L2.
constexpr int kOrd2Pairs = 1 << (kOrdShift - 1);     // row pairs per super-block

// units before super-row B (all earlier super-rows are full): 16 B (T + 1 - 16 B)
__host__ __device__ inline long blk2_units_before_row(long B, long T) { return (long)kOrd2Pairs * B * (T + 1 - (long)kOrd2Pairs * B); }

__device__ __forceinline__ void unit2_seek(int order, long u, int T, int& p, int& J) {
  const double b = (double)T + 1.0;
  double disc = b * b - 4.0 * (double)u;
  if (disc < 0.0) disc = 0.0;
  const double y = (b - sqrt(disc)) * 0.5;             // smaller root of y (T + 1 - y) = u
  if (order == 0) {
    long q = (long)y;
    const long P = ((long)T + 1) / 2;
    if (q < 0) q = 0;
    if (q > P - 1) q = P - 1;
    while (q > 0 && units2_before_pair(q, T) > u) --q;
    while (q + 1 < P && units2_before_pair(q + 1, T) <= u) ++q;
    p = (int)q;
    J = (int)(2 * q + (u - units2_before_pair(q, T)));
    return;
  }
  const long NB = ((long)T + (1 << kOrdShift) - 1) >> kOrdShift;     // super-rows
  long B = (long)(y / kOrd2Pairs);
  if (B < 0) B = 0;
  if (B > NB - 1) B = NB - 1;
  while (B > 0 && blk2_units_before_row(B, T) > u) --B;
  while (B + 1 < NB && blk2_units_before_row(B + 1, T) <= u) ++B;
  long rem = u - blk2_units_before_row(B, T);
  const int row0 = (int)(B << kOrdShift);                               // first tile row (and first tile column) of the diagonal super-block
  const int w = (T - row0) < (1 << kOrdShift) ? (T - row0) : (1 << kOrdShift);
  const int sP = (w + 1) / 2;                                           // row pairs of this super-row
  const long tri = (long)sP * w - (long)sP * (sP - 1);
  if (rem < tri) {                                                      // diagonal super-block: pair lp has the columns 2 lp .. w - 1
    int lp = 0;
    while (lp + 1 < sP && (long)(lp + 1) * w - (long)(lp + 1) * lp <= rem) ++lp;
    const long before = (long)lp * w - (long)lp * (lp - 1);
    p = (int)(B * kOrd2Pairs) + lp;
    J = row0 + 2 * lp + (int)(rem - before);
    return;
  }
  rem -= tri;
  const int col0 = row0 + (1 << kOrdShift);                             // first column right of the diagonal super-block
  const long per = (long)sP << kOrdShift;                               // units of a full-width super-block
  const long q = rem / per;
  const int c0 = col0 + (int)(q << kOrdShift);
  const int wQ = (T - c0) < (1 << kOrdShift) ? (T - c0) : (1 << kOrdShift);
  const long rem2 = rem - q * per;
  const int lp = (int)(rem2 / wQ);
  p = (int)(B * kOrd2Pairs) + lp;
  J = c0 + (int)(rem2 - (long)lp * wQ);
}

__device__ __forceinline__ void unit2_next(int order, int T, int& p, int& J) {
  if (order == 0) {
    if (++J < T) return;
    ++p;
    J = 2 * p;
    return;
  }
  const int B = p / kOrd2Pairs, Q = J >> kOrdShift;
  const int col_end = ((Q + 1) << kOrdShift) < T ? ((Q + 1) << kOrdShift) : T;
  const int P = (T + 1) / 2;
  const int pair_end = (B + 1) * kOrd2Pairs < P ? (B + 1) * kOrd2Pairs : P;
  if (++J < col_end) return;                                            // same pair, same super-block
  if (++p < pair_end) { J = (Q == B) ? 2 * p : (Q << kOrdShift); return; }   // next pair of the super-block
  if (((Q + 1) << kOrdShift) < T) { p = B * kOrd2Pairs; J = (Q + 1) << kOrdShift; return; }   // next super-block of the super-row
  p = (B + 1) * kOrd2Pairs;                                             // next super-row: its diagonal super-block
  J = 2 * p;
}

// Lower bound of the squared distance between any blob of tile I and any blob of tile J (wave-uniform: every lane
// reads the same twelve doubles).  Per direction the separations x_j - x_i fill the interval [lo_J - hi_I, hi_J - lo_I];
// in a pseudo-periodic direction (L > 0) the pair force takes the nearest image of every separation
// (d - rint(d/L) L, positions need not lie in one cell), so the interval is first moved by the multiple of L that
// centres it: it then lies inside (-L, L), and |nearest image| over it is smallest at the end nearer to zero -- or
// zero if the interval contains zero or is at least L long.  `nd` = 2 leaves the z term out (distances taken in the plane).
__device__ __forceinline__ double tile_gap2(const double* bounds, int I, int J, double Lx = 0.0, double Ly = 0.0, double Lz = 0.0, int nd = 3) {
  const double* bi = bounds + 6L * I;
  const double* bj = bounds + 6L * J;
  const double L[3] = {Lx, Ly, Lz};
  double g2 = 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d >= nd) continue;
    double lo = bj[d] - bi[3 + d], hi = bj[3 + d] - bi[d];
    if (L[d] > 0.0) {
      if (hi - lo >= L[d]) { lo = 0.0; hi = 0.0; }
      else {
        const double shift = __builtin_rint(0.5 * (lo + hi) / L[d]) * L[d];
        lo -= shift; hi -= shift;
      }
    }
    const double g = lo > 0.0 ? lo : (hi < 0.0 ? -hi : 0.0);
    g2 = __builtin_fma(g, g, g2);
  }
  return g2;
}

#ifdef __HIPCC__
// bounding box of every 64-blob tile of the packed positions; one wave per tile
// (static: this header is part of every translation unit of the symmetric family)
static __global__ __launch_bounds__(64) void tile_bounds_kernel(const double4* pos, long n, double* bounds) {
  const long T = blockIdx.x;
  const long i = 64 * T + threadIdx.x;
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  if (i < n) {
    const double4 p = pos[i];
    lo[0] = hi[0] = p.x; lo[1] = hi[1] = p.y; lo[2] = hi[2] = p.z;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d)
    for (int off = 32; off > 0; off >>= 1) {
      lo[d] = fmin(lo[d], __shfl_xor(lo[d], off));
      hi[d] = fmax(hi[d], __shfl_xor(hi[d], off));
    }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { bounds[6 * T + d] = lo[d]; bounds[6 * T + 3 + d] = hi[d]; }
  }
}
#endif  // __HIPCC__

}  // namespace rmb
