// lag_sweep_kernels.h -- the frame of the lag sweeps in which a LANE OWNS A LAG (gfx950, fp64): the 6 x 6 mean-square
// displacement (msd_kernels.h) and the scattering lag sums (scattering_kernels.h).  Written once here; a sweep is a policy
// class.  No kernel is defined.
//
// Records: R doubles per (series, frame), series-major and time-contiguous, rec[((y B + b) F + f) R + k] for row y (the
// launch's gridDim.y), series b < B of the row and frame f < F.  For origins o in [o_begin, o_end) and lags l < n_lags a
// lane keeps NS sums over the pairs (record o + l, record o) of all series of its row.
//
// Schedule.  Workgroup blockIdx.x = p lag_blocks + lb of row blockIdx.y serves the 64 lags l0 = 64 lb .. l0 + 63 (lane =
// lag - l0) and the work items [items p / P, items (p + 1) / P); item = b n_chunks + ch is origin chunk ch of series b,
// the origins o0 = o_begin + ch chunk .. o1 = min(o0 + chunk, o_end).  Per item the lagged records f = o0 + l0 .. o0 + l0
// + chunk + 62 of the series -- a sliding, unit-stride window -- are staged in LDS component by component (win[k][j], W =
// chunk + 63 columns; lane l reads win[k][o - o0 + l]: 64 consecutive doubles, conflict-free ds_read_b64), zeros past the
// last frame, so no read leaves the records.  The origin record is wave-uniform and comes through the scalar cache.  Wave
// w of the four takes the origins o0 + w, o0 + w + 4, ...  No cross-lane reduction, no LDS accumulator, no atomic.
// Lanes with l0 + lane >= n_lags compute sums nobody reads.
//
// Order of additions (the bits depend on it, and "the same call gives the same bits" rests on it):
//   1. a lane's sum: items ascending, within an item its wave's origins ascending, one OP::pair per origin;
//   2. the workgroup's sum: the four waves in wave order through one LDS slab, ((w0 + w1) + w2) + w3, written as
//      part[(y gridDim.x + blockIdx.x) NS 64 + slot 64 + lane];
//   3. the lag's sum (lag_sweep_partial_sum, for the finishing kernels): from 0.0, the P partials of its lag block in
//      block order p = 0 .. P - 1.
//
// The policy OP supplies (all static):
//   Args        kernel argument struct, derived from LagSweepArgs
//   R           doubles per record
//   NS          sums per lane
//   MASK_TAIL   a staged zero record does NOT add exactly nothing: the frame runs the unmasked loop over the origins that
//               have all 64 lags of the block inside the trajectory (o < F - l0 - 63) and the masked copy over the rest
//               (`ok` = o + lag < F).  Without it one unmasked loop.
//   pair<MASKED>(acc, win, W, j, org, ok)   __device__ __forceinline__: one (origin, lag) pair of a lane, the lagged record
//               at column j of win[R][W], the origin record at org[0 .. R - 1], added to acc[NS]
#pragma once
#include <hip/hip_runtime.h>

namespace rmb {

constexpr int kLagWaves = 4;
constexpr int kLagBlock = 64 * kLagWaves;

// The fields the frame reads; plan_lag_sweep (rmb_internal.h) fills all but rec / part.
struct LagSweepArgs {
  const double* rec;       // [Y][B][F][R]
  long F, B;               // frames, series per row
  long n_lags, lag_blocks;
  long o_begin, o_end;     // origins
  long chunk, n_chunks;    // origins per work item, work items per series
  long items, P;           // B * n_chunks work items over P workgroups per lag block
  double* part;            // [Y][P * lag_blocks][NS][64]
};

// LDS of a sweep: the staged window (chunk + 63 records of R doubles, component-major), re-used for the combine slab [NS][64]
inline size_t lag_sweep_lds(long chunk, int R, int NS) {
  const size_t win = (size_t)(chunk + 63) * R * sizeof(double), slab = (size_t)NS * 64 * sizeof(double);
  return win > slab ? win : slab;
}

// `lds`: the workgroup's dynamic LDS, lag_sweep_lds(a.chunk, OP::R, OP::NS) bytes
template <class OP>
__device__ __forceinline__ void lag_sweep(const typename OP::Args& a, double* lds) {
  constexpr int R = OP::R, NS = OP::NS;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long lb = blockIdx.x % a.lag_blocks, p = blockIdx.x / a.lag_blocks;
  const long l0 = 64 * lb;
  const long W = a.chunk + 63;
  const int Wi = (int)W;
  const long item_begin = a.items * p / a.P, item_end = a.items * (p + 1) / a.P;
  const double* row = a.rec + (size_t)blockIdx.y * a.B * a.F * R;

  double acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = 0.0;

  for (long item = item_begin; item < item_end; ++item) {
    const long b = item / a.n_chunks, ch = item - b * a.n_chunks;
    const long o0 = a.o_begin + ch * a.chunk;
    const long o1 = o0 + a.chunk < a.o_end ? o0 + a.chunk : a.o_end;
    const double* series = row + R * b * a.F;
    // stage records f0 .. f0 + W - 1 (zeros past the last frame): a contiguous run of the series
    const long f0 = o0 + l0;
    const long have = f0 < a.F ? (a.F - f0 < W ? a.F - f0 : W) : 0;
    __syncthreads();      // the previous item's readers are done
    for (long i = threadIdx.x; i < R * W; i += kLagBlock) {
      const long j = i / R, k = i - R * j;
      lds[k * W + j] = j < have ? series[R * f0 + i] : 0.0;
    }
    __syncthreads();
    long o = o0 + wave;
    if constexpr (OP::MASK_TAIL) {
      // origins below o_full have all 64 lags of this block inside the trajectory: no mask in that loop
      const long lag = l0 + lane;
      const long o_full = a.F - l0 - 63;
      const long o_split = o1 < o_full ? o1 : o_full;
      for (; o < o_split; o += kLagWaves) OP::template pair<false>(acc, lds, Wi, (int)(o - o0) + lane, series + R * o, true);
      for (; o < o1; o += kLagWaves) OP::template pair<true>(acc, lds, Wi, (int)(o - o0) + lane, series + R * o, o + lag < a.F);
    } else {
      for (; o < o1; o += kLagWaves) OP::template pair<false>(acc, lds, Wi, (int)(o - o0) + lane, series + R * o, true);
    }
  }

  // the four waves add their sums in wave order through one slab
  for (int w = 0; w < kLagWaves; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < NS; ++t) lds[t * 64 + lane] = w == 0 ? acc[t] : lds[t * 64 + lane] + acc[t];
    }
  }
  __syncthreads();
  double* out = a.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (NS * 64);
  for (int i = threadIdx.x; i < NS * 64; i += kLagBlock) out[i] = lds[i];
}

// sum `slot` of lag 64 lb + lane in row `row`: the partials of the P workgroups of its lag block in block order
template <int NS>
__device__ __forceinline__ double lag_sweep_partial_sum(const LagSweepArgs& a, long row, long lb, int slot, int lane) {
  const double* in = a.part + ((size_t)(row * a.P * a.lag_blocks + lb) * NS + slot) * 64 + lane;
  double sum = 0.0;
  for (long p = 0; p < a.P; ++p) sum += in[(size_t)p * a.lag_blocks * (NS * 64)];
  return sum;
}

}  // namespace rmb
