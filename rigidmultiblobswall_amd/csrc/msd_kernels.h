// msd_kernels.h -- 6 x 6 translational-rotational mean-square displacement of rigid-body trajectories (gfx950, fp64).
//
// The reference (general_application_utils.py: calc_total_msd_from_matrix_and_center, calc_msd_data_from_trajectory) is an
// interpreted loop over frames x lags of ONE body: rotation matrices, three np.cross and one np.outer per pair.  Here, for
// frames f = 0 .. F-1 of N bodies (rows x y z s p1 p2 p3), origins o and lags l,
//
//   Delta = [ c_b(o + l) - c_b(o) ;  u ],   c_b(f) = x_b(f) + R(q_b(f)) p_b,
//   u     = 1/2 sum_i (R(q_b(o)) e_i) x (R(q_b(o + l)) e_i)  =  2 s_rel v_rel,   (s_rel, v_rel) = q(o + l) (x) conj(q(o)),
//
// and S[l] = sum_o sum_b Delta Delta^T.  The quaternion form of u is the one computed; the two agree for unit quaternions,
// and quaternions are used as they are, never renormalised.
//
//   msd_record_kernel   one thread per (frame, body): tracked point and quaternion, 7 doubles, written body-major and
//                       time-contiguous (rec[(b F + f) 7 + k]); R(q) p is computed here, once per (frame, body).
//   msd_sweep_kernel    a LANE OWNS A LAG.  A workgroup serves one block of 64 consecutive lags and a contiguous range of
//                       work items (body, origin chunk).  Per item the lagged records f = o0 + l0 .. o0 + l0 + C + 62 of the
//                       body -- a sliding, unit-stride window of its series -- are staged in LDS component by component
//                       (win[k][j]: lane l reads win[k][o - o0 + l], 64 consecutive doubles, conflict-free ds_read_b64);
//                       the origin record is wave-uniform and comes through the scalar cache.  Each of the four waves takes
//                       every fourth origin of the chunk; each lane keeps the 21 sums of the upper triangle in registers
//                       over all its origins and bodies.  No cross-lane reduction, no LDS accumulator, no atomic inside
//                       the loops.  At the end the four waves add their sums in wave order through one LDS slab and the
//                       workgroup writes part[block][t][lane].
//   msd_finish_kernel   adds the partials of a lag in block order INTO the caller's (n_lags, 6, 6) tensor, both triangles.
//
// A lane adds nothing where o + l >= F: frames past the end are staged as zeros (no read leaves the records), a zero
// quaternion gives u = 0 and the translational part is masked (only in the loop over the last origins, where that can happen).  Lanes with l0 + lane >= n_lags compute sums nobody reads.
// The sums of a launch plan are the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>

namespace rmb {

constexpr int kMsdWaves = 4;
constexpr int kMsdBlock = 64 * kMsdWaves;
constexpr int kMsdTri = 21;                 // upper triangle of the 6 x 6 sums
constexpr long kMsdMaxChunk = 1024;         // origins per staged window: (1024 + 63) records of 56 bytes < 64 KB of LDS
constexpr long kMsdPlannedChunk = 256;

struct MsdArgs {
  const double* frames;    // (F, N, 7)
  const double* offsets;   // (N, 3) body-frame tracking offsets, or nullptr
  double* rec;             // (N, F, 7): tracked point, quaternion
  long F, N;
  long n_lags, lag_blocks;
  long o_begin, o_end;     // origins
  long chunk, n_chunks;    // origins per work item, work items per body
  long items, P;           // N * n_chunks work items over P workgroups per lag block
  double* part;            // [P * lag_blocks][21][64]
  double* sums;            // (n_lags, 6, 6), added to
};

// LDS of the sweep: the staged window (chunk + 63 records, component-major), re-used for the combine slab [21][64]
inline size_t msd_sweep_lds(long chunk) {
  const size_t win = (size_t)(chunk + 63) * 7 * sizeof(double), slab = (size_t)kMsdTri * 64 * sizeof(double);
  return win > slab ? win : slab;
}

__global__ __launch_bounds__(256) void msd_record_kernel(const MsdArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // (frame, body), the caller's order: coalesced reads
  if (i >= a.F * a.N) return;
  const long f = i / a.N, b = i - f * a.N;
  const double* in = a.frames + 7 * i;
  double x = in[0], y = in[1], z = in[2];
  const double s = in[3], p1 = in[4], p2 = in[5], p3 = in[6];
  if (a.offsets) {
    // the reference's rotation matrix (quaternion.py: rotation_matrix), applied to the body-frame offset
    const double ox = a.offsets[3 * b], oy = a.offsets[3 * b + 1], oz = a.offsets[3 * b + 2];
    const double d = s * s - 0.5;
    x += 2.0 * ((p1 * p1 + d) * ox + (p1 * p2 - s * p3) * oy + (p1 * p3 + s * p2) * oz);
    y += 2.0 * ((p2 * p1 + s * p3) * ox + (p2 * p2 + d) * oy + (p2 * p3 - s * p1) * oz);
    z += 2.0 * ((p3 * p1 - s * p2) * ox + (p3 * p2 + s * p1) * oy + (p3 * p3 + d) * oz);
  }
  double* out = a.rec + 7 * (b * a.F + f);
  out[0] = x; out[1] = y; out[2] = z; out[3] = s; out[4] = p1; out[5] = p2; out[6] = p3;
}

// One (origin, lag) pair of a lane: the lagged record from the staged window win[7][W] at column j, the origin record `org`
// wave-uniform (scalar loads), the 21 products added to the lane's sums.  MASKED: `ok` is false where the lagged frame is
// past the end -- it was staged as zeros, a zero quaternion makes u = 0 by itself, the translational part is zeroed here.
template <bool MASKED>
__device__ __forceinline__ void msd_pair(double (&acc)[kMsdTri], const double* win, int W, int j, const double* org, bool ok) {
  const double cx = org[0], cy = org[1], cz = org[2], s0 = org[3], ax = org[4], ay = org[5], az = org[6];
  const double s1 = win[3 * W + j], bx = win[4 * W + j], by = win[5 * W + j], bz = win[6 * W + j];
  double d[6];
  d[0] = win[j] - cx;
  d[1] = win[W + j] - cy;
  d[2] = win[2 * W + j] - cz;
  if constexpr (MASKED) {
    d[0] = ok ? d[0] : 0.0; d[1] = ok ? d[1] : 0.0; d[2] = ok ? d[2] : 0.0;
  }
  // q1 (x) conj(q0): s_rel = s1 s0 + b.a, v_rel = s0 b - s1 a - b x a; u = 2 s_rel v_rel.  v_rel in the differences
  // e = b - a, ds = s1 - s0 (b x a = e x a): s0 e - ds a - e x a -- no cancellation of O(1) products for a small
  // rotation, and exactly zero at lag 0
  const double sr = __builtin_fma(bz, az, __builtin_fma(by, ay, __builtin_fma(bx, ax, s1 * s0)));
  const double sr2 = sr + sr;
  const double ds = s1 - s0, ex = bx - ax, ey = by - ay, ez = bz - az;
  const double vx = __builtin_fma(s0, ex, -(ds * ax)) - __builtin_fma(ey, az, -(ez * ay));
  const double vy = __builtin_fma(s0, ey, -(ds * ay)) - __builtin_fma(ez, ax, -(ex * az));
  const double vz = __builtin_fma(s0, ez, -(ds * az)) - __builtin_fma(ex, ay, -(ey * ax));
  d[3] = sr2 * vx; d[4] = sr2 * vy; d[5] = sr2 * vz;
  int t = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int k = i; k < 6; ++k, ++t) acc[t] = __builtin_fma(d[i], d[k], acc[t]);
}

__global__ __launch_bounds__(kMsdBlock) void msd_sweep_kernel(const MsdArgs a) {
  extern __shared__ double msd_lds[];      // win[7][W], W = chunk + 63; later the combine slab [21][64]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long lb = blockIdx.x % a.lag_blocks, p = blockIdx.x / a.lag_blocks;
  const long l0 = 64 * lb;
  const long lag = l0 + lane;
  const long W = a.chunk + 63;
  const int Wi = (int)W;
  const long item_begin = a.items * p / a.P, item_end = a.items * (p + 1) / a.P;

  double acc[kMsdTri];
#pragma unroll
  for (int t = 0; t < kMsdTri; ++t) acc[t] = 0.0;

  for (long item = item_begin; item < item_end; ++item) {
    const long b = item / a.n_chunks, ch = item - b * a.n_chunks;
    const long o0 = a.o_begin + ch * a.chunk;
    const long o1 = o0 + a.chunk < a.o_end ? o0 + a.chunk : a.o_end;
    const double* series = a.rec + 7 * b * a.F;
    // stage records f0 .. f0 + W - 1 (zeros past the last frame): a contiguous run of the body's series
    const long f0 = o0 + l0;
    const long have = f0 < a.F ? (a.F - f0 < W ? a.F - f0 : W) : 0;
    __syncthreads();      // the previous item's readers are done
    for (long i = threadIdx.x; i < 7 * W; i += kMsdBlock) {
      const long j = i / 7, k = i - 7 * j;
      msd_lds[k * W + j] = j < have ? series[7 * f0 + i] : 0.0;
    }
    __syncthreads();
    // origins below o_full have all 64 lags of this block inside the trajectory: no mask in that loop
    const long o_full = a.F - l0 - 63;
    const long o_split = o1 < o_full ? o1 : o_full;
    long o = o0 + wave;
    for (; o < o_split; o += kMsdWaves) msd_pair<false>(acc, msd_lds, Wi, (int)(o - o0) + lane, series + 7 * o, true);
    for (; o < o1; o += kMsdWaves) msd_pair<true>(acc, msd_lds, Wi, (int)(o - o0) + lane, series + 7 * o, o + lag < a.F);
  }

  // the four waves add their sums in wave order through one slab
  for (int w = 0; w < kMsdWaves; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < kMsdTri; ++t) msd_lds[t * 64 + lane] = w == 0 ? acc[t] : msd_lds[t * 64 + lane] + acc[t];
    }
  }
  __syncthreads();
  double* out = a.part + (size_t)blockIdx.x * (kMsdTri * 64);
  for (int i = threadIdx.x; i < kMsdTri * 64; i += kMsdBlock) out[i] = msd_lds[i];
}

// one thread per (lag, triangle entry): the partials of the P workgroups of its lag block in block order
__global__ __launch_bounds__(256) void msd_finish_kernel(const MsdArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_lags * kMsdTri) return;
  const long lag = i / kMsdTri;
  const int t = (int)(i - lag * kMsdTri);
  const long lb = lag >> 6;
  const int lane = (int)(lag & 63);
  double sum = 0.0;
  for (long p = 0; p < a.P; ++p) sum += a.part[(size_t)(p * a.lag_blocks + lb) * (kMsdTri * 64) + t * 64 + lane];
  int r = 0, c = t;      // row r of the upper triangle holds 6 - r entries
  while (c >= 6 - r) { c -= 6 - r; ++r; }
  c += r;
  double* m = a.sums + 36 * lag;
  m[6 * r + c] += sum;
  if (r != c) m[6 * c + r] += sum;
}

}  // namespace rmb
