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
//   msd_sweep_kernel    a LANE OWNS A LAG: the frame of lag_sweep_kernels.h (schedule, staging, order of additions) with
//                       MsdOp -- records of 7 doubles, one row, the 21 sums of the upper triangle in registers per lane.
//   msd_finish_kernel   adds the partials of a lag in block order INTO the caller's (n_lags, 6, 6) tensor, both triangles.
//
// A lane adds nothing where o + l >= F: frames past the end are staged as zeros, a zero quaternion gives u = 0 and the
// translational part is masked (MASK_TAIL: only in the loop over the last origins, where that can happen).
// The sums of a launch plan are the same bits on every call.
#pragma once
#include "lag_sweep_kernels.h"

namespace rmb {

constexpr int kMsdTri = 21;                 // upper triangle of the 6 x 6 sums
constexpr long kMsdMaxChunk = 1024;         // origins per staged window: (1024 + 63) records of 56 bytes < 64 KB of LDS
constexpr long kMsdPlannedChunk = 256;

struct MsdRecordArgs {
  const double* frames;    // (F, N, 7)
  const double* offsets;   // (N, 3) body-frame tracking offsets, or nullptr
  double* rec;             // (N, F, 7): tracked point, quaternion
  long F, N;
};

struct MsdArgs : LagSweepArgs {      // B = N bodies, one row
  double* sums;            // (n_lags, 6, 6), added to
};

__global__ __launch_bounds__(256) void msd_record_kernel(const MsdRecordArgs a) {
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

// The policy of the frame.  pair: one (origin, lag) pair of a lane, the lagged record from the staged window win[7][W] at
// column j, the origin record `org` wave-uniform (scalar loads), the 21 products added to the lane's sums.  MASKED: `ok` is
// false where the lagged frame is past the end -- it was staged as zeros, a zero quaternion makes u = 0 by itself, the
// translational part is zeroed here.
struct MsdOp {
  typedef MsdArgs Args;
  static constexpr int R = 7, NS = kMsdTri;
  static constexpr bool MASK_TAIL = true;
  template <bool MASKED>
  static __device__ __forceinline__ void pair(double (&acc)[kMsdTri], const double* win, int W, int j, const double* org, bool ok) {
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
};

__global__ __launch_bounds__(kLagBlock) void msd_sweep_kernel(const MsdArgs a) {
  extern __shared__ double msd_lds[];      // the frame's window win[7][W], later its combine slab [21][64]
  lag_sweep<MsdOp>(a, msd_lds);
}

// one thread per (lag, triangle entry): the partials of the P workgroups of its lag block in block order
__global__ __launch_bounds__(256) void msd_finish_kernel(const MsdArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_lags * kMsdTri) return;
  const long lag = i / kMsdTri;
  const int t = (int)(i - lag * kMsdTri);
  const double sum = lag_sweep_partial_sum<kMsdTri>(a, 0, lag >> 6, t, (int)(lag & 63));
  int r = 0, c = t;      // row r of the upper triangle holds 6 - r entries
  while (c >= 6 - r) { c -= 6 - r; ++r; }
  c += r;
  double* m = a.sums + 36 * lag;
  m[6 * r + c] += sum;
  if (r != c) m[6 * c + r] += sum;
}

}  // namespace rmb
