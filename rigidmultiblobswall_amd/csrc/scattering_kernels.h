// scattering_kernels.h -- density modes, structure factor and intermediate scattering functions of point trajectories by
// direct Fourier sums (gfx950, fp64).  No grid: the sums are exact in the positions.
//
// Frames (F, N, 3), wavevectors k = 2 pi (n_x / L_x, n_y / L_y, n_z / L_z) with integer n.  With c_d = n_d / L_d (one
// correctly rounded division per axis, 0 where n_d = 0), a point's phase in TURNS is
//
//   t_j = fma(z_j, c_z, fma(y_j, c_y, x_j c_x)),   r_j = t_j - rint(t_j)  (exact),   theta_j = 2 pi r_j,
//
// and (cos theta_j, sin theta_j) = sincospi(2 r_j): the reduction happens in turns, before any multiplication by pi, so a
// cloud at 1000 L keeps its accuracy.  Everything below uses this one route (scat_phase).
//
//   rho_k(f)  = sum_j exp(-i theta_j)                      stored (sum cos, -sum sin)                 scat_modes_kernel
//   C[l, k]   = sum_o Re( rho_k(o + l) conj rho_k(o) )                                                  scat_sweep_kernel<1>
//   Sf[l, k]  = sum_o sum_j Re( z_jk(o + l) conj z_jk(o) ),  z = exp(-i theta)                          scat_sweep_kernel<NC>
//
//   scat_coef_kernel    c_d of up to 256 wavevectors per launch, the integers by value in the kernel arguments (no host
//                       memory is read asynchronously).
//   scat_modes_kernel   a LANE OWNS A WAVEVECTOR: c_x c_y c_z in registers.  A workgroup serves (frame, block of 64
//                       wavevectors, point range); tiles of the frame's points are staged in LDS and read wave-uniform
//                       (one broadcast read serves 64 wavevectors); each of the four waves takes every fourth point.  No
//                       cross-lane reduction; the four waves add their sums in wave order through LDS.  One point range:
//                       the modes are written directly.  A split frame (few frames of many points) writes partials and
//                       scat_modes_finish_kernel adds them in range order.
//   scat_transpose_kernel / scat_record_kernel   the records of the lag sweep, series-major and time-contiguous: the modes
//                       of a wavevector (F, K, 2) -> (K, F, 2), or the phases z_jk(f) of a group of NC <= 3 wavevectors
//                       (N, F, 2 NC), computed once per (frame, point), not once per pair.
//   scat_sweep_kernel   a LANE OWNS A LAG: the frame of lag_sweep_kernels.h (schedule, staging, order of additions) with
//                       ScatOp<NC> -- records of 2 NC doubles, NC sums per lane in registers, one row per wavevector
//                       (collective) or one row of N points (self).  Frames past the end are staged as zeros and add
//                       exactly nothing -- no mask.
//   scat_sweep_finish_kernel  adds the partials of a (lag, wavevector) in block order INTO the caller's (n_lags, K).
//
// No floating-point atomic anywhere: the same call gives the same bits.
#pragma once
#include "lag_sweep_kernels.h"
#include "scat_phase.h"      // scat_phase: (cos theta, sin theta) of a point

namespace rmb {

constexpr int kScatWaves = 4;
constexpr int kScatBlock = 64 * kScatWaves;
constexpr int kScatTile = 512;              // points per staged tile of the modes sweep: 12 KB of LDS
constexpr int kScatCoefBatch = 256;         // wavevectors per scat_coef_kernel launch: 3 KB of kernel arguments
constexpr int kScatGroup = 3;               // wavevectors per pass of the self sweep: records of six doubles
constexpr long kScatChunk = 256;            // origins per staged window: (256 + 63) records of 16 NC bytes

struct ScatCoefArgs {
  int n[3 * kScatCoefBatch];
  double L[3];
  long count;
  double* coef;            // (count, 3): n_d / L_d
};

struct ScatModesArgs {
  const double* frames;    // (F, N, 3)
  const double* coef;      // (K, 3)
  long F, N, K, KB;        // KB blocks of 64 wavevectors
  long P;                  // point ranges per frame
  double* part;            // [F][P][KB][2][64], P > 1 only
  double* modes;           // (F, K, 2), overwritten
};

struct ScatRecordArgs {
  const double* src;       // frames (F, N, 3), or the modes (F, K, 2)
  double* rec;
  long F, N;               // N: points, or wavevectors
  double c[3 * kScatGroup];  // c_d of the group's wavevectors (record kernel)
};

struct ScatSweepArgs : LagSweepArgs {      // B: points; 1 for the collective sums
  double* sums;            // (n_lags, K), added to
  long K, k0, k_count;     // row y, component c is wavevector k0 + y NC + c; k_count of them in all
};

__global__ __launch_bounds__(kScatCoefBatch) void scat_coef_kernel(const ScatCoefArgs a) {
  const long i = threadIdx.x;
  if (i >= a.count) return;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int n = a.n[3 * i + d];
    a.coef[3 * i + d] = n != 0 ? (double)n / a.L[d] : 0.0;
  }
}

__global__ __launch_bounds__(kScatBlock) void scat_modes_kernel(const ScatModesArgs a) {
  __shared__ double pts[3 * kScatTile];      // later the combine slab [2][64]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long kb = blockIdx.x % a.KB, rest = blockIdx.x / a.KB;
  const long p = rest % a.P, f = rest / a.P;
  const long k = 64 * kb + lane;
  const long kk = k < a.K ? k : a.K - 1;      // lanes past the last wavevector compute sums nobody reads
  const double cx = a.coef[3 * kk], cy = a.coef[3 * kk + 1], cz = a.coef[3 * kk + 2];
  const long j0 = a.N * p / a.P, j1 = a.N * (p + 1) / a.P;
  const double* frame = a.frames + 3 * f * a.N;
  double sr = 0.0, si = 0.0;
  for (long t0 = j0; t0 < j1; t0 += kScatTile) {
    const int m = (int)(j1 - t0 < kScatTile ? j1 - t0 : kScatTile);
    __syncthreads();      // the previous tile's readers are done
    for (int i = threadIdx.x; i < 3 * m; i += kScatBlock) pts[i] = frame[3 * t0 + i];
    __syncthreads();
    for (int j = wave; j < m; j += kScatWaves) {
      double s, c;
      scat_phase(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2], cx, cy, cz, &s, &c);
      sr += c;
      si -= s;
    }
  }
  // the four waves add their sums in wave order through one slab
  for (int w = 0; w < kScatWaves; ++w) {
    __syncthreads();
    if (wave == w) {
      pts[lane] = w == 0 ? sr : pts[lane] + sr;
      pts[64 + lane] = w == 0 ? si : pts[64 + lane] + si;
    }
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  if (a.P > 1) {
    double* out = a.part + (size_t)blockIdx.x * 128;      // blockIdx.x = (f P + p) KB + kb
    out[lane] = pts[lane];
    out[64 + lane] = pts[64 + lane];
  } else if (k < a.K) {
    double* out = a.modes + 2 * (f * a.K + k);
    out[0] = pts[lane];
    out[1] = pts[64 + lane];
  }
}

// one thread per (frame, wavevector): the partials of the P point ranges in range order
__global__ __launch_bounds__(256) void scat_modes_finish_kernel(const ScatModesArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.F * a.K) return;
  const long f = i / a.K, k = i - f * a.K;
  const long kb = k >> 6;
  const int lane = (int)(k & 63);
  double sr = 0.0, si = 0.0;
  for (long p = 0; p < a.P; ++p) {
    const double* in = a.part + (size_t)((f * a.P + p) * a.KB + kb) * 128;
    sr += in[lane];
    si += in[64 + lane];
  }
  a.modes[2 * i] = sr;
  a.modes[2 * i + 1] = si;
}

// modes (F, K, 2) -> rec (K, F, 2)
__global__ __launch_bounds__(256) void scat_transpose_kernel(const ScatRecordArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // (frame, wavevector), the caller's order: coalesced reads
  if (i >= a.F * a.N) return;
  const long f = i / a.N, k = i - f * a.N;
  double* out = a.rec + 2 * (k * a.F + f);
  out[0] = a.src[2 * i];
  out[1] = a.src[2 * i + 1];
}

// frames (F, N, 3) -> rec (N, F, 2 NC): z = (cos theta, -sin theta) of the group's NC wavevectors
template <int NC>
__global__ __launch_bounds__(256) void scat_record_kernel(const ScatRecordArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // (frame, point)
  if (i >= a.F * a.N) return;
  const long f = i / a.N, j = i - f * a.N;
  const double x = a.src[3 * i], y = a.src[3 * i + 1], z = a.src[3 * i + 2];
  double* out = a.rec + 2 * NC * (j * a.F + f);
#pragma unroll
  for (int g = 0; g < NC; ++g) {
    double s, c;
    scat_phase(x, y, z, a.c[3 * g], a.c[3 * g + 1], a.c[3 * g + 2], &s, &c);
    out[2 * g] = c;
    out[2 * g + 1] = -s;
  }
}

// The policy of the frame: records of the phases (or modes) of NC wavevectors, one sum each.
template <int NC>
struct ScatOp {
  typedef ScatSweepArgs Args;
  static constexpr int R = 2 * NC, NS = NC;
  static constexpr bool MASK_TAIL = false;      // a zero record adds exactly nothing
  template <bool MASKED>
  static __device__ __forceinline__ void pair(double (&acc)[NC], const double* win, int W, int j, const double* org, bool) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      // Re(b conj a): one rounded product, one fused step, one addition to the sum
      const double t = __builtin_fma(win[2 * c * W + j], org[2 * c], win[(2 * c + 1) * W + j] * org[2 * c + 1]);
      acc[c] += t;
    }
  }
};

template <int NC>
__global__ __launch_bounds__(kLagBlock) void scat_sweep_kernel(const ScatSweepArgs a) {
  extern __shared__ double scat_lds[];      // the frame's window win[2 NC][W], later its combine slab [NC][64]
  lag_sweep<ScatOp<NC>>(a, scat_lds);
}

// one thread per (lag, wavevector of this launch): the partials of the P workgroups of its lag block in block order
template <int NC>
__global__ __launch_bounds__(256) void scat_sweep_finish_kernel(const ScatSweepArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_lags * a.k_count) return;
  const long lag = i / a.k_count, kc = i - lag * a.k_count;
  const long y = kc / NC;
  a.sums[lag * a.K + a.k0 + kc] += lag_sweep_partial_sum<NC>(a, y, lag >> 6, (int)(kc - y * NC), (int)(lag & 63));
}

}  // namespace rmb
