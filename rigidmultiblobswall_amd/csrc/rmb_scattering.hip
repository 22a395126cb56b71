// rmb_scattering.hip -- density modes rho_k(f) of caller-owned frames and the lag sums behind the structure factor S(k),
// the intermediate scattering function F(k, t) and its self part F_s(k, t) (scattering_kernels.h): the modes sweep (a lane
// owns a wavevector), the lag sweep (a lane owns a lag) over the modes or over per-point phase records, and their finishing
// launches; what scattering.py is built on.
#include "lag_sweep_host.h"
#include "scattering_kernels.h"

namespace rmbi {
namespace {

constexpr long kScatMaxK = 16384, kScatMaxN = 32768;

int check_wavevectors(const char* who, const double* L, const int* kint, long K) {
  const std::string w(who);
  if (K < 0) return fail(RMB_ERR_ARG, w + ": negative size");
  if (K > kScatMaxK) return fail(RMB_ERR_ARG, w + ": at most 16384 wavevectors per call");
  if (!L) return fail(RMB_ERR_ARG, w + ": null L pointer");
  if (K > 0 && !kint) return fail(RMB_ERR_ARG, w + ": null wavevector pointer");
  for (long i = 0; i < 3 * K; ++i) {
    const long n = kint[i];
    if (n > kScatMaxN || n < -kScatMaxN) return fail(RMB_ERR_ARG, w + ": |n_d| must be at most 32768");
    if (n != 0 && !(L[i % 3] > 0.0)) return fail(RMB_ERR_ARG, w + ": n_d != 0 needs a positive length L_d");
  }
  return 0;
}

// c_d = n_d / L_d of the wavevectors [k0, k0 + count) into coef_dev, the integers by value in the launch
int upload_coefficients(rmb_ctx* c, const double* L, const int* kint, long K, double* coef_dev) {
  for (long k0 = 0; k0 < K; k0 += rmb::kScatCoefBatch) {
    rmb::ScatCoefArgs a{};
    a.count = K - k0 < rmb::kScatCoefBatch ? K - k0 : rmb::kScatCoefBatch;
    for (long i = 0; i < 3 * a.count; ++i) a.n[i] = kint[3 * k0 + i];
    for (int d = 0; d < 3; ++d) a.L[d] = L[d];
    a.coef = coef_dev + 3 * k0;
    hipLaunchKernelGGL(rmb::scat_coef_kernel, dim3(1), dim3(rmb::kScatCoefBatch), 0, c->stream, a);
    RMB_HIP(hipGetLastError());
  }
  return 0;
}

// Launch plan of the modes sweep: one workgroup per (frame, block of 64 wavevectors); where that is less than about eight
// workgroups per CU (few frames of many points) the points of a frame are cut into P ranges of at least 256.
int modes_impl(rmb_ctx* c, const double* frames_dev, long n_frames, long n, const double* L, const int* kint, long K, double* modes_dev) {
  if (n_frames == 0 || K == 0) return 0;
  rmb::ScatModesArgs a{};
  a.frames = frames_dev; a.modes = modes_dev;
  a.F = n_frames; a.N = n; a.K = K; a.KB = (K + 63) / 64;
  if ((double)n_frames * (double)a.KB > 2.0e9) return fail(RMB_ERR_ARG, "density modes: too many frames for one launch");
  const long base = n_frames * a.KB, target = 8 * c->n_cu;
  a.P = base < target ? (target + base - 1) / base : 1;
  const long max_p = n / 256 > 1 ? n / 256 : 1;
  if (a.P > max_p) a.P = max_p;
  const long blocks = base * a.P;
  if (blocks > 0x7fffffffL) return fail(RMB_ERR_ARG, "density modes: too many frames for one launch");
  const size_t coef_bytes = pad256((size_t)K * 3 * sizeof(double));
  const size_t part_bytes = a.P > 1 ? (size_t)blocks * 128 * sizeof(double) : 0;
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->scat_ws.reserve(coef_bytes + part_bytes)) return rc;
  a.coef = (const double*)c->scat_ws.p;
  a.part = (double*)((char*)c->scat_ws.p + coef_bytes);
  if (int rc = upload_coefficients(c, L, kint, K, (double*)c->scat_ws.p)) return rc;
  hipLaunchKernelGGL(rmb::scat_modes_kernel, dim3((unsigned)blocks), dim3(rmb::kScatBlock), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  if (a.P > 1) {
    hipLaunchKernelGGL(rmb::scat_modes_finish_kernel, dim3((unsigned)((n_frames * K + 255) / 256)), dim3(256), 0, c->stream, a);
    RMB_HIP(hipGetLastError());
  }
  return 0;
}

template <int NC>
int launch_sweep(rmb_ctx* c, const rmb::ScatSweepArgs& a, long rows) {
  hipLaunchKernelGGL(rmb::scat_sweep_kernel<NC>, dim3((unsigned)(a.P * a.lag_blocks), (unsigned)rows), dim3(rmb::kLagBlock),
                     rmb::lag_sweep_lds(a.chunk, rmb::ScatOp<NC>::R, rmb::ScatOp<NC>::NS), c->stream, a);
  RMB_HIP(hipGetLastError());
  hipLaunchKernelGGL(rmb::scat_sweep_finish_kernel<NC>, dim3((unsigned)((a.n_lags * a.k_count + 255) / 256)), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}

int lags_impl(rmb_ctx* c, const double* modes_dev, long n_frames, long K, long n_lags, long o_begin, long o_end, double* sums_dev) {
  if (n_frames == 0 || K == 0 || o_begin == o_end) return 0;
  rmb::ScatSweepArgs a{};
  if (int rc = plan_lag_sweep(c, a, "scattering", n_frames, 1, K, n_lags, o_begin, o_end, rmb::kScatChunk)) return rc;
  a.sums = sums_dev; a.K = K; a.k0 = 0; a.k_count = K;
  const size_t rec_bytes = pad256((size_t)n_frames * K * 2 * sizeof(double));
  const size_t part_bytes = (size_t)K * a.P * a.lag_blocks * 64 * sizeof(double);
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->scat_ws.reserve(rec_bytes + part_bytes)) return rc;
  a.rec = (const double*)c->scat_ws.p;
  a.part = (double*)((char*)c->scat_ws.p + rec_bytes);
  rmb::ScatRecordArgs r{};
  r.src = modes_dev; r.rec = (double*)c->scat_ws.p; r.F = n_frames; r.N = K;
  const long pairs = n_frames * K;
  if ((pairs + 255) / 256 > 0x7fffffffL) return fail(RMB_ERR_ARG, "scattering lags: too many frames for one launch");
  hipLaunchKernelGGL(rmb::scat_transpose_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, c->stream, r);
  RMB_HIP(hipGetLastError());
  return launch_sweep<1>(c, a, K);
}

int self_impl(rmb_ctx* c, const double* frames_dev, long n_frames, long n, const double* L, const int* kint, long K, long n_lags, long o_begin,
              long o_end, double* sums_dev) {
  if (n_frames == 0 || K == 0 || n == 0 || o_begin == o_end) return 0;
  rmb::ScatSweepArgs a{};
  if (int rc = plan_lag_sweep(c, a, "scattering", n_frames, n, 1, n_lags, o_begin, o_end, rmb::kScatChunk)) return rc;
  a.sums = sums_dev; a.K = K;
  const long pairs = n_frames * n;
  if ((pairs + 255) / 256 > 0x7fffffffL) return fail(RMB_ERR_ARG, "self scattering: too many frames for one launch");
  const size_t rec_bytes = pad256((size_t)pairs * 2 * rmb::kScatGroup * sizeof(double));
  const size_t part_bytes = (size_t)a.P * a.lag_blocks * rmb::kScatGroup * 64 * sizeof(double);
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->scat_ws.reserve(rec_bytes + part_bytes)) return rc;
  a.rec = (const double*)c->scat_ws.p;
  a.part = (double*)((char*)c->scat_ws.p + rec_bytes);
  // one pass per group of three wavevectors; the passes follow each other on the stream and share the workspace
  for (long k0 = 0; k0 < K; k0 += rmb::kScatGroup) {
    const int nc = (int)(K - k0 < rmb::kScatGroup ? K - k0 : rmb::kScatGroup);
    rmb::ScatRecordArgs r{};
    r.src = frames_dev; r.rec = (double*)c->scat_ws.p; r.F = n_frames; r.N = n;
    for (int i = 0; i < 3 * nc; ++i) {
      const int nd = kint[3 * k0 + i];
      r.c[i] = nd != 0 ? (double)nd / L[i % 3] : 0.0;
    }
    a.k0 = k0; a.k_count = nc;
    const dim3 grid((unsigned)((pairs + 255) / 256));
    int rc = 0;
    if (nc == 3) {
      hipLaunchKernelGGL(rmb::scat_record_kernel<3>, grid, dim3(256), 0, c->stream, r);
      RMB_HIP(hipGetLastError());
      rc = launch_sweep<3>(c, a, 1);
    } else if (nc == 2) {
      hipLaunchKernelGGL(rmb::scat_record_kernel<2>, grid, dim3(256), 0, c->stream, r);
      RMB_HIP(hipGetLastError());
      rc = launch_sweep<2>(c, a, 1);
    } else {
      hipLaunchKernelGGL(rmb::scat_record_kernel<1>, grid, dim3(256), 0, c->stream, r);
      RMB_HIP(hipGetLastError());
      rc = launch_sweep<1>(c, a, 1);
    }
    if (rc) return rc;
  }
  return 0;
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

// nothing of the context but its device, its stream and the workspace of these entries is read or written

int rmb_density_modes_frames_device(rmb_ctx* c, const double* frames_dev, long n_frames, long n, const double* L, const int* kint, long K,
                                    double* modes_dev) {
  if (int rc = rmbi::check_frames("density modes", frames_dev, n_frames, n, 3)) return rc;
  if (int rc = rmbi::check_wavevectors("density modes", L, kint, K)) return rc;
  if (n_frames > 0 && K > 0 && !modes_dev) return fail(RMB_ERR_ARG, "density modes: null modes pointer");
  if (!c) return fail(RMB_ERR_ARG, "null context");      // last: the argument checks need no context, let alone a device
  return rmbi::modes_impl(c, frames_dev, n_frames, n, L, kint, K, modes_dev);
}

int rmb_scattering_lags_device(rmb_ctx* c, const double* modes_dev, long n_frames, long K, long n_lags, long o_begin, long o_end,
                               double* sums_dev) {
  if (int rc = rmbi::check_frames("scattering lags", modes_dev, n_frames, K, 2, "modes")) return rc;
  if (K > rmbi::kScatMaxK) return fail(RMB_ERR_ARG, "scattering lags: at most 16384 wavevectors per call");
  if (int rc = rmbi::check_lag_range("scattering lags", n_frames, n_lags, o_begin, o_end)) return rc;
  if (K > 0 && !sums_dev) return fail(RMB_ERR_ARG, "scattering lags: null sums pointer");
  if (!c) return fail(RMB_ERR_ARG, "null context");
  return rmbi::lags_impl(c, modes_dev, n_frames, K, n_lags, o_begin, o_end, sums_dev);
}

int rmb_self_scattering_frames_device(rmb_ctx* c, const double* frames_dev, long n_frames, long n, const double* L, const int* kint, long K,
                                      long n_lags, long o_begin, long o_end, double* sums_dev) {
  if (int rc = rmbi::check_frames("self scattering", frames_dev, n_frames, n, 2 * rmb::kScatGroup)) return rc;      // the records' width
  if (int rc = rmbi::check_wavevectors("self scattering", L, kint, K)) return rc;
  if (int rc = rmbi::check_lag_range("self scattering", n_frames, n_lags, o_begin, o_end)) return rc;
  if (K > 0 && !sums_dev) return fail(RMB_ERR_ARG, "self scattering: null sums pointer");
  if (!c) return fail(RMB_ERR_ARG, "null context");
  return rmbi::self_impl(c, frames_dev, n_frames, n, L, kint, K, n_lags, o_begin, o_end, sums_dev);
}

}  // extern "C"
