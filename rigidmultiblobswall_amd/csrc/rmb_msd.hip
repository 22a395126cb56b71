// rmb_msd.hip -- 6 x 6 mean-square displacement sums of a batch of caller-owned rigid-body frames (msd_kernels.h): the
// record pass, the lag sweep and its finishing launch; what dynamics analysis (msd.py) is built on.
#include "lag_sweep_host.h"
#include "msd_kernels.h"

namespace rmbi {
namespace {

typedef rmb::MsdArgs A;

int check_msd_args(rmb_ctx* c, const void* frames, long n_frames, long n_bodies, long n_lags, long o_begin, long o_end, long origin_chunk,
                   const void* sums) {
  if (!sums) return fail(RMB_ERR_ARG, "msd: null sums pointer");
  if (int rc = check_frames("msd", frames, n_frames, n_bodies, 7)) return rc;
  if (int rc = check_lag_range("msd", n_frames, n_lags, o_begin, o_end)) return rc;
  if (origin_chunk < 0) return fail(RMB_ERR_ARG, "msd: origin_chunk must not be negative (0 = planned)");
  if (!c) return fail(RMB_ERR_ARG, "null context");      // last: the argument checks need no context, let alone a device
  return 0;
}

int msd_impl(rmb_ctx* c, const double* frames_dev, long n_frames, long n_bodies, const double* offsets_dev, long n_lags, long o_begin, long o_end,
             long origin_chunk, double* sums_dev) {
  if (n_frames == 0 || n_bodies == 0 || o_begin == o_end) return 0;
  A a{};
  a.sums = sums_dev;
  long chunk = origin_chunk > 0 ? origin_chunk : rmb::kMsdPlannedChunk;
  if (chunk > rmb::kMsdMaxChunk) chunk = rmb::kMsdMaxChunk;
  if (int rc = plan_lag_sweep(c, a, "msd", n_frames, n_bodies, 1, n_lags, o_begin, o_end, chunk)) return rc;
  const long blocks = a.P * a.lag_blocks;
  const size_t rec_pad = pad256((size_t)n_frames * n_bodies * 7 * sizeof(double));
  const size_t part_bytes = (size_t)blocks * rmb::kMsdTri * 64 * sizeof(double);
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->msd_ws.reserve(rec_pad + part_bytes)) return rc;
  a.rec = (const double*)c->msd_ws.p;
  a.part = (double*)((char*)c->msd_ws.p + rec_pad);
  const rmb::MsdRecordArgs r{frames_dev, offsets_dev, (double*)c->msd_ws.p, n_frames, n_bodies};
  const long pairs = n_frames * n_bodies;
  if ((pairs + 255) / 256 > 0x7fffffffL) return fail(RMB_ERR_ARG, "msd: too many frames for one launch");
  hipLaunchKernelGGL(rmb::msd_record_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, c->stream, r);
  RMB_HIP(hipGetLastError());
  hipLaunchKernelGGL(rmb::msd_sweep_kernel, dim3((unsigned)blocks), dim3(rmb::kLagBlock), rmb::lag_sweep_lds(a.chunk, rmb::MsdOp::R, rmb::MsdOp::NS),
                     c->stream, a);
  RMB_HIP(hipGetLastError());
  hipLaunchKernelGGL(rmb::msd_finish_kernel, dim3((unsigned)((n_lags * rmb::kMsdTri + 255) / 256)), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

int rmb_msd_frames_device(rmb_ctx* c, const double* frames_dev, long n_frames, long n_bodies, const double* offsets_dev, long n_lags, long o_begin,
                          long o_end, long origin_chunk, double* sums_dev) {
  if (int rc = rmbi::check_msd_args(c, frames_dev, n_frames, n_bodies, n_lags, o_begin, o_end, origin_chunk, sums_dev)) return rc;
  // nothing of the context but its device, its stream and the workspace of this entry is read or written
  return rmbi::msd_impl(c, frames_dev, n_frames, n_bodies, offsets_dev, n_lags, o_begin, o_end, origin_chunk, sums_dev);
}

int rmb_msd_frames(rmb_ctx* c, const double* frames_host, long n_frames, long n_bodies, const double* offsets_host, long n_lags, long o_begin,
                   long o_end, long origin_chunk, double* sums_host) {
  if (int rc = rmbi::check_msd_args(c, frames_host, n_frames, n_bodies, n_lags, o_begin, o_end, origin_chunk, sums_host)) return rc;
  RMB_HIP(hipSetDevice(c->device));
  const size_t fb = (size_t)n_frames * n_bodies * 7 * sizeof(double), ob = offsets_host ? (size_t)n_bodies * 3 * sizeof(double) : 0;
  const size_t sb = (size_t)n_lags * 36 * sizeof(double);
  if (int rc = c->r_stage.reserve(fb)) return rc;
  if (int rc = c->vec.reserve(ob)) return rc;
  if (int rc = c->out.reserve(sb)) return rc;
  if (fb) RMB_HIP(hipMemcpyAsync(c->r_stage.p, frames_host, fb, hipMemcpyHostToDevice, c->stream));
  if (ob) RMB_HIP(hipMemcpyAsync(c->vec.p, offsets_host, ob, hipMemcpyHostToDevice, c->stream));
  RMB_HIP(hipMemsetAsync(c->out.p, 0, sb, c->stream));
  if (int rc = rmbi::msd_impl(c, (const double*)c->r_stage.p, n_frames, n_bodies, ob ? (const double*)c->vec.p : nullptr, n_lags, o_begin, o_end,
                              origin_chunk, (double*)c->out.p))
    return rc;
  RMB_HIP(hipMemcpyAsync(sums_host, c->out.p, sb, hipMemcpyDeviceToHost, c->stream));
  RMB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
