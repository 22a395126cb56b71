// rmb_msd.hip -- 6 x 6 mean-square displacement sums of a batch of caller-owned rigid-body frames (msd_kernels.h): the
// record pass, the lag sweep and its finishing launch; what dynamics analysis (msd.py) is built on.
#include "rmb_internal.h"

#include "msd_kernels.h"

namespace rmbi {
namespace {

typedef rmb::MsdArgs A;

int check_msd_args(rmb_ctx* c, const void* frames, long n_frames, long n_bodies, long n_lags, long o_begin, long o_end, long origin_chunk,
                   const void* sums) {
  if (!sums) return fail(RMB_ERR_ARG, "msd: null sums pointer");
  if (n_frames < 0 || n_bodies < 0) return fail(RMB_ERR_ARG, "msd: negative size");
  if (n_lags < 1) return fail(RMB_ERR_ARG, "msd: n_lags must be at least 1");
  if (n_lags > (1L << 24)) return fail(RMB_ERR_ARG, "msd: n_lags must be at most 2^24");
  if (o_begin < 0 || o_end < o_begin || o_end > n_frames) return fail(RMB_ERR_ARG, "msd: origins must satisfy 0 <= o_begin <= o_end <= n_frames");
  if (origin_chunk < 0) return fail(RMB_ERR_ARG, "msd: origin_chunk must not be negative (0 = planned)");
  if ((double)n_frames * (double)n_bodies * 7.0 > 1.0e18) return fail(RMB_ERR_ARG, "msd: too many frames for one call");
  if (n_frames > 0 && n_bodies > 0 && !frames) return fail(RMB_ERR_ARG, "msd: null frames pointer");
  if (!c) return fail(RMB_ERR_ARG, "null context");      // last: the argument checks need no context, let alone a device
  return 0;
}

// Launch plan: about eight workgroups per CU over all lag blocks (the sweep is VALU-bound with 4 waves per workgroup; more
// workgroups only add partials), never more than there are work items.
int msd_impl(rmb_ctx* c, const double* frames_dev, long n_frames, long n_bodies, const double* offsets_dev, long n_lags, long o_begin, long o_end,
             long origin_chunk, double* sums_dev) {
  if (n_frames == 0 || n_bodies == 0 || o_begin == o_end) return 0;
  A a{};
  a.frames = frames_dev; a.offsets = offsets_dev; a.sums = sums_dev;
  a.F = n_frames; a.N = n_bodies;
  a.n_lags = n_lags; a.lag_blocks = (n_lags + 63) / 64;
  a.o_begin = o_begin; a.o_end = o_end;
  const long n_origins = o_end - o_begin;
  a.chunk = origin_chunk > 0 ? origin_chunk : rmb::kMsdPlannedChunk;
  if (a.chunk > rmb::kMsdMaxChunk) a.chunk = rmb::kMsdMaxChunk;
  if (a.chunk > n_origins) a.chunk = n_origins;
  a.n_chunks = (n_origins + a.chunk - 1) / a.chunk;
  if ((double)a.n_chunks * (double)n_bodies > 4.0e18) return fail(RMB_ERR_ARG, "msd: too many work items for one call");
  a.items = a.n_chunks * n_bodies;
  const long target = 8 * c->n_cu;
  a.P = (target + a.lag_blocks - 1) / a.lag_blocks;
  if (a.P > a.items) a.P = a.items;
  if ((double)a.items * (double)(a.P + 1) > 9.0e18) return fail(RMB_ERR_ARG, "msd: too many work items for one call");      // items * p in the kernel
  const long blocks = a.P * a.lag_blocks;
  if (blocks > 0x7fffffffL) return fail(RMB_ERR_ARG, "msd: too many lag blocks for one launch");
  const size_t rec_bytes = (size_t)n_frames * n_bodies * 7 * sizeof(double);
  const size_t rec_pad = (rec_bytes + 255) & ~(size_t)255;
  const size_t part_bytes = (size_t)blocks * rmb::kMsdTri * 64 * sizeof(double);
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->msd_ws.reserve(rec_pad + part_bytes)) return rc;
  a.rec = (double*)c->msd_ws.p;
  a.part = (double*)((char*)c->msd_ws.p + rec_pad);
  const long pairs = n_frames * n_bodies;
  if ((pairs + 255) / 256 > 0x7fffffffL) return fail(RMB_ERR_ARG, "msd: too many frames for one launch");
  hipLaunchKernelGGL(rmb::msd_record_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  hipLaunchKernelGGL(rmb::msd_sweep_kernel, dim3((unsigned)blocks), dim3(rmb::kMsdBlock), rmb::msd_sweep_lds(a.chunk), c->stream, a);
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
