// rmb_pair_hist.hip -- histogram of pair distances (pair_hist_kernels.h): of the resident raw positions, and of a batch of
// caller-owned frames; the counts behind the radial distribution function (correlation.py).
#include "rmb_internal.h"

#include <cmath>
#include <limits>

#include "pair_hist_kernels.h"

namespace rmbi {
namespace {

typedef rmb::PairHistArgs A;

int check_hist_args(double r_max, long n_bins, const void* hist) {
  if (!hist) return fail(RMB_ERR_ARG, "pair histogram: null histogram pointer");
  if (!(r_max > 0.0) || !std::isfinite(r_max)) return fail(RMB_ERR_ARG, "pair histogram: r_max must be positive and finite");
  if (n_bins < 1 || n_bins > rmb::kPairHistMaxBins) return fail(RMB_ERR_ARG, "pair histogram: n_bins must be 1 ... 8192");
  return 0;
}

template <bool BATCH>
SymKernel hist_kernel(bool periodic) {
  const size_t slabs = sizeof(double4) * 64 * rmb::kSymWaves;
  return periodic ? sym_kernel_of<A, rmb::pair_hist_kernel<true, BATCH>>(slabs) : sym_kernel_of<A, rmb::pair_hist_kernel<false, BATCH>>(slabs);
}

// Launch plan: plan_cull_sweep with two resident rounds of workgroups (every workgroup ends with up to n_bins global
// atomics, so fewer and longer workgroups than the energy sweep's eight rounds).  A workgroup's LDS counters are uint32:
// the plan is refined until a workgroup meets fewer than 2^31 pairs, and refused if it cannot be.
int plan_hist(rmb_ctx* c, const SymKernel& k, size_t dyn_lds, long total_steps, long* blocks, long* chunk_steps) {
  return plan_cull_sweep(c, k, total_steps, blocks, chunk_steps, 2, dyn_lds, 2147483648.0, "pair histogram");
}

void fill_hist(A& a, double r_max, long n_bins, unsigned long long* hist) {
  a.r_max2 = r_max * r_max;
  a.inv_dr = (double)n_bins / r_max;
  a.n_bins = (int)n_bins;
  a.hist = hist;
}

int hist_resident_impl(rmb_ctx* c, double r_max, long n_bins, unsigned long long* hist_dev) {
  if (int rc = check_ready(c)) return rc;
  if (int rc = check_hist_args(r_max, n_bins, hist_dev)) return rc;
  A a{};
  // spatial order, tile bounds and the frame's arguments, always with a fresh Morton permutation: what is left behind is
  // what a potential evaluation that rebuilt its permutation leaves
  const PairOnceErrors msg{"the pair histogram uses raw positions: call rmb_set_positions with wall = 0",
                           "the pair histogram runs over all points: reset the target range", "pair histogram: more than 2^32 points"};
  bool empty;
  if (int rc = pair_once_prepare(c, a, msg, 2, false, &empty)) return rc;
  if (empty) return 0;
  a.Lz = c->L[2]; a.iLz = inv_length(a.Lz);
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  fill_hist(a, r_max, n_bins, hist_dev);
  a.cull2 = c->opt_force_cull ? a.r_max2 : std::numeric_limits<double>::infinity();

  const size_t dyn = (size_t)n_bins * sizeof(unsigned);
  const SymKernel k = hist_kernel<false>(periodic);
  long blocks;
  if (int rc = plan_hist(c, k, dyn, a.step_end, &blocks, &a.chunk_steps)) return rc;
  return sym_launch(c, k, 1, blocks, dyn, a, rmb::PairConsts{}, (void (*)(A)) nullptr, 0);
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

int rmb_pair_histogram_device(rmb_ctx* c, double r_max, long n_bins, unsigned long long* hist_dev) {
  return rmbi::hist_resident_impl(c, r_max, n_bins, hist_dev);
}

int rmb_pair_histogram(rmb_ctx* c, double r_max, long n_bins, unsigned long long* hist_host) {
  if (int rc = rmbi::check_ready(c)) return rc;
  if (int rc = rmbi::check_hist_args(r_max, n_bins, hist_host)) return rc;
  RMB_HIP(hipSetDevice(c->device));
  const size_t bytes = (size_t)n_bins * sizeof(unsigned long long);
  if (int rc = c->out.reserve(bytes)) return rc;
  RMB_HIP(hipMemsetAsync(c->out.p, 0, bytes, c->stream));
  if (int rc = rmbi::hist_resident_impl(c, r_max, n_bins, (unsigned long long*)c->out.p)) return rc;
  RMB_HIP(hipMemcpyAsync(hist_host, c->out.p, bytes, hipMemcpyDeviceToHost, c->stream));
  RMB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int rmb_pair_histogram_frames_device(rmb_ctx* c, const double* frames_dev, long n_frames, long n, const double* L, double r_max, long n_bins,
                                     unsigned long long* hist_dev) {
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (int rc = rmbi::check_hist_args(r_max, n_bins, hist_dev)) return rc;
  if (n_frames < 0 || n < 0) return fail(RMB_ERR_ARG, "pair histogram: negative size");
  if (!L) return fail(RMB_ERR_ARG, "pair histogram: null periodic_length");
  if (n_frames == 0 || n < 2) return 0;
  if (!frames_dev) return fail(RMB_ERR_ARG, "pair histogram: null frames pointer");
  const long tiles = (n + 63) / 64;
  if (tiles > 0x7fffffffL) return fail(RMB_ERR_ARG, "pair histogram: too many points per frame");
  const long upf = tiles * (tiles + 1) / 2;
  if ((double)upf * (double)n_frames * 64.0 > 9.0e18) return fail(RMB_ERR_ARG, "pair histogram: too many pairs for one launch");
  RMB_HIP(hipSetDevice(c->device));
  rmbi::A a{};
  a.n = n; a.n_tiles = (int)tiles;
  a.frames = frames_dev; a.units_per_frame = upf;
  a.step_end = upf * n_frames * 64;
  a.Lx = L[0]; a.Ly = L[1]; a.Lz = L[2];
  a.iLx = rmbi::inv_length(L[0]); a.iLy = rmbi::inv_length(L[1]); a.iLz = rmbi::inv_length(L[2]);
  rmbi::fill_hist(a, r_max, n_bins, hist_dev);
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  const size_t dyn = (size_t)n_bins * sizeof(unsigned);
  const rmbi::SymKernel k = rmbi::hist_kernel<true>(periodic);
  long blocks;
  if (int rc = rmbi::plan_hist(c, k, dyn, a.step_end, &blocks, &a.chunk_steps)) return rc;
  // launched directly: nothing of the context but its device and stream is read, nothing is written (no bookkeeping of the
  // last launch, no timing slot)
  k.launch(&a, rmb::PairConsts{}, (unsigned)blocks, dyn, c->stream);
  RMB_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
