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
const void* hist_kernel(bool periodic) {
  return periodic ? (const void*)rmb::pair_hist_kernel<true, BATCH> : (const void*)rmb::pair_hist_kernel<false, BATCH>;
}

// Launch plan: two resident rounds of workgroups (every workgroup ends with up to n_bins global atomics, so fewer and
// longer workgroups than the energy sweep's eight rounds), at least 256 steps each, a wave's steps cut into strided
// chunks as in plan_cull_sweep.  A workgroup's LDS counters are uint32: the plan is refined until a workgroup meets
// fewer than 2^31 pairs (64 per step), and refused if it cannot be.
int plan_hist(rmb_ctx* c, const void* fn, size_t dyn_lds, long total_steps, long* blocks, long* chunk_steps) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64 * rmb::kSymWaves, dyn_lds) != hipSuccess || occ < 1) occ = 1;
  if (occ > 8) occ = 8;
  long b = c->n_cu * occ * 2;
  const long need = (total_steps + 255) / 256;
  if (b > need) b = need;
  if (b < 1) b = 1;
  for (;;) {
    const long waves = b * rmb::kSymWaves;
    const long spw = (total_steps + waves - 1) / waves;
    const long ch = chunked_steps(c, total_steps, waves, spw, c->opt_sym_chunk_steps / 4);
    const long step = ch < spw ? ch : spw;
    const long n_chunks = (total_steps + step - 1) / step;
    const long per_wave = (n_chunks + waves - 1) / waves * step;      // steps of the busiest wave
    if ((double)per_wave * rmb::kSymWaves * 64.0 < 2147483648.0) {
      *blocks = b;
      *chunk_steps = ch < spw ? ch : 0;
      return 0;
    }
    if (b > (1L << 30)) return fail(RMB_ERR_ARG, "pair histogram: too many pairs for one launch");
    b *= 2;
  }
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
  if (c->wall) return fail(RMB_ERR_STATE, "the pair histogram uses raw positions: call rmb_set_positions with wall = 0");
  if (c->tgt_begin != 0 || c->tgt_end != c->n) return fail(RMB_ERR_STATE, "the pair histogram runs over all points: reset the target range");
  const long n = c->n, tiles = (n + 63) / 64;
  if (n < 2) return 0;
  if (n > 0xffffffffL) return fail(RMB_ERR_ARG, "pair histogram: more than 2^32 points");
  RMB_HIP(hipSetDevice(c->device));

  A a{};
  fill_sym_args(a, SymConf{(const double4*)c->pos.p, n, {c->L[0], c->L[1], c->L[2]}, 0, nullptr}, c, 0.0, tiles * (tiles + 1) / 2, 0, 1);
  a.Lz = c->L[2]; a.iLz = inv_length(a.Lz);
  a.order = 0; a.xcd = 0;      // as the energy sweep: after culling the surviving units hug the diagonal
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  fill_hist(a, r_max, n_bins, hist_dev);

  // Spatial order and tile bounds as the energy sweep's (rmb_potential.hip), always with a fresh Morton permutation: what
  // is left behind is what a potential evaluation that rebuilt its permutation leaves.
  const bool sorted = c->opt_force_sort && tiles >= 32;
  if (int rc = build_tile_bounds(c, sorted, false)) return rc;
  if (sorted) c->pot_sort_age = 0;
  c->tile_bounds_valid = true;
  c->force_sorted = sorted;
  a.pos = sorted ? (const double4*)c->fpos.p : (const double4*)c->pos.p;
  a.bounds = (const double*)c->tile_bounds.p;
  a.cull2 = c->opt_force_cull ? a.r_max2 : std::numeric_limits<double>::infinity();

  const size_t dyn = (size_t)n_bins * sizeof(unsigned);
  SymKernel k = periodic ? sym_kernel_of<A, rmb::pair_hist_kernel<true, false>>(sizeof(double4) * 64 * rmb::kSymWaves)
                         : sym_kernel_of<A, rmb::pair_hist_kernel<false, false>>(sizeof(double4) * 64 * rmb::kSymWaves);
  long blocks;
  if (int rc = plan_hist(c, k.fn, dyn, a.step_end, &blocks, &a.chunk_steps)) return rc;
  if (blocks > 0x7fffffffL) return fail(RMB_ERR_ARG, "pair histogram: too many pairs for one launch");
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
  long blocks;
  if (int rc = rmbi::plan_hist(c, rmbi::hist_kernel<true>(periodic), dyn, a.step_end, &blocks, &a.chunk_steps)) return rc;
  if (blocks > 0x7fffffffL) return fail(RMB_ERR_ARG, "pair histogram: too many pairs for one launch");
  // launched directly: nothing of the context but its device and stream is read, nothing is written (no bookkeeping of the
  // last launch, no timing slot)
  if (periodic) hipLaunchKernelGGL((rmb::pair_hist_kernel<true, true>), dim3((unsigned)blocks), dim3(64 * rmb::kSymWaves), dyn, c->stream, a);
  else hipLaunchKernelGGL((rmb::pair_hist_kernel<false, true>), dim3((unsigned)blocks), dim3(64 * rmb::kSymWaves), dyn, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
