// rmb_van_hove.hip -- lag histograms behind the van Hove functions G_s(r, t) and G_d(r, t) of caller-owned point frames
// (van_hove_kernels.h): the self sweep with its moments and finishing launch, and the distinct sweep over ordered pairs.
#include "lag_sweep_host.h"

#include <cmath>

#include "van_hove_kernels.h"

namespace rmbi {
namespace {

typedef rmb::VanHoveArgs A;

// Everything that can be refused without a context (the callers check that one last): the argument checks need no device.
int check_van_hove_args(const char* who, const void* frames, long n_frames, long n, long n_lags, long o_begin, long o_end, int plane,
                        double r_max, long n_bins, const void* hist) {
  const std::string w(who);
  if (!hist) return fail(RMB_ERR_ARG, w + ": null histogram pointer");
  if (int rc = check_frames(who, frames, n_frames, n, 3)) return rc;
  if (int rc = check_lag_range(who, n_frames, n_lags, o_begin, o_end)) return rc;
  if (plane != 0 && plane != 1) return fail(RMB_ERR_ARG, w + ": plane must be 0 (xyz) or 1 (xy)");
  if (!(r_max > 0.0) || !std::isfinite(r_max)) return fail(RMB_ERR_ARG, w + ": r_max must be positive and finite");
  if (n_bins < 1 || n_bins > rmb::kPairHistMaxBins) return fail(RMB_ERR_ARG, w + ": n_bins must be 1 ... 8192");
  return 0;
}

void fill_common(A& a, const double* frames, long n_frames, long n, long n_lags, long o_begin, long o_end, double r_max, long n_bins,
                 unsigned long long* hist) {
  a.frames = frames; a.F = n_frames; a.n = n;
  a.n_lags = n_lags; a.o_begin = o_begin; a.o_end = o_end;
  // the padding sentinels of the distinct sweep give r^2 >= 1e200: the gate stays below them whatever r_max
  a.r_max2 = std::fmin(r_max * r_max, 1e199);
  a.inv_dr = (double)n_bins / r_max;
  a.n_bins = (int)n_bins;
  a.hist = hist;
}

// the instance of a box and a plane: its host handle (occupancy) and its launch
struct DistinctKernel {
  const void* fn;
  void (*launch)(const A& a, long blocks, size_t dyn, hipStream_t s);
};

template <bool PERIODIC, bool XY, bool PZ>
void launch_distinct(const A& a, long blocks, size_t dyn, hipStream_t s) {
  hipLaunchKernelGGL((rmb::van_hove_distinct_kernel<PERIODIC, XY, PZ>), dim3((unsigned)blocks), dim3(rmb::kVhBlock), dyn, s, a);
}

template <bool PERIODIC, bool XY, bool PZ>
DistinctKernel distinct_of() {
  return DistinctKernel{(const void*)rmb::van_hove_distinct_kernel<PERIODIC, XY, PZ>, launch_distinct<PERIODIC, XY, PZ>};
}

DistinctKernel distinct_kernel(bool periodic, bool xy, bool pz) {
  if (!periodic) return xy ? distinct_of<false, true, false>() : distinct_of<false, false, false>();
  if (xy) return distinct_of<true, true, false>();
  return pz ? distinct_of<true, false, true>() : distinct_of<true, false, false>();
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

int rmb_van_hove_self_frames_device(rmb_ctx* c, const double* frames_dev, long n_frames, long n, long n_lags, long o_begin, long o_end, int plane,
                                    double r_max, long n_bins, unsigned long long* hist_dev, double* moments_dev) {
  if (int rc = rmbi::check_van_hove_args("van hove self", frames_dev, n_frames, n, n_lags, o_begin, o_end, plane, r_max, n_bins, hist_dev)) return rc;
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (n_frames == 0 || n == 0 || o_begin == o_end) return 0;
  rmbi::A a{};
  rmbi::fill_common(a, frames_dev, n_frames, n, n_lags, o_begin, o_end, r_max, n_bins, hist_dev);
  // Launch plan: a lag tile's counters fit kVhSelfCounters; about eight workgroups per CU over (lag tile, origin range, point
  // block); an origin range is short enough that no counter can reach 2^31 (256 points x 2^22 origins)
  const long n_origins = o_end - o_begin;
  a.lt = (int)(rmb::kVhSelfCounters / n_bins);
  if (a.lt > rmb::kVhLagTile) a.lt = rmb::kVhLagTile;
  if (a.lt > n_lags) a.lt = (int)n_lags;
  a.lag_tiles = (n_lags + a.lt - 1) / a.lt;
  a.point_blocks = (n + rmb::kVhBlock - 1) / rmb::kVhBlock;
  const long base = a.lag_tiles * a.point_blocks, target = 8 * c->n_cu;
  a.S = (target + base - 1) / base;
  const long s_min = (n_origins + rmb::kVhMaxOriginsPerWg - 1) / rmb::kVhMaxOriginsPerWg;
  if (a.S < s_min) a.S = s_min;
  if (a.S > n_origins) a.S = n_origins;
  if ((double)base * (double)a.S > 2147483647.0) return fail(RMB_ERR_ARG, "van hove self: too many terms for one launch");
  const long blocks = base * a.S;
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->vh_ws.reserve((size_t)blocks * 2 * rmb::kVhLagTile * sizeof(double))) return rc;
  a.part = (double*)c->vh_ws.p;
  a.moments = moments_dev;
  const size_t dyn = (size_t)a.lt * n_bins * sizeof(unsigned);
  if (plane) hipLaunchKernelGGL(rmb::van_hove_self_kernel<true>, dim3((unsigned)blocks), dim3(rmb::kVhBlock), dyn, c->stream, a);
  else       hipLaunchKernelGGL(rmb::van_hove_self_kernel<false>, dim3((unsigned)blocks), dim3(rmb::kVhBlock), dyn, c->stream, a);
  RMB_HIP(hipGetLastError());
  if (moments_dev) {
    hipLaunchKernelGGL(rmb::van_hove_moments_finish_kernel, dim3((unsigned)((2 * n_lags + 255) / 256)), dim3(256), 0, c->stream, a);
    RMB_HIP(hipGetLastError());
  }
  return 0;
}

int rmb_van_hove_distinct_frames_device(rmb_ctx* c, const double* frames_dev, long n_frames, long n, const double* L, long n_lags, long o_begin,
                                        long o_end, int plane, double r_max, long n_bins, unsigned long long* hist_dev) {
  if (int rc = rmbi::check_van_hove_args("van hove distinct", frames_dev, n_frames, n, n_lags, o_begin, o_end, plane, r_max, n_bins, hist_dev))
    return rc;
  if (!L) return fail(RMB_ERR_ARG, "van hove distinct: null periodic_length");
  const long tiles = (n + 63) / 64;
  if (tiles > 0x7fffffffL) return fail(RMB_ERR_ARG, "van hove distinct: too many points per frame");
  // the steps of the busiest lag, as rmb_pair_histogram_frames_device counts them
  if ((double)tiles * (double)tiles * (double)(o_end - o_begin) * 64.0 > 9.0e18)
    return fail(RMB_ERR_ARG, "van hove distinct: too many pairs for one launch");
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (n_frames == 0 || n < 2 || o_begin == o_end) return 0;
  rmbi::A a{};
  rmbi::fill_common(a, frames_dev, n_frames, n, n_lags, o_begin, o_end, r_max, n_bins, hist_dev);
  a.Lx = L[0]; a.Ly = L[1]; a.Lz = plane ? 0.0 : L[2];
  a.iLx = rmbi::inv_length(a.Lx); a.iLy = rmbi::inv_length(a.Ly); a.iLz = rmbi::inv_length(a.Lz);
  a.T = tiles;
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  const size_t dyn = (size_t)n_bins * sizeof(unsigned);
  RMB_HIP(hipSetDevice(c->device));
  // Launch plan: two resident rounds of workgroups over all lags (every workgroup ends with up to n_bins global atomics), P
  // per lag; at least one unit per wave of the busiest lag; P is raised until a workgroup meets fewer than 2^30 terms, and
  // the plan is refused if one launch has not that many workgroups
  const rmbi::DistinctKernel k = rmbi::distinct_kernel(periodic, plane != 0, a.Lz > 0);
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k.fn, rmb::kVhBlock, dyn) != hipSuccess || occ < 1) occ = 1;
  if (occ > 8) occ = 8;
  const long units = tiles * tiles * (o_end - o_begin);      // of lag 0, the busiest
  a.P = (2 * c->n_cu * occ + n_lags - 1) / n_lags;
  const long p_max = units / rmb::kVhWaves > 1 ? units / rmb::kVhWaves : 1;
  if (a.P > p_max) a.P = p_max;
  const long p_min = (units + rmb::kVhMaxUnitsPerWg - 1) / rmb::kVhMaxUnitsPerWg;
  if (a.P < p_min) a.P = p_min;
  if ((double)a.P * (double)n_lags > 2147483647.0) return fail(RMB_ERR_ARG, "van hove distinct: too many pairs for one launch");
  const long blocks = a.P * n_lags;
  // launched directly: nothing of the context but its device and stream is read, nothing is written
  k.launch(a, blocks, dyn, c->stream);
  RMB_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
