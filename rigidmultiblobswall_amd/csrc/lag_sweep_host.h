// lag_sweep_host.h -- host side shared by the trajectory analyses over lags (rmb_msd.hip, rmb_scattering.hip,
// rmb_van_hove.hip): the argument checks of a batch of caller-owned frames and of a lag / origin range, and the launch plan
// of the lag sweeps (lag_sweep_kernels.h).
#pragma once
#include "rmb_internal.h"

#include "lag_sweep_kernels.h"

namespace rmbi {

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// `ptr`: n_frames frames of n rows of `width` doubles, named `what` in the null-pointer refusal
inline int check_frames(const char* who, const void* ptr, long n_frames, long n, int width, const char* what = "frames") {
  const std::string w(who);
  if (n_frames < 0 || n < 0) return fail(RMB_ERR_ARG, w + ": negative size");
  if ((double)n_frames * (double)n * (double)width > 1.0e18) return fail(RMB_ERR_ARG, w + ": too many frames for one call");
  if (n_frames > 0 && n > 0 && !ptr) return fail(RMB_ERR_ARG, w + ": null " + what + " pointer");
  return 0;
}

inline int check_lag_range(const char* who, long n_frames, long n_lags, long o_begin, long o_end) {
  const std::string w(who);
  if (n_lags < 1) return fail(RMB_ERR_ARG, w + ": n_lags must be at least 1");
  if (n_lags > (1L << 24)) return fail(RMB_ERR_ARG, w + ": n_lags must be at most 2^24");
  if (o_begin < 0 || o_end < o_begin || o_end > n_frames) return fail(RMB_ERR_ARG, w + ": origins must satisfy 0 <= o_begin <= o_end <= n_frames");
  return 0;
}

// Launch plan of a lag sweep over `rows` rows of `series` series each, windows of at most `chunk` origins: about eight
// workgroups per CU over all rows and lag blocks (the sweeps are VALU-bound with 4 waves per workgroup; more workgroups
// only add partials), never more than a row has work items.  Needs o_begin < o_end.  Fills everything of `a` but rec / part.
inline int plan_lag_sweep(rmb_ctx* c, rmb::LagSweepArgs& a, const char* who, long n_frames, long series, long rows, long n_lags, long o_begin,
                          long o_end, long chunk) {
  const std::string w(who);
  a.F = n_frames; a.B = series;
  a.n_lags = n_lags; a.lag_blocks = (n_lags + 63) / 64;
  a.o_begin = o_begin; a.o_end = o_end;
  const long n_origins = o_end - o_begin;
  a.chunk = chunk < n_origins ? chunk : n_origins;
  a.n_chunks = (n_origins + a.chunk - 1) / a.chunk;
  if ((double)a.n_chunks * (double)series > 4.0e18) return fail(RMB_ERR_ARG, w + ": too many work items for one call");      // items
  a.items = a.n_chunks * series;
  const long per = a.lag_blocks * rows, target = 8 * c->n_cu;
  a.P = (target + per - 1) / per;
  if (a.P > a.items) a.P = a.items;
  if ((double)a.items * (double)(a.P + 1) > 9.0e18) return fail(RMB_ERR_ARG, w + ": too many work items for one call");      // items * p in the kernel
  if (a.P * a.lag_blocks > 0x7fffffffL) return fail(RMB_ERR_ARG, w + ": too many lag blocks for one launch");
  return 0;
}

}  // namespace rmbi
