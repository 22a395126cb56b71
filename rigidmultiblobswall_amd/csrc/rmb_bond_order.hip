// rmb_bond_order.hip -- bond-orientational order of caller-owned point frames (bond_order_kernels.h): the neighbour sums
// behind psi_m(i) (a policy of the one-sided frame, the frame of the trajectory a grid dimension) and the pair correlation of
// a quantised per-point field behind g_m(r) (a policy of the pair-once frame, integer accumulators).
#include "rmb_internal.h"

#include <cmath>

#include "bond_order_kernels.h"

namespace rmbi {
namespace {

constexpr long kMaxGridFrames = 65535;      // gridDim.z / gridDim.y of one launch

int check_box_plane(const std::string& w, const double* L, int plane) {
  if (!L) return fail(RMB_ERR_ARG, w + ": null periodic_length");
  if (plane != 0 && plane != 1) return fail(RMB_ERR_ARG, w + ": plane must be 0 (xyz) or 1 (xy)");
  return 0;
}

int check_frames_arg(const std::string& w, const void* frames, long n_frames, long n) {
  if (n_frames < 0 || n < 0) return fail(RMB_ERR_ARG, w + ": negative size");
  if ((double)n_frames * (double)n > 1.0e17) return fail(RMB_ERR_ARG, w + ": too many frames for one call");
  if (n_frames > 0 && n > 0 && !frames) return fail(RMB_ERR_ARG, w + ": null frames pointer");
  return 0;
}

typedef rmb::PairFieldArgs FA;

SymKernel field_kernel(bool periodic) {
  const size_t slabs = sizeof(double4) * 64 * rmb::kSymWaves;
  return periodic ? sym_kernel_of<FA, rmb::pair_field_kernel<true>>(slabs) : sym_kernel_of<FA, rmb::pair_field_kernel<false>>(slabs);
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

int rmb_bond_order_frames_device(rmb_ctx* c, const double* frames_dev, long n_frames, long n, const double* L, double r_cut, int plane,
                                 const int* orders, int n_orders, long source_chunk, double* out_dev) {
  const std::string w("bond order");
  if (int rc = rmbi::check_frames_arg(w, frames_dev, n_frames, n)) return rc;
  if (int rc = rmbi::check_box_plane(w, L, plane)) return rc;
  if (!(r_cut > 0.0) || !std::isfinite(r_cut)) return fail(RMB_ERR_ARG, w + ": r_cut must be positive and finite");
  if (!orders) return fail(RMB_ERR_ARG, w + ": null orders pointer");
  if (n_orders < 1 || n_orders > rmb::kBondMaxOrders) return fail(RMB_ERR_ARG, w + ": n_orders must be 1 ... 4");
  for (int k = 0; k < n_orders; ++k)
    if (orders[k] < 1 || orders[k] > rmb::kBondMaxOrder) return fail(RMB_ERR_ARG, w + ": every order must be 1 ... 16");
  if (source_chunk < 0) return fail(RMB_ERR_ARG, w + ": source_chunk must not be negative");
  if (n_frames > 0 && n > 0 && !out_dev) return fail(RMB_ERR_ARG, w + ": null output pointer");
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (n_frames == 0 || n == 0) return 0;
  RMB_HIP(hipSetDevice(c->device));

  typedef rmb::BondOrderArgs A;
  constexpr int NOUT = 1 + 2 * rmb::kBondMaxOrders;
  A a{};
  a.n_src = n; a.tgt_begin = 0; a.tgt_end = n;
  a.rc2 = r_cut * r_cut;
  a.xy = plane;
  a.Lx = L[0]; a.Ly = L[1]; a.Lz = plane ? 0.0 : L[2];
  a.iLx = rmbi::inv_length(a.Lx); a.iLy = rmbi::inv_length(a.Ly); a.iLz = rmbi::inv_length(a.Lz);
  a.n_orders = n_orders;
  for (int k = 0; k < n_orders; ++k) a.orders[k] = orders[k];
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  const void* fn = periodic ? (const void*)rmb::bond_order_kernel<true> : (const void*)rmb::bond_order_kernel<false>;
  static int occ[2] = {0, 0};

  // Chunk plan of one frame (choose_chunks) on the frame's share of the resident workgroups; a forced source_chunk is
  // rounded up to whole groups of kWaves sources
  const long tiles = (n + 63) / 64;
  if (tiles > 0x7fffffffL) return fail(RMB_ERR_ARG, w + ": too many points per frame");
  const long batch = n_frames < rmbi::kMaxGridFrames ? n_frames : rmbi::kMaxGridFrames;
  long n_chunks, chunk_len;
  if (source_chunk > 0) {
    chunk_len = ((source_chunk + rmb::kWaves - 1) / rmb::kWaves) * rmb::kWaves;
    n_chunks = (n + chunk_len - 1) / chunk_len;
  } else {
    long slots = c->n_cu * rmbi::resident_blocks(fn, &occ[periodic ? 1 : 0]) / batch;
    if (slots < 1) slots = 1;
    rmbi::choose_chunks(n, n, 0, slots, &n_chunks, &chunk_len);
  }
  if (n_chunks > 65535) return fail(RMB_ERR_ARG, w + ": source_chunk makes more than 65535 chunks");
  a.n_tgt_pad = 64 * tiles;
  a.chunk_len = chunk_len;
  a.n_chunks = (int)n_chunks;
  a.out_stride = n * (1 + 2 * n_orders);
  a.partial_stride = n_chunks * NOUT * a.n_tgt_pad;
  a.partial = nullptr;
  if (n_chunks > 1) {
    if ((double)batch * (double)a.partial_stride * 8.0 > 6.0e10) return fail(RMB_ERR_ARG, w + ": the chunk partials would not fit; use fewer frames per call");
    if (int rc = c->partial.reserve((size_t)batch * a.partial_stride * sizeof(double))) return rc;
    a.partial = (double*)c->partial.p;
  }
  // launched directly: of the context only the device, the stream and the workspace of chunk partials are used
  for (long f0 = 0; f0 < n_frames; f0 += batch) {
    const long nf = n_frames - f0 < batch ? n_frames - f0 : batch;
    a.frames = frames_dev + 3 * n * f0;
    a.out = out_dev + a.out_stride * f0;
    const dim3 grid((unsigned)tiles, (unsigned)n_chunks, (unsigned)nf);
    if (periodic) hipLaunchKernelGGL(rmb::bond_order_kernel<true>, grid, dim3(rmb::kBlock), 0, c->stream, a);
    else          hipLaunchKernelGGL(rmb::bond_order_kernel<false>, grid, dim3(rmb::kBlock), 0, c->stream, a);
    RMB_HIP(hipGetLastError());
    if (n_chunks > 1) {
      hipLaunchKernelGGL(rmb::bond_order_finalize_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)nf), dim3(256), 0, c->stream, a);
      RMB_HIP(hipGetLastError());
    }
  }
  return 0;
}

int rmb_pair_field_frames_device(rmb_ctx* c, const double* frames_dev, const int* field_dev, long n_frames, long n, const double* L, int plane,
                                 double r_max, long n_bins, unsigned long long* counts_dev, long long* sums_dev) {
  const std::string w("pair field");
  if (!counts_dev || !sums_dev) return fail(RMB_ERR_ARG, w + ": null counts or sums pointer");
  if (int rc = rmbi::check_frames_arg(w, frames_dev, n_frames, n)) return rc;
  if (n_frames > 0 && n > 0 && !field_dev) return fail(RMB_ERR_ARG, w + ": null field pointer");
  if (int rc = rmbi::check_box_plane(w, L, plane)) return rc;
  if (!(r_max > 0.0) || !std::isfinite(r_max)) return fail(RMB_ERR_ARG, w + ": r_max must be positive and finite");
  if (n_bins < 1 || n_bins > rmb::kPairFieldMaxBins) return fail(RMB_ERR_ARG, w + ": n_bins must be 1 ... 4096");
  const long tiles = (n + 63) / 64;
  if (tiles > 0x7fffffffL) return fail(RMB_ERR_ARG, w + ": too many points per frame");
  const long upf = tiles * (tiles + 1) / 2;
  if ((double)upf * (double)n_frames * 64.0 > 9.0e18) return fail(RMB_ERR_ARG, w + ": too many pairs for one launch");
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (n_frames == 0 || n < 2) return 0;
  RMB_HIP(hipSetDevice(c->device));
  rmbi::FA a{};
  a.n = n; a.n_tiles = (int)tiles;
  a.frames = frames_dev; a.field = (const long long*)field_dev; a.units_per_frame = upf;
  a.step_end = upf * n_frames * 64;
  a.xy = plane;
  a.Lx = L[0]; a.Ly = L[1]; a.Lz = plane ? 0.0 : L[2];
  a.iLx = rmbi::inv_length(a.Lx); a.iLy = rmbi::inv_length(a.Ly); a.iLz = rmbi::inv_length(a.Lz);
  a.r_max2 = std::fmin(r_max * r_max, 1e199);      // the padding sentinels give r^2 >= 1e200: the gate stays below them
  a.inv_dr = (double)n_bins / r_max;
  a.n_bins = (int)n_bins;
  a.counts = counts_dev; a.sums = sums_dev;
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  const size_t dyn = (size_t)n_bins * (sizeof(long long) + sizeof(unsigned));
  const rmbi::SymKernel k = rmbi::field_kernel(periodic);
  // the pair histogram's plan: two resident rounds, refined until a workgroup meets fewer than 2^31 pairs (the uint32 counts
  // cannot wrap, the int64 sums stay below 2^62)
  long blocks;
  if (int rc = rmbi::plan_cull_sweep(c, k, a.step_end, &blocks, &a.chunk_steps, 2, dyn, 2147483648.0, "pair field")) return rc;
  // launched directly: nothing of the context but its device and stream is read, nothing is written
  k.launch(&a, rmb::PairConsts{}, (unsigned)blocks, dyn, c->stream);
  RMB_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
