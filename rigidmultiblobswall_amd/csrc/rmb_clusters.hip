// rmb_clusters.hip -- connected components of the bond graph (cluster_kernels.h): cluster labels and sizes of a batch of
// caller-owned frames, and of the resident raw positions; what clusters.py streams a trajectory through.
#include "rmb_internal.h"

#include <cmath>
#include <limits>

#include "cluster_kernels.h"

namespace rmbi {
namespace {

typedef rmb::ClusterArgs A;

// everything that can be said without the context or the device
int check_cluster_args(const std::string& w, double r_cut, int plane, bool outputs) {
  if (!outputs) return fail(RMB_ERR_ARG, w + ": null labels or sizes pointer");
  if (!(r_cut > 0.0) || !std::isfinite(r_cut)) return fail(RMB_ERR_ARG, w + ": r_cut must be positive and finite");
  if (plane != 0 && plane != 1) return fail(RMB_ERR_ARG, w + ": plane must be 0 (xyz) or 1 (xy)");
  return 0;
}

template <bool BATCH>
SymKernel cluster_kernel_of(bool periodic) {
  const size_t slabs = sizeof(double4) * 64 * rmb::kSymWaves;
  return periodic ? sym_kernel_of<A, rmb::cluster_kernel<true, BATCH>>(slabs) : sym_kernel_of<A, rmb::cluster_kernel<false, BATCH>>(slabs);
}

// the parent array from the context's workspace, then the init launch (parent = identity, sizes = 0)
int cluster_begin(rmb_ctx* c, A& a, const unsigned char* select, double r_cut, int plane, int* labels, int* sizes) {
  if (int rc = c->cluster_ws.reserve((size_t)a.total * sizeof(int))) return rc;
  a.parent = (int*)c->cluster_ws.p;
  a.select = select; a.labels = labels; a.sizes = sizes;
  a.rc2 = r_cut * r_cut;
  a.xy = plane;
  hipLaunchKernelGGL(rmb::cluster_init_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

int rmb_cluster_labels_frames_device(rmb_ctx* c, const double* frames_dev, const unsigned char* select_dev_or_null, long n_frames, long n,
                                     const double* L, double r_cut, int plane, int* labels_dev, int* sizes_dev) {
  const std::string w("cluster labels");
  if (n_frames < 0 || n < 0) return fail(RMB_ERR_ARG, w + ": negative size");
  if (!L) return fail(RMB_ERR_ARG, w + ": null periodic_length");
  const bool nothing = n_frames == 0 || n == 0;      // empty outputs may be null
  if (int rc = rmbi::check_cluster_args(w, r_cut, plane, nothing || (labels_dev && sizes_dev))) return rc;
  if (!nothing && !frames_dev) return fail(RMB_ERR_ARG, w + ": null frames pointer");
  if ((double)n_frames * (double)n > 2147483647.0) return fail(RMB_ERR_ARG, w + ": too many points for one call (n_frames * n above 2^31 - 1)");
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (nothing) return 0;
  RMB_HIP(hipSetDevice(c->device));
  const long tiles = (n + 63) / 64;
  const long upf = tiles * (tiles + 1) / 2;
  if ((double)upf * (double)n_frames * 64.0 > 9.0e18) return fail(RMB_ERR_ARG, w + ": too many pairs for one launch");
  rmbi::A a{};
  a.n = n; a.n_tiles = (int)tiles;
  a.frames = frames_dev; a.units_per_frame = upf;
  a.step_end = upf * n_frames * 64;
  a.total = n_frames * n;
  a.Lx = L[0]; a.Ly = L[1]; a.Lz = plane ? 0.0 : L[2];
  a.iLx = rmbi::inv_length(a.Lx); a.iLy = rmbi::inv_length(a.Ly); a.iLz = rmbi::inv_length(a.Lz);
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  const rmbi::SymKernel k = rmbi::cluster_kernel_of<true>(periodic);
  // the plan of the culling sweeps with "sym_oversub" rounds: a workgroup ends with nothing to flush, and the plan changes
  // neither the partition nor a label
  long blocks;
  rmbi::plan_cull_sweep(c, k, a.step_end, &blocks, &a.chunk_steps);
  if (int rc = rmbi::cluster_begin(c, a, select_dev_or_null, r_cut, plane, labels_dev, sizes_dev)) return rc;
  // launched directly: of the context only the device, the stream and the parent workspace are used
  k.launch(&a, rmb::PairConsts{}, (unsigned)blocks, 0, c->stream);
  RMB_HIP(hipGetLastError());
  hipLaunchKernelGGL(rmb::cluster_finish_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}

int rmb_cluster_labels_device(rmb_ctx* c, const unsigned char* select_dev_or_null, double r_cut, int plane, int* labels_dev, int* sizes_dev) {
  const std::string w("cluster labels");
  if (int rc = rmbi::check_cluster_args(w, r_cut, plane, labels_dev && sizes_dev)) return rc;
  if (int rc = rmbi::check_ready(c)) return rc;
  if (c->n > 0x7fffffffL) return fail(RMB_ERR_ARG, w + ": too many points (more than 2^31 - 1)");
  rmbi::A a{};
  // spatial order, tile bounds and the frame's arguments, with a fresh Morton permutation (as the pair histogram)
  const rmbi::PairOnceErrors msg{"cluster labels use raw positions: call rmb_set_positions with wall = 0",
                                 "cluster labels run over all points: reset the target range", "cluster labels: more than 2^32 points"};
  bool empty;
  if (int rc = rmbi::pair_once_prepare(c, a, msg, 1, false, &empty)) return rc;
  if (empty) return 0;
  a.total = c->n;
  a.Lz = plane ? 0.0 : c->L[2]; a.iLz = rmbi::inv_length(a.Lz);
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  a.cull2 = c->opt_force_cull ? r_cut * r_cut : std::numeric_limits<double>::infinity();
  const rmbi::SymKernel k = rmbi::cluster_kernel_of<false>(periodic);
  long blocks;
  rmbi::plan_cull_sweep(c, k, a.step_end, &blocks, &a.chunk_steps);
  if (int rc = rmbi::cluster_begin(c, a, select_dev_or_null, r_cut, plane, labels_dev, sizes_dev)) return rc;
  return rmbi::sym_launch(c, k, 1, blocks, 0, a, rmb::PairConsts{}, rmb::cluster_finish_kernel, (a.total + 255) / 256);
}

}  // extern "C"
