// rmb_potential.hip -- total potential energy of the resident blob configuration (potential_kernels.h) and the Metropolis
// proposal of the equilibrium sampler (many_bodyMCMC/many_body_potential_pycuda.py, many_body_MCMC.py:158-169).
#include "rmb_internal.h"

#include <cmath>
#include <limits>

#include "potential_kernels.h"

namespace rmbi {
namespace {

// The sweep + the finishing launch on the context's stream; the two sums end up in out_dev[0..1].
// `body`: the resident points are body locations and the energy is the body-body Yukawa law's (the BODY instance of
// potential_kernels.h): the yukawa pair expression without contact distance, wall gate and one-blob term, imaged in all three
// directions; ONE sum in out_dev[0].
// `table`: the pair term is the context's tabulated law (the TABLE instances): eps and b are not read, the reach is r_cut,
// the records are staged in tab_k * 32 bytes of dynamic LDS; the one-blob term and the wall gate are `form`'s as ever.
int potential_device_impl(rmb_ctx* c, double eps, double b, double eps_wall, double b_wall, double weight, double blob_radius, int form,
                          double* out_dev, bool body = false, bool table = false) {
  if (int rc = check_ready(c)) return rc;
  if (!out_dev) return fail(RMB_ERR_ARG, "null output pointer");
  if (form != rmb::POT_SOFT && form != rmb::POT_YUKAWA) return fail(RMB_ERR_ARG, "potential form must be 0 (soft) or 1 (yukawa)");
  if (table && c->tab_k == 0) return fail(RMB_ERR_STATE, "no pair table is set: call rmb_ctx_set_pair_table");
  if (table) { eps = 0.0; b = 1.0; }
  if (!(b > 0.0)) return fail(RMB_ERR_ARG, "debye_length must be positive");
  if (eps_wall != 0.0 && !(b_wall > 0.0)) return fail(RMB_ERR_ARG, "debye_length_wall must be positive when repulsion_strength_wall is not zero");
  typedef rmb::PotentialArgs A;
  A a;
  // spatial order, tile bounds and the frame's arguments; the Morton permutation ages by "potential_resort"
  const PairOnceErrors msg{body ? "the body-body potential uses raw locations: call rmb_set_positions with wall = 0"
                                : "the potential uses raw heights: call rmb_set_positions with wall = 0",
                           "the potential is a sum over all blobs: reset the target range", "potential: more than 2^32 blobs"};
  bool empty;
  if (int rc = pair_once_prepare(c, a, msg, 1, true, &empty)) return rc;
  if (empty) { RMB_HIP(hipMemsetAsync(out_dev, 0, (body ? 1 : 2) * sizeof(double), c->stream)); return 0; }
  // x and y only (fill_sym_args): the reference ignores periodic_length[2]; the body centres alone see the z period
  a.Lz = body ? c->L[2] : 0.0; a.iLz = inv_length(a.Lz);
  a.n_out = body ? 1 : 2;
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  a.eps = eps; a.inv_b = 1.0 / b; a.two_a = 2.0 * blob_radius;
  a.eps_wall = eps_wall; a.inv_b_wall = eps_wall != 0.0 ? 1.0 / b_wall : 0.0; a.a = blob_radius; a.weight = weight;
  a.ec = exp_consts();
  const double reach = form == rmb::POT_SOFT ? 2.0 * blob_radius + 750.0 * b : 750.0 * b;
  a.tab = table ? pair_table_ref(c) : rmb::PairTableRef{};
  a.cull2 = !c->opt_force_cull ? std::numeric_limits<double>::infinity() : table ? a.tab.rcut2 : reach * reach;
  const size_t dyn_lds = table ? (size_t)c->tab_k * sizeof(double4) : 0;

  const SymKernel k = table ? (form == rmb::POT_SOFT
                                   ? (periodic ? sym_kernel_of<A, rmb::potential_kernel<rmb::POT_SOFT, true, false, true>>(0)
                                               : sym_kernel_of<A, rmb::potential_kernel<rmb::POT_SOFT, false, false, true>>(0))
                                   : (periodic ? sym_kernel_of<A, rmb::potential_kernel<rmb::POT_YUKAWA, true, false, true>>(0)
                                               : sym_kernel_of<A, rmb::potential_kernel<rmb::POT_YUKAWA, false, false, true>>(0)))
                      : body ? (periodic ? sym_kernel_of<A, rmb::potential_kernel<rmb::POT_YUKAWA, true, true>>(0)
                                       : sym_kernel_of<A, rmb::potential_kernel<rmb::POT_YUKAWA, false, true>>(0))
                      : form == rmb::POT_SOFT
                          ? (periodic ? sym_kernel_of<A, rmb::potential_kernel<rmb::POT_SOFT, true>>(0) : sym_kernel_of<A, rmb::potential_kernel<rmb::POT_SOFT, false>>(0))
                          : (periodic ? sym_kernel_of<A, rmb::potential_kernel<rmb::POT_YUKAWA, true>>(0)
                                      : sym_kernel_of<A, rmb::potential_kernel<rmb::POT_YUKAWA, false>>(0));
  long blocks;
  plan_cull_sweep(c, k, a.step_end, &blocks, &a.chunk_steps, 0, dyn_lds);
  const long waves = blocks * rmb::kSymWaves;
  if (int rc = c->pot_ws.reserve((size_t)(2 * waves + 2) * sizeof(double))) return rc;
  a.partial = (double*)c->pot_ws.p;
  a.n_partial = waves;
  a.out = out_dev;
  return sym_launch(c, k, 1, blocks, dyn_lds, a, rmb::PairConsts{}, rmb::potential_finish_kernel, 1);
}

struct ProposeArgs {
  long n_bodies, n_free, n_blobs;
  const int* blob_body;   // [n_blobs] body of every blob (bodies in order)
  const int* blob_ref;    // [n_blobs] row of `ref` that is this blob's body-frame position
  const double* ref;      // (rows, 3) reference configurations of every structure
  const double *loc, *quat, *draws;
  double max_angle_shift;
  double *loc_new, *quat_new, *r_new;
};

// many_body_MCMC.py:160-169 for every body at once: x' = x + du, q' = quaternion(dphi) q (quaternion.py:17-39), bodies from
// n_free on keep theirs; r = R(q') ref + x' for every blob (body.py:64-78).  One thread per blob; the first blob of a
// body also stores the body's proposal.
__global__ __launch_bounds__(256) void mcmc_propose_kernel(const ProposeArgs a) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= a.n_blobs) return;
  const long b = a.blob_body[id];
  double x = a.loc[3 * b], y = a.loc[3 * b + 1], z = a.loc[3 * b + 2];
  double s = a.quat[4 * b], p0 = a.quat[4 * b + 1], p1 = a.quat[4 * b + 2], p2 = a.quat[4 * b + 3];
  if (b < a.n_free) {
    const double* d = a.draws + 6 * b;
    x += d[0]; y += d[1]; z += d[2];
    const double px = d[3] * a.max_angle_shift, py = d[4] * a.max_angle_shift, pz = d[5] * a.max_angle_shift;
    const double nrm = sqrt(px * px + py * py + pz * pz);
    const double qs = cos(0.5 * nrm), f = nrm != 0.0 ? sin(0.5 * nrm) / nrm : 0.0;
    const double qx = f * px, qy = f * py, qz = f * pz;
    const double ns = qs * s - (qx * p0 + qy * p1 + qz * p2);
    const double n0 = qs * p0 + s * qx + (qy * p2 - qz * p1);
    const double n1 = qs * p1 + s * qy + (qz * p0 - qx * p2);
    const double n2 = qs * p2 + s * qz + (qx * p1 - qy * p0);
    s = ns; p0 = n0; p1 = n1; p2 = n2;
  }
  if (id == 0 || a.blob_body[id - 1] != b) {
    a.loc_new[3 * b] = x; a.loc_new[3 * b + 1] = y; a.loc_new[3 * b + 2] = z;
    a.quat_new[4 * b] = s; a.quat_new[4 * b + 1] = p0; a.quat_new[4 * b + 2] = p1; a.quat_new[4 * b + 3] = p2;
  }
  const double* rf = a.ref + 3L * a.blob_ref[id];
  const double d = s * s - 0.5;
  const double rx = 2.0 * ((p0 * p0 + d) * rf[0] + (p0 * p1 - s * p2) * rf[1] + (p0 * p2 + s * p1) * rf[2]);
  const double ry = 2.0 * ((p1 * p0 + s * p2) * rf[0] + (p1 * p1 + d) * rf[1] + (p1 * p2 - s * p0) * rf[2]);
  const double rz = 2.0 * ((p2 * p0 - s * p1) * rf[0] + (p2 * p1 + s * p0) * rf[1] + (p2 * p2 + d) * rf[2]);
  a.r_new[3 * id] = rx + x; a.r_new[3 * id + 1] = ry + y; a.r_new[3 * id + 2] = rz + z;
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

int rmb_blob_potential_device(rmb_ctx* c, double eps, double b, double eps_wall, double b_wall, double weight, double blob_radius, int form,
                              double* out_dev) {
  return rmbi::potential_device_impl(c, eps, b, eps_wall, b_wall, weight, blob_radius, form, out_dev);
}

int rmb_blob_potential(rmb_ctx* c, double eps, double b, double eps_wall, double b_wall, double weight, double blob_radius, int form,
                       double* out) {
  if (int rc = rmbi::check_ready(c)) return rc;
  if (!out) return fail(RMB_ERR_ARG, "null output pointer");
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->out.reserve(2 * sizeof(double))) return rc;
  if (int rc = rmbi::potential_device_impl(c, eps, b, eps_wall, b_wall, weight, blob_radius, form, (double*)c->out.p)) return rc;
  RMB_HIP(hipMemcpyAsync(out, c->out.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RMB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int rmb_blob_potential_table_device(rmb_ctx* c, double eps_wall, double b_wall, double weight, double blob_radius, int form, double* out_dev) {
  return rmbi::potential_device_impl(c, 0.0, 1.0, eps_wall, b_wall, weight, blob_radius, form, out_dev, false, true);
}

int rmb_blob_potential_table(rmb_ctx* c, double eps_wall, double b_wall, double weight, double blob_radius, int form, double* out) {
  if (int rc = rmbi::check_ready(c)) return rc;
  if (!out) return fail(RMB_ERR_ARG, "null output pointer");
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->out.reserve(2 * sizeof(double))) return rc;
  if (int rc = rmb_blob_potential_table_device(c, eps_wall, b_wall, weight, blob_radius, form, (double*)c->out.p)) return rc;
  RMB_HIP(hipMemcpyAsync(out, c->out.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RMB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int rmb_body_body_potential_device(rmb_ctx* c, double eps, double b, double* out_dev) {
  return rmbi::potential_device_impl(c, eps, b, 0.0, 1.0, 0.0, 0.0, rmb::POT_YUKAWA, out_dev, true);
}

int rmb_body_body_potential(rmb_ctx* c, double eps, double b, double* out) {
  if (int rc = rmbi::check_ready(c)) return rc;
  if (!out) return fail(RMB_ERR_ARG, "null output pointer");
  RMB_HIP(hipSetDevice(c->device));
  if (int rc = c->out.reserve(sizeof(double))) return rc;
  if (int rc = rmb_body_body_potential_device(c, eps, b, (double*)c->out.p)) return rc;
  RMB_HIP(hipMemcpyAsync(out, c->out.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RMB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int rmb_potential_oneshot(long n, const double* r, const double* L, double eps, double b, double eps_wall, double b_wall, double weight,
                          double blob_radius, int form, double* out) {
  std::lock_guard<std::mutex> lk(rmbi::g_default_mu);
  rmb_ctx* c;
  if (int rc = rmbi::default_ctx(&c)) return rc;
  if (int rc = rmb_set_positions(c, r, n, blob_radius, L, 0)) return rc;
  return rmb_blob_potential(c, eps, b, eps_wall, b_wall, weight, blob_radius, form, out);
}

int rmb_mcmc_propose_device(rmb_ctx* c, long n_bodies, long n_free, long n_blobs, const int* blob_body_dev, const int* blob_ref_dev,
                            const double* ref_dev, const double* loc_dev, const double* quat_dev, const double* draws_dev,
                            double max_angle_shift, double* loc_new_dev, double* quat_new_dev, double* r_new_dev) {
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (n_bodies < 0 || n_blobs < 0 || n_free < 0 || n_free > n_bodies) return fail(RMB_ERR_ARG, "rmb_mcmc_propose_device: bad sizes");
  if (n_blobs == 0) return 0;
  if (!blob_body_dev || !blob_ref_dev || !ref_dev || !loc_dev || !quat_dev || !loc_new_dev || !quat_new_dev || !r_new_dev ||
      (n_free > 0 && !draws_dev))
    return fail(RMB_ERR_ARG, "rmb_mcmc_propose_device: null pointer");
  RMB_HIP(hipSetDevice(c->device));
  rmbi::ProposeArgs a{n_bodies, n_free, n_blobs, blob_body_dev, blob_ref_dev, ref_dev, loc_dev, quat_dev, draws_dev, max_angle_shift,
                      loc_new_dev, quat_new_dev, r_new_dev};
  hipLaunchKernelGGL(rmbi::mcmc_propose_kernel, dim3((unsigned)((n_blobs + 255) / 256)), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
