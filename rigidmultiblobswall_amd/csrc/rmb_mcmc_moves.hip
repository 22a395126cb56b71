// rmb_mcmc_moves.hip -- single-body Metropolis moves of the equilibrium sampler (mcmc_move_kernels.h): the energy
// difference of one moved body on caller-supplied coordinates, and one sweep over the free bodies inside the library
// (two launches per move, no host synchronisation and no copy command between moves).  The *_bb entries add the body-body
// Yukawa energy of the body locations (the BODY instances) as a third difference / running sum.
#include "rmb_internal.h"

#include "mcmc_move_kernels.h"

namespace rmbi {
namespace {

typedef rmb::MoveArgs A;

int check_potential(const char* who, double b, double eps_wall, double b_wall, int form) {
  if (form != rmb::POT_SOFT && form != rmb::POT_YUKAWA) return fail(RMB_ERR_ARG, std::string(who) + ": potential form must be 0 (soft) or 1 (yukawa)");
  if (!(b > 0.0)) return fail(RMB_ERR_ARG, std::string(who) + ": debye_length must be positive");
  if (eps_wall != 0.0 && !(b_wall > 0.0))
    return fail(RMB_ERR_ARG, std::string(who) + ": debye_length_wall must be positive when repulsion_strength_wall is not zero");
  return 0;
}

// x and y only: the reference ignores periodic_length[2]
void fill_potential(A& a, const double* L, double eps, double b, double eps_wall, double b_wall, double weight, double blob_radius) {
  a.p = rmb::PotentialArgs{};
  a.p.Lx = L[0]; a.p.Ly = L[1];
  a.p.iLx = inv_length(L[0]); a.p.iLy = inv_length(L[1]);
  a.p.eps = eps; a.p.inv_b = 1.0 / b; a.p.two_a = 2.0 * blob_radius;
  a.p.eps_wall = eps_wall; a.p.inv_b_wall = eps_wall != 0.0 ? 1.0 / b_wall : 0.0; a.p.a = blob_radius; a.p.weight = weight;
  a.p.ec = exp_consts();
}

// The body-body law of the *_bb entries (nullptr: the entries without the centre term)
struct BodyLaw { long n_bodies; double eps, b; };

// the centre term sees the z period too; the blob terms never read it
void fill_body_law(A& a, const double* L, const BodyLaw& law) {
  a.p.Lz = L[2]; a.p.iLz = inv_length(L[2]);
  a.n_bodies = law.n_bodies; a.body_eps = law.eps; a.body_inv_b = 1.0 / law.b;
}

typedef void (*MoveKernel)(A);
template <bool COMPOSE, bool BODY>
MoveKernel delta_kernel_of(int form, bool periodic) {
  if (form == rmb::POT_SOFT)
    return periodic ? rmb::body_delta_kernel<rmb::POT_SOFT, true, COMPOSE, BODY> : rmb::body_delta_kernel<rmb::POT_SOFT, false, COMPOSE, BODY>;
  return periodic ? rmb::body_delta_kernel<rmb::POT_YUKAWA, true, COMPOSE, BODY> : rmb::body_delta_kernel<rmb::POT_YUKAWA, false, COMPOSE, BODY>;
}
template <bool COMPOSE>
MoveKernel delta_kernel_of(int form, bool periodic, bool body) {
  return body ? delta_kernel_of<COMPOSE, true>(form, periodic) : delta_kernel_of<COMPOSE, false>(form, periodic);
}

// The context's scratch of the moves: [sums n_waves] partials (sums = 2, with the centre term 3), then [3 max_count + 7] the
// proposed body.  Sized once per call.
int reserve_scratch(rmb_ctx* c, long blocks, long max_count, int sums, A& a) {
  const long n_waves = blocks * rmb::kMoveWaves;
  if (int rc = c->mcmc_ws.reserve((size_t)(sums * n_waves + 3 * max_count + 7) * sizeof(double))) return rc;
  a.partial = (double*)c->mcmc_ws.p;
  a.n_partial = n_waves;
  a.prop = a.partial + sums * n_waves;
  return 0;
}

int delta_impl(const char* who, rmb_ctx* c, long n_blobs, const double* r_dev, long first, long count, const double* r_body_new_dev,
               const double* periodic_length, double eps, double b, double eps_wall, double b_wall, double weight, double blob_radius, int form,
               double* out_dev, const BodyLaw* law, const double* loc_dev, long body, const double* loc_new_dev) {
  const std::string w(who);
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (!r_dev || !r_body_new_dev || !periodic_length || !out_dev) return fail(RMB_ERR_ARG, w + ": null pointer");
  if (n_blobs <= 0 || first < 0 || count <= 0 || first + count > n_blobs) return fail(RMB_ERR_ARG, w + ": bad blob range");
  if (int rc = check_potential(who, b, eps_wall, b_wall, form)) return rc;
  long lanes = n_blobs;
  if (law) {
    if (!loc_dev || !loc_new_dev) return fail(RMB_ERR_ARG, w + ": null pointer");
    if (law->n_bodies <= 0 || body < 0 || body >= law->n_bodies) return fail(RMB_ERR_ARG, w + ": bad body index");
    if (!(law->b > 0.0)) return fail(RMB_ERR_ARG, w + ": the body-body debye_length must be positive");
    if (law->n_bodies > lanes) lanes = law->n_bodies;
  }
  const long blocks = (lanes + rmb::kMoveChunk - 1) / rmb::kMoveChunk;
  if (blocks > 0x7fffffffL) return fail(RMB_ERR_ARG, w + ": too many blobs for one launch");
  RMB_HIP(hipSetDevice(c->device));
  A a{};
  fill_potential(a, periodic_length, eps, b, eps_wall, b_wall, weight, blob_radius);
  a.r = r_dev; a.n = n_blobs; a.first = first; a.count = count; a.body_new = r_body_new_dev;
  a.out = out_dev; a.decide = 0;
  if (law) { fill_body_law(a, periodic_length, *law); a.loc = loc_dev; a.body = body; a.loc_new3 = loc_new_dev; }
  if (int rc = reserve_scratch(c, blocks, 0, law ? 3 : 2, a)) return rc;
  const bool periodic = a.p.Lx > 0 || a.p.Ly > 0 || a.p.Lz > 0;
  hipLaunchKernelGGL(delta_kernel_of<false>(form, periodic, law != nullptr), dim3((unsigned)blocks), dim3(rmb::kMoveChunk), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  if (law) hipLaunchKernelGGL(rmb::move_finish_kernel<true>, dim3(1), dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL(rmb::move_finish_kernel<false>, dim3(1), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}

int sweep_impl(const char* who, rmb_ctx* c, long n_bodies, long n_free, long n_blobs, const long* body_first, const int* blob_ref_dev,
               const double* ref_dev, double* loc_dev, double* quat_dev, double* r_dev, const double* draws_dev, double max_angle_shift,
               const double* periodic_length, double eps, double b, double eps_wall, double b_wall, double weight, double blob_radius, int form,
               double kT, double* energy_dev, int* accepted_dev, const BodyLaw* law) {
  const std::string w(who);
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (n_bodies < 0 || n_blobs < 0 || n_free < 0 || n_free > n_bodies) return fail(RMB_ERR_ARG, w + ": bad sizes");
  if (int rc = check_potential(who, b, eps_wall, b_wall, form)) return rc;
  if (law && !(law->b > 0.0)) return fail(RMB_ERR_ARG, w + ": the body-body debye_length must be positive");
  if (!(kT > 0.0)) return fail(RMB_ERR_ARG, w + ": kT must be positive");
  if (!body_first || !periodic_length) return fail(RMB_ERR_ARG, w + ": null pointer");
  // the bodies' blob ranges tile [0, n_blobs) in order
  long max_count = 0;
  if (body_first[0] != 0 || body_first[n_bodies] != n_blobs) return fail(RMB_ERR_ARG, w + ": body_first must run from 0 to n_blobs");
  for (long k = 0; k < n_bodies; ++k) {
    const long count = body_first[k + 1] - body_first[k];
    if (count < 0) return fail(RMB_ERR_ARG, w + ": body_first must be non-decreasing");
    if (k < n_free && count > max_count) max_count = count;
  }
  if (n_free == 0) return 0;
  // (with the centre term a deck may hold bodies without blobs: the blob arrays are then not read)
  const bool blob_arrays = blob_ref_dev && ref_dev && r_dev;
  if ((!blob_arrays && !(law && n_blobs == 0)) || !loc_dev || !quat_dev || !draws_dev || !energy_dev || !accepted_dev)
    return fail(RMB_ERR_ARG, w + ": null pointer");
  const long lanes = law && n_bodies > n_blobs ? n_bodies : n_blobs;
  const long blocks = lanes > 0 ? (lanes + rmb::kMoveChunk - 1) / rmb::kMoveChunk : 1;
  if (blocks > 0x7fffffffL) return fail(RMB_ERR_ARG, w + ": too many blobs for one launch");
  RMB_HIP(hipSetDevice(c->device));
  A a{};
  fill_potential(a, periodic_length, eps, b, eps_wall, b_wall, weight, blob_radius);
  a.r = r_dev; a.n = n_blobs;
  a.blob_ref = blob_ref_dev; a.ref = ref_dev; a.loc = loc_dev; a.quat = quat_dev; a.draws = draws_dev; a.max_angle_shift = max_angle_shift;
  a.decide = 1; a.kT = kT;
  a.r_rw = r_dev; a.loc_rw = loc_dev; a.quat_rw = quat_dev; a.energy = energy_dev; a.accepted = accepted_dev;
  if (law) fill_body_law(a, periodic_length, BodyLaw{n_bodies, law->eps, law->b});
  if (int rc = reserve_scratch(c, blocks, max_count, law ? 3 : 2, a)) return rc;
  const bool periodic = a.p.Lx > 0 || a.p.Ly > 0 || a.p.Lz > 0;
  const MoveKernel delta = delta_kernel_of<true>(form, periodic, law != nullptr);
  const MoveKernel finish = law ? rmb::move_finish_kernel<true> : rmb::move_finish_kernel<false>;
  // the events of the "timing" option bracket the whole sweep
  int slot;
  if (int rc = timing_begin(c, &slot)) return rc;
  const auto moves = [&]() -> int {
    for (long k = 0; k < n_free; ++k) {
      a.body = k; a.first = body_first[k]; a.count = body_first[k + 1] - body_first[k];
      // (a body without blobs: every lane idles, the partials are zeros and the move is decided on dE = 0)
      hipLaunchKernelGGL(delta, dim3((unsigned)blocks), dim3(rmb::kMoveChunk), 0, c->stream, a);
      RMB_HIP(hipGetLastError());
      hipLaunchKernelGGL(finish, dim3(1), dim3(256), 0, c->stream, a);
      RMB_HIP(hipGetLastError());
    }
    return 0;
  };
  const int rc = moves();
  const int rc_end = timing_end(c, slot);      // the slot is closed whatever the launches returned
  return rc ? rc : rc_end;
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

int rmb_mcmc_body_delta_device(rmb_ctx* c, long n_blobs, const double* r_dev, long first, long count, const double* r_body_new_dev,
                               const double* periodic_length, double eps, double b, double eps_wall, double b_wall, double weight,
                               double blob_radius, int form, double* out_dev) {
  return rmbi::delta_impl("rmb_mcmc_body_delta_device", c, n_blobs, r_dev, first, count, r_body_new_dev, periodic_length, eps, b, eps_wall, b_wall,
                          weight, blob_radius, form, out_dev, nullptr, nullptr, 0, nullptr);
}

int rmb_mcmc_body_delta_bb_device(rmb_ctx* c, long n_blobs, const double* r_dev, long first, long count, const double* r_body_new_dev,
                                  long n_bodies, const double* loc_dev, long body, const double* loc_new_dev, const double* periodic_length,
                                  double eps, double b, double eps_wall, double b_wall, double weight, double blob_radius, int form,
                                  double body_eps, double body_b, double* out_dev) {
  const rmbi::BodyLaw law{n_bodies, body_eps, body_b};
  return rmbi::delta_impl("rmb_mcmc_body_delta_bb_device", c, n_blobs, r_dev, first, count, r_body_new_dev, periodic_length, eps, b, eps_wall,
                          b_wall, weight, blob_radius, form, out_dev, &law, loc_dev, body, loc_new_dev);
}

int rmb_mcmc_sweep_device(rmb_ctx* c, long n_bodies, long n_free, long n_blobs, const long* body_first, const int* blob_ref_dev,
                          const double* ref_dev, double* loc_dev, double* quat_dev, double* r_dev, const double* draws_dev,
                          double max_angle_shift, const double* periodic_length, double eps, double b, double eps_wall, double b_wall,
                          double weight, double blob_radius, int form, double kT, double* energy_dev, int* accepted_dev) {
  return rmbi::sweep_impl("rmb_mcmc_sweep_device", c, n_bodies, n_free, n_blobs, body_first, blob_ref_dev, ref_dev, loc_dev, quat_dev, r_dev,
                          draws_dev, max_angle_shift, periodic_length, eps, b, eps_wall, b_wall, weight, blob_radius, form, kT, energy_dev,
                          accepted_dev, nullptr);
}

int rmb_mcmc_sweep_bb_device(rmb_ctx* c, long n_bodies, long n_free, long n_blobs, const long* body_first, const int* blob_ref_dev,
                             const double* ref_dev, double* loc_dev, double* quat_dev, double* r_dev, const double* draws_dev,
                             double max_angle_shift, const double* periodic_length, double eps, double b, double eps_wall, double b_wall,
                             double weight, double blob_radius, int form, double body_eps, double body_b, double kT, double* energy_dev,
                             int* accepted_dev) {
  const rmbi::BodyLaw law{n_bodies, body_eps, body_b};
  return rmbi::sweep_impl("rmb_mcmc_sweep_bb_device", c, n_bodies, n_free, n_blobs, body_first, blob_ref_dev, ref_dev, loc_dev, quat_dev, r_dev,
                          draws_dev, max_angle_shift, periodic_length, eps, b, eps_wall, b_wall, weight, blob_radius, form, kT, energy_dev,
                          accepted_dev, &law);
}

}  // extern "C"
