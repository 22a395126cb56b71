// rmb_laplace.hip -- Laplace layer operators of phoretic bodies (laplace_kernels.h): launchers, the two fused device
// sweeps of the concentration solve on a context, and the six reference-shaped host entry points on the default context.
#include "rmb_internal.h"

#include <cmath>

#include "laplace_kernels.h"

namespace rmbi {

namespace {

template <int OP, bool WALL, bool SELF>
int laplace_launch(rmb_ctx* c, const rmb::LapArgs& a) {
  constexpr int NOUT = rmb::LapShape<OP>::NOUT;
  return one_sided_launch<rmb::laplace_sweep_kernel<OP, WALL, SELF>, rmb::laplace_finalize_kernel<NOUT>, NOUT>(c, a);
}

template <int OP, bool SELF>
int laplace_wall(rmb_ctx* c, const rmb::LapArgs& a, int wall) {
  return wall ? laplace_launch<OP, true, SELF>(c, a) : laplace_launch<OP, false, SELF>(c, a);
}

// op: LAP_*; self: sources are the targets (tgt == src, ns == nt).  Fields that the op does not read may be nullptr.
int laplace_device(rmb_ctx* c, int op, bool self, long ns, const double* src, long nt, const double* tgt, const double* nrm,
                   const double* w, const double* p, const double* q, double sp, double sq, double alpha, const double* cfield,
                   int wall, double* out) {
  rmb::LapArgs a{};
  a.src = src; a.tgt = tgt; a.nrm = nrm; a.w = w; a.p = p; a.q = q; a.c = cfield; a.out = out;
  a.n_src = ns; a.tgt_end = nt; a.sp = sp; a.sq = sq; a.alpha = alpha; a.prefactor = 1.0 / (4.0 * M_PI);
  if (self) {
    switch (op) {
      case rmb::LAP_S: return laplace_wall<rmb::LAP_S, true>(c, a, wall);
      case rmb::LAP_D: return laplace_wall<rmb::LAP_D, true>(c, a, wall);
      case rmb::LAP_OPERATOR: return laplace_wall<rmb::LAP_OPERATOR, true>(c, a, wall);
      case rmb::LAP_GRAD_D: return laplace_wall<rmb::LAP_GRAD_D, true>(c, a, wall);
      case rmb::LAP_DIPOLE: return laplace_wall<rmb::LAP_DIPOLE, true>(c, a, wall);
      case rmb::LAP_GRADIENT: return laplace_wall<rmb::LAP_GRADIENT, true>(c, a, wall);
      default: break;
    }
  } else {
    switch (op) {
      case rmb::LAP_S: return laplace_wall<rmb::LAP_S, false>(c, a, wall);
      case rmb::LAP_D: return laplace_wall<rmb::LAP_D, false>(c, a, wall);
      default: break;
    }
  }
  return fail(RMB_ERR_ARG, "laplace: no such operator");
}

int check_common(rmb_ctx* c, long ns, long nt, int wall) {
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (ns < 0 || nt < 0) return fail(RMB_ERR_ARG, "negative size");
  if (wall != 0 && wall != 1) return fail(RMB_ERR_ARG, "wall must be 0 or 1");
  return 0;
}

// host arrays -> staging buffers st[slot] of the default context
int stage(rmb_ctx* c, int slot, const double* host, size_t bytes, const double** dev) {
  if (int rc = c->st[slot].reserve(bytes ? bytes : sizeof(double))) return rc;
  if (bytes && host) RMB_HIP(hipMemcpyAsync(c->st[slot].p, host, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = (const double*)c->st[slot].p;
  return 0;
}

// One reference-shaped operator through the default context: stage, sweep, copy back, synchronise.
// nrm == nullptr for S / P; tgt == nullptr for the self operators.
int laplace_host(int op, long ns, const double* src, long nt, const double* tgt, const double* field, const double* weights,
                 const double* nrm, int wall, double* out) {
  std::lock_guard<std::mutex> lk(g_default_mu);
  rmb_ctx* c;
  if (int rc = default_ctx(&c)) return rc;
  if (int rc = check_common(c, ns, nt, wall)) return rc;
  const bool self = tgt == nullptr;
  const bool needs_nrm = op == rmb::LAP_D || op == rmb::LAP_GRAD_D;
  const int nout = (op == rmb::LAP_GRAD_D || op == rmb::LAP_DIPOLE) ? 3 : 1;
  if (nt == 0) return 0;
  if (!out || (ns > 0 && (!src || !field || !weights || (needs_nrm && !nrm)))) return fail(RMB_ERR_ARG, "null pointer");
  RMB_HIP(hipSetDevice(c->device));
  const size_t b1 = (size_t)ns * sizeof(double), b3 = 3 * b1;
  const double *src_d, *tgt_d, *f_d, *w_d, *n_d = nullptr;
  if (int rc = stage(c, 2, src, b3, &src_d)) return rc;
  tgt_d = src_d;
  if (!self)
    if (int rc = stage(c, 4, tgt, (size_t)3 * nt * sizeof(double), &tgt_d)) return rc;
  if (int rc = stage(c, 3, field, b1, &f_d)) return rc;
  if (int rc = stage(c, 5, weights, b1, &w_d)) return rc;
  if (needs_nrm)
    if (int rc = stage(c, 6, nrm, b3, &n_d)) return rc;
  const size_t bo = (size_t)nout * nt * sizeof(double);
  if (int rc = c->st[7].reserve(bo)) return rc;
  double* out_d = (double*)c->st[7].p;
  if (ns == 0) {
    RMB_HIP(hipMemsetAsync(out_d, 0, bo, c->stream));
  } else {
    const bool on_p = op == rmb::LAP_D || op == rmb::LAP_GRAD_D;
    if (int rc = laplace_device(c, op, self, ns, src_d, nt, tgt_d, n_d, w_d, on_p ? f_d : nullptr, on_p ? nullptr : f_d, 1.0, 1.0,
                                0.0, nullptr, wall, out_d))
      return rc;
  }
  RMB_HIP(hipMemcpyAsync(out, out_d, bo, hipMemcpyDeviceToHost, c->stream));
  RMB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace

}  // namespace rmbi

using namespace rmbi;

extern "C" {

int rmb_laplace_operator_device(rmb_ctx* c, long n, const double* r_dev, const double* normals_dev, const double* weights_dev,
                                const double* p_dev, const double* q_dev, double alpha, int wall, double* out_dev) {
  if (int rc = check_common(c, n, n, wall)) return rc;
  if (n == 0) return 0;
  if (!p_dev && !q_dev) return fail(RMB_ERR_ARG, "laplace operator: p and q are both null");
  if (!out_dev || !r_dev || !weights_dev || (p_dev && !normals_dev)) return fail(RMB_ERR_ARG, "null pointer");
  RMB_HIP(hipSetDevice(c->device));
  const int op = p_dev && q_dev ? rmb::LAP_OPERATOR : (p_dev ? rmb::LAP_D : rmb::LAP_S);
  return laplace_device(c, op, true, n, r_dev, n, r_dev, normals_dev, weights_dev, p_dev, q_dev, -1.0, 1.0, alpha,
                        p_dev && alpha != 0.0 ? p_dev : nullptr, wall, out_dev);
}

int rmb_laplace_gradient_device(rmb_ctx* c, long n, const double* r_dev, const double* normals_dev, const double* weights_dev,
                                const double* p_dev, const double* q_dev, int wall, double* out_dev) {
  if (int rc = check_common(c, n, n, wall)) return rc;
  if (n == 0) return 0;
  if (!p_dev && !q_dev) return fail(RMB_ERR_ARG, "laplace gradient: p and q are both null");
  if (!out_dev || !r_dev || !weights_dev || (p_dev && !normals_dev)) return fail(RMB_ERR_ARG, "null pointer");
  RMB_HIP(hipSetDevice(c->device));
  const int op = p_dev && q_dev ? rmb::LAP_GRADIENT : (p_dev ? rmb::LAP_GRAD_D : rmb::LAP_DIPOLE);
  return laplace_device(c, op, true, n, r_dev, n, r_dev, normals_dev, weights_dev, p_dev, q_dev, 2.0, -2.0, 0.0, nullptr, wall,
                        out_dev);
}

int rmb_laplace_single_layer(long n, const double* r, const double* field, const double* weights, int wall, double* out) {
  return laplace_host(rmb::LAP_S, n, r, n, nullptr, field, weights, nullptr, wall, out);
}

int rmb_laplace_double_layer(long n, const double* r, const double* field, const double* weights, const double* normals,
                             int wall, double* out) {
  return laplace_host(rmb::LAP_D, n, r, n, nullptr, field, weights, normals, wall, out);
}

int rmb_laplace_deriv_double_layer(long n, const double* r, const double* field, const double* weights, const double* normals,
                                   int wall, double* out) {
  return laplace_host(rmb::LAP_GRAD_D, n, r, n, nullptr, field, weights, normals, wall, out);
}

int rmb_laplace_dipole(long n, const double* r, const double* field, const double* weights, int wall, double* out) {
  return laplace_host(rmb::LAP_DIPOLE, n, r, n, nullptr, field, weights, nullptr, wall, out);
}

int rmb_laplace_single_layer_source_target(long ns, const double* src, long nt, const double* tgt, const double* field,
                                           const double* weights, int wall, double* out) {
  if (nt > 0 && !tgt) return fail(RMB_ERR_ARG, "null pointer");
  return laplace_host(rmb::LAP_S, ns, src, nt, tgt, field, weights, nullptr, wall, out);
}

int rmb_laplace_double_layer_source_target(long ns, const double* src, long nt, const double* tgt, const double* field,
                                           const double* weights, const double* normals, int wall, double* out) {
  if (nt > 0 && !tgt) return fail(RMB_ERR_ARG, "null pointer");
  return laplace_host(rmb::LAP_D, ns, src, nt, tgt, field, weights, normals, wall, out);
}

}  // extern "C"
