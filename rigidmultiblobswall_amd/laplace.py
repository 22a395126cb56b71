"""Phoretic (chemically active) bodies: Laplace layer operators and the concentration-driven active slip.

A `structure` line may name a third file ending in `.Laplace` (multi_bodies/multi_bodies.py:1175-1217): per node the
body-frame normal, reaction rate k, emitting rate e, surface mobility mu and quadrature weight w.  Before every rigid
solve the reference's `calc_slip` (multi_bodies.py:77-177) solves a boundary-integral Laplace problem for the
concentration c on the body surfaces and turns its surface gradient into active slip.  This module holds

  * the six operators of Laplace_kernels/Laplace_kernels_numba.py under their names with a `_hip` suffix (numpy in /
    out, `wall=` keyword as there), served by csrc/laplace_kernels.h;
  * `PhoreticSlip`, the device-resident `calc_slip` hook of rigid_integrator.RigidIntegrator: each call solves
        0.5 c - D[c] + S[k c / Dc] = c_bg + S[e / Dc]
    by GMRES(200) without preconditioner from a zero guess (one fused sweep per iteration,
    MobilityContext.laplace_operator_device), then forms
        g = 4 r H + 2 b + 2 G[c] - 2 P[(e - k c) / Dc]      (one fused sweep, laplace_gradient_device)
        slip = mu (g - n (n.g))   (+ the lab-frame .slip slip, when the structure has one).
Images of the wall only for `domain single_wall`, as the reference (in_plane gets none); no periodic images.
"""
import numpy as np
import torch

from . import _lib

LAPLACE_COLUMNS = 7    # n_x n_y n_z  reaction_rate  emitting_rate  surface_mobility  weight


# ---------------------------------------------------------------------------------------------
# the reference's six operators (Laplace_kernels_numba.py), numpy in / out
# ---------------------------------------------------------------------------------------------
def _flat(x, what, n=None):
  x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
  if n is not None and x.size != n:
    raise ValueError("%s must have %d entries, got %d" % (what, n, x.size))
  return x


def _p(x):
  import ctypes
  return ctypes.c_void_p(x.ctypes.data)


def Laplace_single_layer_operator_hip(r_vectors, field, weights, wall=0):
  '''S[f]_i = 1/(4 pi) sum_{j != i} w_j f_j / |r_ij| (+ image 1/|r_i - rbar_j| for every j with wall = 1); (N,) out.'''
  r = _flat(r_vectors, "r_vectors")
  n = r.size // 3
  f, w = _flat(field, "field", n), _flat(weights, "weights", n)
  out = np.empty(n)
  _lib.check(_lib.load().rmb_laplace_single_layer(n, _p(r), _p(f), _p(w), 1 if wall else 0, _p(out)))
  return out


def Laplace_double_layer_operator_hip(r_vectors, field, weights, normals, wall=0):
  '''D[f]_i = 1/(4 pi) sum_{j != i} w_j f_j (r_ij . n_j) / |r_ij|^3 (+ image term); (N,) out.'''
  r = _flat(r_vectors, "r_vectors")
  n = r.size // 3
  f, w, nv = _flat(field, "field", n), _flat(weights, "weights", n), _flat(normals, "normals", 3 * n)
  out = np.empty(n)
  _lib.check(_lib.load().rmb_laplace_double_layer(n, _p(r), _p(f), _p(w), _p(nv), 1 if wall else 0, _p(out)))
  return out


def Laplace_deriv_double_layer_operator_hip(r_vectors, field, weights, normals, wall=0):
  '''Gradient of the double layer, 1/(4 pi) sum_{j != i} w_j f_j (I - 3 r r^T / r^2) n_j / r^3 (+ image term);
  flat (3N,) out as the reference.'''
  r = _flat(r_vectors, "r_vectors")
  n = r.size // 3
  f, w, nv = _flat(field, "field", n), _flat(weights, "weights", n), _flat(normals, "normals", 3 * n)
  out = np.empty(3 * n)
  _lib.check(_lib.load().rmb_laplace_deriv_double_layer(n, _p(r), _p(f), _p(w), _p(nv), 1 if wall else 0, _p(out)))
  return out


def Laplace_dipole_operator_hip(r_vectors, field, weights, wall=0):
  '''1/(4 pi) sum_{j != i} w_j f_j r_ij / |r_ij|^3 (+ image term); flat (3N,) out.'''
  r = _flat(r_vectors, "r_vectors")
  n = r.size // 3
  f, w = _flat(field, "field", n), _flat(weights, "weights", n)
  out = np.empty(3 * n)
  _lib.check(_lib.load().rmb_laplace_dipole(n, _p(r), _p(f), _p(w), 1 if wall else 0, _p(out)))
  return out


def Laplace_single_layer_operator_source_target_hip(source, target, field, weights_source, wall=0):
  '''S from the sources to the targets; pairs closer than 1e-12 skip the free-space term (never the image).'''
  src, tgt = _flat(source, "source"), _flat(target, "target")
  ns, nt = src.size // 3, tgt.size // 3
  f, w = _flat(field, "field", ns), _flat(weights_source, "weights_source", ns)
  out = np.empty(nt)
  _lib.check(_lib.load().rmb_laplace_single_layer_source_target(ns, _p(src), nt, _p(tgt), _p(f), _p(w), 1 if wall else 0, _p(out)))
  return out


def Laplace_double_layer_operator_source_target_hip(source, target, field, weights_source, normals_source, wall=0):
  '''D from the sources to the targets; pairs closer than 1e-12 skip the free-space term (never the image).'''
  src, tgt = _flat(source, "source"), _flat(target, "target")
  ns, nt = src.size // 3, tgt.size // 3
  f, w = _flat(field, "field", ns), _flat(weights_source, "weights_source", ns)
  nv = _flat(normals_source, "normals_source", 3 * ns)
  out = np.empty(nt)
  _lib.check(_lib.load().rmb_laplace_double_layer_source_target(ns, _p(src), nt, _p(tgt), _p(f), _p(w), _p(nv), 1 if wall else 0,
                                                                  _p(out)))
  return out


# ---------------------------------------------------------------------------------------------
# deck data
# ---------------------------------------------------------------------------------------------
def read_laplace_file(path, n_vertex):
  """(n_vertex, 7) array of a .Laplace file (np.loadtxt, as multi_bodies.py:1185): one row per vertex."""
  data = np.loadtxt(path, dtype=np.float64, ndmin=2)
  if data.shape[1] != LAPLACE_COLUMNS:
    raise ValueError("%s: expected %d columns (normal, reaction rate, emitting rate, surface mobility, weight), got %d"
                     % (path, LAPLACE_COLUMNS, data.shape[1]))
  if data.shape[0] != n_vertex:
    raise ValueError("%s has %d rows but its vertex file has %d blobs" % (path, data.shape[0], n_vertex))
  return data


def background_vector(values):
  """`background_Laplace` zero-padded to 9 values (read_input/read_input.py:100-101)."""
  v = np.zeros(0) if values is None else np.asarray(values, dtype=np.float64).reshape(-1)
  if v.size > 9:
    raise ValueError("background_Laplace takes at most 9 values (c0, gradient 3, Hessian xx xy xz yy yz), got %d" % v.size)
  return np.concatenate([v, np.zeros(9 - v.size)])


def background_hessian(background):
  """Symmetric, traceless H from background_Laplace[4:9] = (H_xx, H_xy, H_xz, H_yy, H_yz) (multi_bodies.py:125-129)."""
  b = background_vector(background)
  H = np.zeros((3, 3))
  H[0, 0:3] = b[4:7]
  H[1, 1:3] = b[7:9]
  H[2, 2] = -H[0, 0] - H[1, 1]
  return H + H.T - np.diag(H.diagonal())


def _sweep_context(susp):
  """The plain MobilityContext the Laplace sweeps run through: the suspension's own, the helper context of a multi-device
  engine or a replicated facade (the sweeps are one-sided and deterministic: every rank computes the same bits), else
  a new one on the suspension's device.  -> (context, owned)"""
  from .context import MobilityContext
  if type(susp.ctx) is MobilityContext:
    return susp.ctx, False
  h = getattr(susp.ctx, "helper_context", None)
  if type(h) is MobilityContext:
    return h, False
  return MobilityContext(susp.device.index or 0), True


class PhoreticSlip(object):
  """`calc_slip` hook of a RigidIntegrator whose bodies carry .Laplace data (see the module docstring).

  laplace: (Nblobs, 7) body-frame rows in blob order; background: background_Laplace (up to 9 values);
  slip_body_frame: optional (Nblobs, 3) tensor of prescribed body-frame slip (.slip files), added in the lab frame.
  Counters: `last_iterations` (GMRES iterations of the last solve), `iterations` (running total), `solves`.  The
  integrator's det_iterations_count is not touched (the reference's Laplace counter is local to calc_slip)."""

  restart = 200
  maxiter = 1000

  def __init__(self, susp, laplace, background=None, diffusion_coefficient=1.0, tolerance=1e-8, wall=None,
               slip_body_frame=None):
    dev = susp.device
    L = np.asarray(laplace, dtype=np.float64).reshape(-1, LAPLACE_COLUMNS)
    if L.shape[0] != susp.n_blobs:
      raise ValueError("Laplace data for %d nodes, the suspension has %d blobs" % (L.shape[0], susp.n_blobs))
    Dc = float(diffusion_coefficient)
    k, e = L[:, 3] / Dc, L[:, 4] / Dc
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    self.normals_body = t(L[:, 0:3])
    self.k = t(k) if np.any(k != 0) else None        # a zero field is not swept
    self.e = t(e) if np.any(e != 0) else None
    self.mu = t(L[:, 5]).view(-1, 1)
    self.weights = t(L[:, 6])
    bg = background_vector(background)
    self.c0, self.grad0 = float(bg[0]), t(bg[1:4])
    self.H = t(background_hessian(bg))
    if getattr(susp, "boundary", None) == "free_surface":
      raise ValueError("phoretic slip above a free surface: the Laplace layer operators have wall and unbounded images only")
    self.wall = bool(susp.wall if wall is None else wall)
    self.tolerance = float(tolerance)
    self.slip_body_frame = slip_body_frame
    self.print_residual = False
    self.last_iterations = 0
    self.iterations = 0
    self.solves = 0
    self.last_residual = 0.0
    self.concentration = None         # (Nblobs,) tensor of the last solve
    self._ctx, self._own_ctx = _sweep_context(susp)
    self._key = None
    self._slip = None

  def close(self):
    if self._own_ctx and self._ctx is not None:
      self._ctx.close()
    self._ctx = None

  def __call__(self, integ):
    return self.compute(integ.susp, print_residual=getattr(integ, "print_residual", False))

  def compute(self, susp, print_residual=False):
    """(Nblobs, 3) lab-frame slip at the suspension's bound configuration.  The result is reused while that configuration
    stays bound (set_configuration installs a new location tensor): the paired solves of one configuration solve the
    Laplace problem once."""
    if self._slip is not None and self._key is susp.location:
      return self._slip
    from .krylov import gmres_right_preconditioned
    from .rigid_integrator import lab_frame_slip
    ctx = self._ctx
    r = susp.r_dev.view(-1, 3)
    rf = r.reshape(-1)
    n = lab_frame_slip(susp, self.normals_body).view(-1, 3)
    nf = n.reshape(-1)
    w = self.weights
    # right-hand side: c_bg + S[e / Dc]
    Hr = r @ self.H
    rhs = self.c0 + r @ self.grad0 + (r * Hr).sum(dim=1)
    if self.e is not None:
      rhs = rhs + ctx.laplace_operator_device(rf, w, q=self.e, wall=self.wall)

    def A(x):
      return ctx.laplace_operator_device(rf, w, p=x, q=None if self.k is None else self.k * x, normals=nf, alpha=0.5,
                                         wall=self.wall)
    ortho = ctx.krylov_orthogonalize_device if self.restart < 256 and r.device.type == "cuda" else None
    c, info = gmres_right_preconditioned(A, lambda x: x, rhs.contiguous(), tol=self.tolerance, restart=self.restart,
                                         maxiter=self.maxiter, ortho=ortho)
    self.last_iterations = int(info["iterations"])
    self.last_residual = float(info["residual"])
    self.iterations += self.last_iterations
    self.solves += 1
    if print_residual:
      print("Laplace gmres: iterations = %d, residual = %.3e" % (self.last_iterations, self.last_residual), flush=True)
    c = c.contiguous()
    # gradient: 4 r H + 2 b + 2 G[c] - 2 P[(e - k c) / Dc]
    if self.k is None:
      q = self.e
    elif self.e is None:
      q = -(self.k * c)
    else:
      q = self.e - self.k * c
    g = ctx.laplace_gradient_device(rf, w, p=c, q=q, normals=nf, wall=self.wall).view(-1, 3)
    g = g + 4.0 * Hr + 2.0 * self.grad0
    slip = self.mu * (g - n * (n * g).sum(dim=1, keepdim=True))
    if self.slip_body_frame is not None:
      slip = slip + lab_frame_slip(susp, self.slip_body_frame).view(-1, 3)
    self.concentration = c
    self._key, self._slip = susp.location, slip
    return slip
