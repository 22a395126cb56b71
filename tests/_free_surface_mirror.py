"""The rotational products above a free (stress-free) surface at z = 0 from the UNBOUNDED oracle -- TEST infrastructure.

The image of blob j sits at S r_j, S = diag(1, 1, -1).  A force is a polar vector, its image is S f; a torque is an
axial one, its image is -S tau.  So a free-surface product of N blobs is the unbounded product of the doubled system
[r; S r] with sources [v; +-S v], read at the first N targets: every block of the 6N mobility comes from the
reference-pinned `no_wall_*_oracle` functions, periodic_length passed through (images in x and y only)."""
import numpy as np
import torch

from _oracle_ctx import OracleContext

S = np.array([1.0, 1.0, -1.0])
_FN = {"tt": "no_wall_mobility_trans_times_force_oracle", "tr": "no_wall_mobility_trans_times_torque_oracle",
       "rt": "no_wall_mobility_rot_times_force_oracle", "rr": "no_wall_mobility_rot_times_torque_oracle"}


def cloud(n, a, seed):
  """The cloud of tests/test_gpu_free_surface.py::_cloud: blobs below z = a (the image's overlapping branch), blobs 0 and
  1 touching."""
  rng = np.random.RandomState(seed)
  side = 2.2 * a * n ** (1.0 / 3.0)
  r = np.column_stack([side * rng.rand(n), side * rng.rand(n), 0.05 * a + side * rng.rand(n)])
  r[0, 2] = 0.4 * a
  r[1] = r[0] + [2 * a, 0, 0]
  assert np.sum(r[:, 2] < a) >= 2
  return r


def periodic_box(n, a):
  """L = (1.5 s, 1.3 s, 0) for the cloud of side s."""
  side = 2.2 * a * n ** (1.0 / 3.0)
  return np.array([1.5 * side, 1.3 * side, 0.0])


def product(oracle, kind, r, v, eta, a, L=None):
  """Block `kind` (tt, tr, rt, rr) of the free-surface mobility applied to v: (3N,)."""
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
  n = len(r)
  sign = 1.0 if kind in ("tt", "rt") else -1.0          # the source: a force (polar) or a torque (axial)
  r2 = np.concatenate([r, r * S])
  v2 = np.concatenate([v, sign * v * S])
  kw = {} if L is None else {"periodic_length": np.asarray(L, dtype=np.float64)}
  return getattr(oracle, _FN[kind])(r2, v2.reshape(-1), eta, a, **kw)[:3 * n]


def fused_row(oracle, r, f, t, eta, a, L=None):
  return product(oracle, "tt", r, f, eta, a, L) + product(oracle, "tr", r, t, eta, a, L)


def grand(oracle, r, f, t, eta, a, L=None):
  """(u, w) = [[M_tt, M_tr], [M_rt, M_rr]] [f; t]"""
  return fused_row(oracle, r, f, t, eta, a, L), product(oracle, "rt", r, f, eta, a, L) + product(oracle, "rr", r, t, eta, a, L)


def dense_block(oracle, kind, r, eta, a, L=None):
  n3 = 3 * len(np.asarray(r).reshape(-1, 3))
  M = np.empty((n3, n3))
  e = np.zeros(n3)
  for k in range(n3):
    e[k] = 1.0
    M[:, k] = product(oracle, kind, r, e, eta, a, L)
    e[k] = 0.0
  return M


def dense_grand(oracle, r, eta, a, L=None):
  """The 6N x 6N matrix [[tt, tr], [rt, rr]]."""
  b = {k: dense_block(oracle, k, r, eta, a, L) for k in ("tt", "tr", "rt", "rr")}
  return np.block([[b["tt"], b["tr"]], [b["rt"], b["rr"]]])


class MirrorContext(OracleContext):
  """CPU stand-in: the OracleContext that serves the mirror products once set_option("free_surface_rotation", 1) and
  set_positions(wall="free_surface") are set, and refuses them like the library otherwise."""
  supports_free_surface = True
  supports_free_surface_rotation = True

  def set_positions(self, r, a, L=None, wall=True):
    self.free_surface = isinstance(wall, str)
    if self.free_surface and wall != "free_surface":
      raise ValueError("wall must be True, False or \"free_surface\"")
    OracleContext.set_positions(self, r, a, L, wall=False if self.free_surface else wall)

  def matvec_device(self, kind, vec, eta, vec2=None, in_plane=False, out=None):
    if not getattr(self, "free_surface", False):
      return OracleContext.matvec_device(self, kind, vec, eta, vec2=vec2, in_plane=in_plane, out=out)
    if in_plane or (kind != "tt" and not self.get_option("free_surface_rotation")):
      raise RuntimeError("free-surface context: not served above a free surface")
    v = vec.detach().cpu().numpy()
    if kind == "tt_tr":
      u = fused_row(self.o, self.r, v, vec2.detach().cpu().numpy(), eta, self.a, self.L)
    else:
      u = product(self.o, kind, self.r, v, eta, self.a, self.L)
    return torch.from_numpy(u)

  def matvec2_device(self, *args, **kwargs):
    if getattr(self, "free_surface", False):
      raise RuntimeError("free-surface context: no two-vector pass above a free surface")
    return OracleContext.matvec2_device(self, *args, **kwargs)
