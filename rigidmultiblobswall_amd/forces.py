"""Blob-blob pair forces -- the `calc_blob_blob_forces_<impl>` surface on MI355X.

Replaces multi_bodies/forces_pycuda.py:148-180 (float32 CUDA) and its CPU twins
(multi_bodies/forces_numba.py:58-71) behind the same call:
  calc_blob_blob_forces_hip(r_vectors, periodic_length=L, repulsion_strength=eps,
                            debye_length=b, blob_radius=a) -> ndarray (N,3)
selected in the reference by `blob_blob_force_implementation`
(multi_bodies/multi_bodies_functions.py:249-278).  fp64 here; minimal image only.

Body-body forces (`body_body_force_torque_implementation python`, multi_bodies_functions.py:359-408) behind the
reference's call as well:
  calc_body_body_forces_torques_hip(bodies, r_vectors, periodic_length=L, repulsion_strength=eps,
                                    debye_length=b) -> ndarray (2 N_b, 3), rows [f_0, t_0, f_1, t_1, ...]
"""
import numpy as np

from .context import MobilityContext

_ctx = None
_mctx = None


def _context(n=0):
  """Own contexts (the forces use raw positions, the products clamped ones: sharing would re-pack on every call), on
  the devices mobility.py is configured with (mobility.set_devices / RMB_DEVICES / RMB_DEVICE)."""
  global _ctx, _mctx
  from . import mobility
  devs = mobility.devices()
  if len(devs) > 1 and n >= mobility.multi_min_blobs:
    if _mctx is None or _mctx.devices != devs:
      if _mctx is not None:
        _mctx.close()
      from .multi import MultiContext
      _mctx = MultiContext(devs)
    return _mctx
  if _ctx is None or _ctx.device != devs[0]:
    if _ctx is not None:
      _ctx.close()
    _ctx = MobilityContext(devs[0])
  return _ctx


def reset():
  """Drop the module-level contexts (frees device memory)."""
  global _ctx, _mctx
  for c in (_ctx, _mctx):
    if c is not None:
      c.close()
  _ctx = _mctx = None


def calc_blob_blob_forces_hip(r_vectors, *args, **kwargs):
  L = kwargs.get('periodic_length')
  eps = kwargs.get('repulsion_strength')
  b = kwargs.get('debye_length')
  a = kwargs.get('blob_radius')
  if L is None:
    L = np.zeros(3)
  ctx = _context(np.asarray(r_vectors).size // 3)
  # wall=False: raw positions, no height clamp (the reference passes r_vectors untouched)
  ctx.set_positions(r_vectors, a, L, wall=False)
  return ctx.blob_blob_force(eps, b, a)


def calc_blob_blob_forces_tree_hip(r_vectors, *args, **kwargs):
  """`tree_numba` twin (multi_bodies/forces_numba.py:142-271): the reference builds a k-d tree and keeps the pairs within
  2 a + 30 b.  The force kernel here skips whole tile pairs whose bounding boxes are further apart than the exponential
  reaches in double precision (after a device Morton sort of the blobs), which changes no bit of the full sum -- so this
  is `calc_blob_blob_forces_hip`, and it differs from the reference's truncated sum by e^-30 of a contact force per
  dropped pair (4e-14 relative on the goldens)."""
  return calc_blob_blob_forces_hip(r_vectors, *args, **kwargs)


def calc_blob_blob_forces_radii_hip(r_vectors, radius_blobs, *args, **kwargs):
  """`radii_numba` twin (multi_bodies/forces_numba.py:125-137): every blob has its own radius and two blobs touch at
  r = a_i + a_j.  Same keyword arguments as above (`blob_radius` is ignored, as in the reference kernel)."""
  L = kwargs.get('periodic_length')
  if L is None:
    L = np.zeros(3)
  ctx = _context(0)      # per-blob radii: one device
  ctx.set_positions(r_vectors, 1.0, L, wall=False)
  return ctx.blob_blob_force_radii(radius_blobs, kwargs.get('repulsion_strength'), kwargs.get('debye_length'))


def calc_blob_blob_forces_table_hip(r_vectors, *args, **kwargs):
  """Blob-blob forces of a user-defined radial law: pair_table= a PairTable (pair_table.py), periodic_length= as above.
  One symmetric fp64 sweep on one device; repulsion_strength, debye_length and blob_radius are not read (the table is the
  whole law).  Per-blob radii, single precision and the multi-device engine do not serve a table."""
  from .pair_table import PairTable
  table = kwargs.get('pair_table')
  if not isinstance(table, PairTable):
    raise ValueError("calc_blob_blob_forces_table_hip needs pair_table= a PairTable, got %r" % (type(table).__name__,))
  if kwargs.get('radius_blobs') is not None:
    raise ValueError("a pair table is one law for every pair: per-blob radii are not served")
  L = kwargs.get('periodic_length')
  if L is None:
    L = np.zeros(3)
  ctx = _context(0)      # a table lives in one single-device context
  ctx.set_positions(r_vectors, 1.0, L, wall=False)
  ctx._use_pair_table(table)
  return ctx.pair_table_force()


def calc_body_body_forces_torques_hip(bodies, r_vectors, *args, **kwargs):
  """`calc_body_body_forces_torques_python` (multi_bodies_functions.py:387-408) on the device: a Yukawa repulsion between
  the bodies' `location`s, one symmetric fp64 sweep over the N_b centres instead of the Python double loop.  Returns
  (2 N_b, 3): force rows from the kernel, torque rows zero (the reference's law has no torque).  r_vectors is not read,
  as in the reference."""
  L = kwargs.get('periodic_length')
  if L is None:
    L = np.zeros(3)
  nb = len(bodies)
  out = np.zeros((2 * nb, 3))
  if nb == 0:
    return out
  centres = np.array([np.asarray(b.location, dtype=np.float64).reshape(3) for b in bodies])
  ctx = _context(0)      # the sweep over body centres runs on one device
  ctx.set_positions(centres, 1.0, L, wall=False)
  out[0::2] = ctx.body_body_force(kwargs.get('repulsion_strength'), kwargs.get('debye_length'))
  return out
