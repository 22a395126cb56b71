"""Potential energy of a blob configuration -- the `many_body_potential_pycuda` surface on MI355X.

Replaces many_bodyMCMC/many_body_potential_pycuda.py:234-351 (one CUDA thread per blob, allocation and both copies on
every call) behind the same calls and keyword names:
  blobs_potential_hip(r_vectors, periodic_length=L, debye_length_wall=.., repulsion_strength_wall=.., debye_length=..,
                      repulsion_strength=.., weight=.., blob_radius=..) -> float
  bodies_potential_hip(bodies, **kwargs) -> 0.0          (the reference's default body potentials are empty); with
                      body_potential=(eps, b) the Yukawa energy between the body locations (the law of forces.py's
                      body-body forces), HIP
  compute_total_energy_hip(bodies, r_vectors, **kwargs)  -> U_blobs + U_bodies
and, beyond the reference, the energy difference of ONE moved body in O(n_body N) (the single-body moves of mcmc.py):
  body_energy_difference_hip(r_vectors, first, body_new, **kwargs) -> (dU_one_blob, dU_pair)
`pair_table=T` (a PairTable, pair_table.py) replaces the blob-blob pair term by a user-defined radial law in
blobs_potential_hip / compute_total_energy_hip (bodies_potential_hip passes it by: a table is a blob-blob law, there are no
body-body tables); body_energy_difference_hip refuses it (single-body moves do not serve a table).
`potential="soft"|"yukawa"` is the other extra keyword: the module's own form, or the Yukawa form of the reference's only
MCMC example (examples/boomerang_suspension/potential_pycuda_user_defined.py).  A reference checkout binds it with
  import rigidmultiblobswall_amd.potential as p; many_body_potential_pycuda.compute_total_energy = p.compute_total_energy_hip
"""
import numpy as np

from .context import MobilityContext, POTENTIAL_FORMS

_ctx = None


def _context():
  """Own context (raw positions, as forces.py) on the first device mobility.py is configured with."""
  global _ctx
  from . import mobility
  dev = mobility.devices()[0]
  if _ctx is None or _ctx.device != dev:
    if _ctx is not None:
      _ctx.close()
    _ctx = MobilityContext(dev)
  return _ctx


def reset():
  """Drop the module-level context (frees device memory)."""
  global _ctx
  if _ctx is not None:
    _ctx.close()
  _ctx = None


def potential_terms(ctx, **kwargs):
  """(U_one_blob, U_pair) of ctx's resident positions from the reference's keyword arguments."""
  return ctx.blob_potential(kwargs.get('repulsion_strength'), kwargs.get('debye_length'), kwargs.get('blob_radius'),
                            repulsion_strength_wall=kwargs.get('repulsion_strength_wall') or 0.0,
                            debye_length_wall=kwargs.get('debye_length_wall') or 1.0, weight=kwargs.get('weight') or 0.0,
                            potential=kwargs.get('potential', 'soft'), pair_table=kwargs.get('pair_table'))


def blobs_potential_hip(r_vectors, *args, **kwargs):
  L = kwargs.get('periodic_length')
  if L is None:
    L = np.zeros(3)
  if kwargs.get('potential', 'soft') not in POTENTIAL_FORMS:
    raise ValueError("potential must be 'soft' or 'yukawa'")
  ctx = _context()
  # wall=False: raw heights, the reference passes r_vectors untouched
  ctx.set_positions(r_vectors, kwargs.get('blob_radius'), L, wall=False)
  u_one, u_pair = potential_terms(ctx, **kwargs)
  return u_one + u_pair


def body_energy_difference_hip(r_vectors, first, body_new, *args, **kwargs):
  """(U_one(r') - U_one(r), U_pair(r') - U_pair(r)) for r' = r_vectors with the rows first ... first + len(body_new) - 1
  replaced by body_new: the touched terms only, each subtracted before it is accumulated (rmb_mcmc_body_delta_device).
  r_vectors / body_new: numpy arrays or CUDA float64 tensors; same keyword arguments as blobs_potential_hip."""
  import torch
  if kwargs.get('pair_table') is not None:
    raise ValueError("the single-body energy difference does not serve a pair table (pair_table=): use the whole-configuration energy")
  if kwargs.get('potential', 'soft') not in POTENTIAL_FORMS:
    raise ValueError("potential must be 'soft' or 'yukawa'")
  ctx = _context()
  dev = torch.device("cuda", ctx.device)
  t = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64))).to(dev).reshape(-1, 3).contiguous()  # noqa: E731
  r, new = t(r_vectors), t(body_new)
  with torch.cuda.device(dev):
    out = ctx.mcmc_body_delta_device(r, int(first), new.shape[0], new, kwargs.get('periodic_length'), kwargs.get('repulsion_strength'),
                                     kwargs.get('debye_length'), kwargs.get('blob_radius'),
                                     repulsion_strength_wall=kwargs.get('repulsion_strength_wall') or 0.0,
                                     debye_length_wall=kwargs.get('debye_length_wall') or 1.0, weight=kwargs.get('weight') or 0.0,
                                     potential=kwargs.get('potential', 'soft'))
    d = out.cpu().numpy()
  return float(d[0]), float(d[1])


def bodies_potential_hip(bodies, *args, **kwargs):
  """one_body_potential / body_body_potential of the reference are empty (many_body_potential_pycuda.py:125-155): 0.0.
  body_potential=(eps, b): U_body = sum_{i<j} eps exp(-r_ij/b) / r_ij between the locations of `bodies` (objects with a
  .location, or an (n, 3) array), minimal image in every direction of periodic_length= with a positive period
  (rmb_body_body_potential) -- the energy of the steppers' body-body forces."""
  law = kwargs.get('body_potential')
  if law is None:
    return 0.0
  eps, b = MobilityContext._body_law(law)
  if hasattr(bodies, "__len__") and len(bodies) and hasattr(bodies[0], "location"):
    loc = np.array([np.asarray(body.location, dtype=np.float64) for body in bodies]).reshape(-1, 3)
  else:
    loc = np.asarray(bodies, dtype=np.float64).reshape(-1, 3)
  L = kwargs.get('periodic_length')
  ctx = _context()
  ctx.set_positions(loc, kwargs.get('blob_radius') or 1.0, np.zeros(3) if L is None else L, wall=False)
  return ctx.body_body_potential(eps, b)


def compute_total_energy_hip(bodies, r_vectors, *args, **kwargs):
  return blobs_potential_hip(r_vectors, *args, **kwargs) + bodies_potential_hip(bodies, *args, **kwargs)
