"""What a reference input deck asks for, mapped onto what this engine runs -- or a ValueError.

The reference picks its backends by strings (multi_bodies/multi_bodies.py:207-287 `set_mobility_blobs`,
`set_mobility_vector_prod`; multi_bodies_functions.py:249-278 `set_blob_blob_forces`, :348-356
`set_body_body_forces_torques`).  The backend name itself (python / C++ / numba / pycuda / hip) does not change the
physics and is ignored; the SUFFIX does (`_no_wall`, `_free_surface`, `radii_*`), and so do per-blob radii in a
4-column .vertex file.  A deck that asks for a mode the time steppers here do not run must fail loudly: silently
running it with a wall, a uniform radius or without the body-body forces would be different physics.

`body_body_force_torque_implementation`: `None`, or `python` / `hip` -- the same Yukawa repulsion between body locations
(multi_bodies_functions.py:359-408), run as one symmetric HIP sweep over the centres.  It needs a context that has the
sweep (a single-GPU MobilityContext): the caller says so through validate(..., body_body_forces=True); on any other
context the deck is refused.  Rigid decks follow the reference's driver (force_torque_calculator_sort_by_bodies adds the
term, :443).  The reference's roller integrator builds its forces from calc_one_blob_forces + calc_blob_blob_forces alone
(quaternion_integrator_rollers.py:930-933) and never evaluates the option; a roller deck here adds the law the option
names to every force evaluation, which is that integrator with the law in its pair-force hook.

`blob_blob_force_implementation table_hip` with `blob_blob_pair_table FILE` is this engine's own spelling: the blob-blob
law is the radial table in FILE (pair_table.py; rows `r U dU/dr`, path relative to the deck) instead of the contact
exponential.  Refused when the file is missing and, like the body-body forces, on a context without the sweep
(validate(..., pair_tables=...)).
"""
import numpy as np

_BACKENDS = ("python", "C++", "numba", "pycuda", "hip", "cpp")


def _split(impl):
  """-> (backend, suffix) for strings like 'pycuda_no_wall', 'numba', 'C++_free_surface'."""
  for b in sorted(_BACKENDS, key=len, reverse=True):
    if impl == b:
      return b, ""
    if impl.startswith(b + "_"):
      return b, impl[len(b) + 1:]
  return None, impl


def hydrodynamic_mode(impl, option, free_surface=False):
  """'single_wall' | 'no_wall' (| 'free_surface' where the caller runs it: free_surface=True) from a mobility
  implementation string; ValueError for anything else."""
  if "radii" in impl:
    raise ValueError("%s %r: per-blob radii are served by the source-target products (dispatch.set_mobility_vector_prod), "
                     "not by the time steppers, which assume one blob radius" % (option, impl))
  backend, suffix = _split(impl)
  if backend is None:
    raise ValueError("%s %r: unknown implementation string" % (option, impl))
  if suffix == "":
    return "single_wall"
  if suffix == "no_wall":
    return "no_wall"
  if suffix == "free_surface" and free_surface:
    return "free_surface"
  if suffix == "free_surface":
    raise ValueError("%s %r: the time steppers do not run above a free surface (the product itself exists: "
                     "free_surface_mobility_trans_times_force_hip)" % (option, impl))
  raise ValueError("%s %r: unknown implementation suffix %r" % (option, impl, suffix))


def validate(read, uses_dense_blocks=True, body_body_forces=False, pair_tables=None):
  """Checks every implementation option of a ReadInput deck against `domain`; returns the hydrodynamic mode
  ('single_wall', 'no_wall' or 'in_plane' as given by `domain`, or 'free_surface': a rigid deck whose product is a
  `<backend>_free_surface` one under `domain single_wall`, multi_bodies.py:262-265).

  Above a free surface the dense blocks (uses_dense_blocks: the rigid schemes) may be `<backend>_no_wall` -- what a
  reference deck can run: its `C++_free_surface` names a function mobility.py does not define -- or
  `<backend>_free_surface`, this engine's own blocks (free_surface_blocks below).  The roller schemes do not run a
  reference deck there: the reference has no rotational products above a free surface.

  `domain free_surface` is this engine's own spelling, for roller decks (uses_dense_blocks = False) only: the rotational
  blocks of the mirror-image system (context option "free_surface_rotation", beyond the reference).  It requires a
  `<backend>_free_surface` product and returns 'free_surface'; rigid decks keep the reference's spelling.

  body_body_forces: the caller's context serves the body-body force sweep (hasattr(ctx, "body_body_force_device"));
  without it a deck with `body_body_force_torque_implementation` other than `None` is refused.
  pair_tables: the same for `blob_blob_force_implementation table_hip` (hasattr(ctx, "pair_table_force_device"); None: as
  body_body_forces -- both sweeps live on a single-GPU MobilityContext)."""
  if pair_tables is None:
    pair_tables = body_body_forces
  domain = read.domain
  if domain == "free_surface":
    if uses_dense_blocks:
      raise ValueError("domain free_surface: a rigid deck above a free surface keeps the reference's spelling, `domain "
                       "single_wall` with mobility_vector_prod_implementation <backend>_free_surface; `domain free_surface` "
                       "is for roller decks")
    impl = read.mobility_vector_prod_implementation
    if "radii" in impl or _split(impl)[0] is None or _split(impl)[1] != "free_surface":
      raise ValueError("mobility_vector_prod_implementation %r: `domain free_surface` needs a <backend>_free_surface "
                       "product" % (impl,))
    _check_forces(read, body_body_forces, pair_tables)
    return "free_surface"
  if domain not in ("single_wall", "no_wall", "in_plane"):
    raise ValueError("domain %r: expected single_wall, no_wall or in_plane" % (domain,))
  # (a roller deck, uses_dense_blocks = False, raises here for a free-surface product)
  modes = [("mobility_vector_prod_implementation", hydrodynamic_mode(read.mobility_vector_prod_implementation,
                                                                      "mobility_vector_prod_implementation", uses_dense_blocks))]
  if uses_dense_blocks:
    modes.append(("mobility_blobs_implementation", hydrodynamic_mode(read.mobility_blobs_implementation,
                                                                     "mobility_blobs_implementation", True)))
    product, blocks = modes[0][1], modes[1][1]
    if product != "free_surface" and blocks == "free_surface":
      raise ValueError("mobility_blobs_implementation %r builds free surface blocks but mobility_vector_prod_implementation %r "
                       "is a %s product: state the intended boundary"
                       % (read.mobility_blobs_implementation, read.mobility_vector_prod_implementation, product))
    if product == "free_surface":
      if blocks == "single_wall":
        raise ValueError("mobility_blobs_implementation %r builds wall blocks but mobility_vector_prod_implementation %r is a "
                         "free surface product: use a <backend>_no_wall (the reference's choice) or <backend>_free_surface one"
                         % (read.mobility_blobs_implementation, read.mobility_vector_prod_implementation))
      if "dense_algebra" in read.scheme and blocks != "free_surface":
        raise ValueError("scheme %s above a free surface takes the whole blob mobility from mobility_blobs_implementation: %r "
                         "would run it unbounded; use a <backend>_free_surface one" % (read.scheme, read.mobility_blobs_implementation))
      if domain != "single_wall":
        raise ValueError("mobility_vector_prod_implementation %r (free surface) needs `domain single_wall` (the reference's "
                         "position check), the deck says `domain %s`" % (read.mobility_vector_prod_implementation, domain))
      modes = []
      domain = "free_surface"
  want = "no_wall" if domain == "no_wall" else "single_wall"
  for option, mode in modes:
    if mode != want:
      raise ValueError("%s %r is a %s implementation but the deck says `domain %s`: the reference would mix an unbounded "
                       "mobility with wall checks (or the reverse); state the intended one"
                       % (option, getattr(read, option), mode, domain))
  _check_forces(read, body_body_forces, pair_tables)
  return domain


def pair_table_path(read):
  """The file of a `blob_blob_force_implementation table_hip` deck (`blob_blob_pair_table FILE`, relative to the deck), or a
  ValueError: keyword missing, file missing, or the keyword without the implementation string."""
  import os
  ff, name = read.blob_blob_force_implementation, getattr(read, "blob_blob_pair_table", None)
  if ff != "table_hip":
    if name is not None:
      raise ValueError("blob_blob_pair_table %r is read by `blob_blob_force_implementation table_hip` only; the deck says %r" % (name, ff))
    return None
  if name is None:
    raise ValueError("blob_blob_force_implementation table_hip needs `blob_blob_pair_table FILE` (text, rows `r U dU/dr` on a uniform grid)")
  path = read.resolve(name)
  if not os.path.isfile(path):
    raise ValueError("blob_blob_pair_table %r: no such file (looked for %s)" % (name, path))
  return path


def pair_table(read):
  """The PairTable of a `table_hip` deck, or None."""
  path = pair_table_path(read)
  if path is None:
    return None
  from .pair_table import PairTable
  return PairTable.load(path)


def _check_forces(read, body_body_forces=False, pair_tables=False):
  """The force options of a deck the time steppers can honour, or a ValueError."""
  ff = read.blob_blob_force_implementation
  if pair_table_path(read) is not None:       # table_hip: a user-defined radial law (pair_table.py)
    if not pair_tables:
      raise ValueError("blob_blob_force_implementation table_hip: a pair table runs on a single-GPU MobilityContext; this "
                       "context does not serve the sweep (no pair shards, no multi-device engine)")
    ff = "hip"
  if "radii" in ff:
    raise ValueError("blob_blob_force_implementation %r needs per-blob radii; the time steppers assume one blob radius "
                     "(dispatch.set_blob_blob_forces serves the product)" % (ff,))
  if ff != "None" and _split(ff)[0] is None and ff != "tree_numba":
    raise ValueError("blob_blob_force_implementation %r: unknown implementation string" % (ff,))
  bb = read.body_body_force_torque_implementation
  if bb not in ("None", "python", "hip"):
    raise ValueError("body_body_force_torque_implementation %r: unknown implementation string (None, python or hip)" % (bb,))
  if bb != "None" and not body_body_forces:
    raise ValueError("body_body_force_torque_implementation %r: body-body forces (multi_bodies_functions.py:359-408, a Yukawa "
                     "potential between body centres) run on a single-GPU MobilityContext; this context does not serve the "
                     "sweep" % (bb,))


def free_surface_blocks(read):
  """'no_wall' | 'free_surface': the dense blocks of a rigid deck that validate() found to run above a free surface."""
  return hydrodynamic_mode(read.mobility_blobs_implementation, "mobility_blobs_implementation", True)


def uniform_vertices(coor, blob_radius, path):
  """(n,3) coordinates of a .vertex array; a 4th column (per-blob radius) must equal the deck's blob_radius."""
  coor = np.asarray(coor, dtype=np.float64)
  if coor.shape[1] > 3:
    rad = coor[:, 3]
    if not np.allclose(rad, blob_radius, rtol=1e-12, atol=0.0):
      raise ValueError("%s lists per-blob radii (%.6g .. %.6g) that differ from blob_radius %.6g: blobs of different "
                       "radii (the reference's radii_* modes) are not run by the time steppers"
                       % (path, rad.min(), rad.max(), blob_radius))
  return coor[:, :3]


def phoretic(read):
  """True when a `structure` line of the deck names a .Laplace file (phoretic bodies, multi_bodies.py:1175-1217).
  ValueError for what the phoretic slip here does not run: structures without a .Laplace file next to ones with it
  (the reference's calc_slip fails on them: `b.normals` is missing), periodic images (the Laplace operators have none)
  and the roller schemes."""
  flags = [any(f.endswith(".Laplace") for f in s[2:]) for s in read.structures]
  if not any(flags):
    return False
  if not all(flags):
    missing = [s[0] for s, f in zip(read.structures, flags) if not f]
    raise ValueError("phoretic deck: every structure needs a .Laplace file (the reference's calc_slip reads normals and "
                     "rates of every body); missing for %s" % ", ".join(missing))
  L = np.asarray(read.periodic_length, dtype=np.float64).reshape(-1)
  if np.any(L != 0):
    raise ValueError("phoretic deck with periodic_length %s: the Laplace layer operators have no periodic images"
                     % " ".join("%g" % x for x in L))
  if "rollers" in read.scheme:
    raise ValueError("phoretic deck with scheme %s: the roller schemes do not run the phoretic slip" % read.scheme)
  return True
