"""The HIP pair laws against the extended-precision restatement of tests/_pair_forces_numpy.py, blob by blob -- shared by
tests/test_gpu_pair_forces.py and tools/pair_forces_report.py.

A family is a set of context options plus an entry point; `last_path` is asserted after every launch (1 = the symmetric
force sweep sym_force_kernel / its fp32 twin, 0 = the one-sided force_sweep_kernel: "deterministic" = 1, "symmetric" = 0, a
target sub-range or N < 128).  Every comparison also asserts that the blobs whose every neighbour lies beyond the culling
reach (2a + 750 b; 2a + 110 b for the fp32 kernel) get 0.0 in every component, bitwise.  The worst ratio per
(family, law, boundary), in units of C eps_prec S beyond the floor, goes into RESULTS."""
import numpy as np

import _pair_forces_numpy as pf
from _pair_forces_numpy import A, B, EPS, EXT

RESULTS = {}
_loners = {}


class Family(object):
  def __init__(self, name, law, options, path, cases, entry="host", precision=64, bound_precision=None, target_range=None, shards=None):
    self.name, self.law, self.options, self.path, self.entry = name, law, dict(options), path, entry
    self.case_list, self.precision, self.target_range, self.shards = list(cases), precision, target_range, shards
    self.bound_precision = bound_precision or precision

  def cases(self):
    return [(self.name, size, variant) for size, variant in self.case_list]


N, NS, NB = pf.N_CLOUD, pf.N_SUB, pf.N_BIG
SYM = {"deterministic": 0}
SMALL4 = [(N, "open"), (N, "offset"), (N, "box"), (N, "pow2")]
FAMILIES = [
    # --- contact law, fp64, symmetric sweep --------------------------------------------------------------------------------
    Family("contact_cull0", "contact", dict(SYM, force_cull=0), 1, SMALL4 + [(N, "box3")]),
    Family("contact_cull1", "contact", dict(SYM, force_cull=1), 1, SMALL4 + [(N, "box3")]),
    Family("contact_device_entry", "contact", dict(SYM), 1, [(N, "open"), (N, "box")], entry="device"),
    Family("contact_big_sort0", "contact", dict(SYM, force_cull=1, force_sort=0), 1, [(NB, "open"), (NB, "box")]),
    Family("contact_big_sort1", "contact", dict(SYM, force_cull=1, force_sort=1), 1, [(NB, "open"), (NB, "box")]),
    Family("contact_big_cull0", "contact", dict(SYM, force_cull=0), 1, [(NB, "open")]),
    Family("contact_shards3", "contact", dict(SYM), 1, [(N, "open"), (N, "box"), (NB, "open")], entry="shards", shards=3),
    # --- contact law, one-sided sweep ----------------------------------------------------------------------------------------
    Family("contact_deterministic1", "contact", {"deterministic": 1}, 0, [(N, "open"), (N, "box")]),
    Family("contact_symmetric0", "contact", {"symmetric": 0}, 0, [(N, "open"), (N, "pow2"), (N, "offset")]),
    Family("contact_target_range", "contact", {}, 0, [(N, "open"), (N, "box")], target_range=pf.TARGET_RANGE),
    Family("contact_n72", "contact", {}, 0, [(NS, "open"), (NS, "box")]),
    # --- per-blob radii ------------------------------------------------------------------------------------------------------
    Family("radii_sym", "radii", dict(SYM), 1, [(N, "open"), (N, "box"), (N, "pow2")]),
    Family("radii_sym_device_entry", "radii", dict(SYM), 1, [(N, "open"), (N, "box")], entry="device"),
    Family("radii_sweep", "radii", {"symmetric": 0}, 0, [(N, "open"), (N, "box")]),
    Family("radii_sweep_device_entry", "radii", {"symmetric": 0}, 0, [(N, "open"), (N, "box")], entry="device"),
    Family("radii_n72", "radii", {}, 0, [(NS, "open"), (NS, "box")]),
    # --- single precision: open boundaries; in a box the option falls back to the fp64 kernel and meets the fp64 bound ----------
    Family("f32_contact_cull0", "contact", dict(SYM, precision=32, force_cull=0), 1, [(N, "open"), (N, "offset")], precision=32),
    Family("f32_contact_cull1", "contact", dict(SYM, precision=32, force_cull=1), 1, [(N, "open"), (N, "offset"), (NB, "open")], precision=32),
    Family("f32_force_precision", "contact", dict(SYM, precision=64, force_precision=32), 1, [(N, "open")], precision=32),
    Family("f32_radii", "radii", dict(SYM, precision=32), 1, [(N, "open"), (N, "offset")], precision=32),
    Family("f32_radii_force_precision", "radii", dict(SYM, force_precision=32, force_cull=0), 1, [(N, "open")], precision=32),
    Family("f32_box_falls_back", "contact", dict(SYM, precision=32), 1, [(N, "box")], precision=32, bound_precision=64),
    Family("f32_radii_box_falls_back", "radii", dict(SYM, force_precision=32), 1, [(N, "box")], precision=32, bound_precision=64),
    # --- body-body Yukawa law: always fp64, always symmetric -----------------------------------------------------------------
    Family("yukawa_cull0", "yukawa", {"force_cull": 0}, 1, [(N, "open"), (N, "box3"), (N, "pow2")]),
    Family("yukawa_cull1", "yukawa", {"force_cull": 1}, 1, [(N, "open"), (N, "box3"), (N, "pow2"), (NS, "open")]),
    Family("yukawa_device_entry", "yukawa", {}, 1, [(N, "open"), (N, "box3")], entry="device"),
    Family("yukawa_big_sorted", "yukawa", {"force_cull": 1, "force_sort": 1}, 1, [(NB, "open"), (NB, "box")]),
]
BY_NAME = {f.name: f for f in FAMILIES}
assert len(BY_NAME) == len(FAMILIES)


def all_cases():
  return [c for f in FAMILIES for c in f.cases()]


def _boundary(L):
  return "open" if L is None else "box"


def open_context(Ctx, options, r, a, L, target_range=None):
  import torch
  ctx = Ctx(0)
  for key, val in options.items():
    ctx.set_option(key, val)
  ctx.set_positions(torch.as_tensor(np.ascontiguousarray(r).reshape(-1), device="cuda"), a, np.zeros(3) if L is None else L, wall=False)
  if target_range:
    ctx.set_target_range(*target_range)
  return ctx


def launch(ctx, fam, n, radii):
  """(n_targets, 3) numpy result of the family's entry point; `last_path` asserted."""
  import torch
  law, entry = fam.law, fam.entry
  if law == "yukawa":
    got = ctx.body_body_force(EPS, B) if entry == "host" else ctx.body_body_force_device(EPS, B).cpu().numpy()
  elif law == "radii":
    if entry == "host":
      got = ctx.blob_blob_force_radii(radii, EPS, B)
    else:
      got = ctx.blob_blob_force_radii_device(torch.as_tensor(radii, device="cuda"), EPS, B).cpu().numpy()
  elif entry == "shards":
    total = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    for g in range(fam.shards):
      total += ctx.blob_blob_force_pairshard_device(EPS, B, A, g, fam.shards)
      assert ctx.get_option("last_path") == fam.path
    got = total.cpu().numpy()
  else:
    got = ctx.blob_blob_force(EPS, B, A) if entry == "host" else ctx.blob_blob_force_device(EPS, B, A).cpu().numpy()
  path = ctx.get_option("last_path")
  assert path == fam.path, "%s: last_path %d, expected %d" % (fam.name, path, fam.path)
  return np.asarray(got).reshape(-1, 3)


def loners_of(law, size, variant, precision):
  key = (law, size, variant, precision)
  if key not in _loners:
    r, L = pf.cloud(size, variant)
    _loners[key] = pf.loners(law, r, L, radii=pf.radii_of(size) if law == "radii" else None, precision=precision)
    assert len(_loners[key]) >= 4
  return _loners[key]


def compare(label, law, size, variant, got, precision=64, rows=None):
  """Assert |got - EXT| <= MARGIN C eps S + floor per blob and component, and exact zeros on the loners; returns the worst
  ratio in units of C eps S."""
  r, L = pf.cloud(size, variant)
  F, S, floor = pf.reference(law, size, variant, precision)
  lo, hi = rows if rows is not None else (0, size)
  F, S, floor = F[lo:hi], S[lo:hi], floor[lo:hi]
  assert got.shape == F.shape, (got.shape, F.shape)
  assert np.all(np.isfinite(got)), "%s %s %d %s: non-finite force" % (label, law, size, variant)
  c = pf.C32[law] if precision == 32 else pf.C[law, L is not None]
  ratio, i, k = pf.worst(got, F, S, floor, c, precision)
  key = (label, law, _boundary(L))
  RESULTS[key] = max(RESULTS.get(key, 0.0), ratio)
  print("%-28s %-8s %4d %-6s worst %.3f C at blob %d component %d" % (label, law, size, variant, ratio, i + lo, k))
  assert ratio <= pf.MARGIN, (
      "family %s law %s cloud %d %s: blob %d component %d is off by %.3g C (bound %g C, C = %g units of %s S); got %.17g, extended "
      "precision %s, scale %s" % (label, law, size, variant, i + lo, k, ratio, pf.MARGIN, c, "2^-24" if precision == 32 else "2^-53",
                                  got[i, k], np.format_float_scientific(F[i, k], precision=20), np.format_float_scientific(S[i, k], precision=6)))
  lon = loners_of(law, size, variant, precision)
  lon = lon[(lon >= lo) & (lon < hi)] - lo
  bits = np.ascontiguousarray(got[lon]).view(np.uint64)
  assert not bits.any(), "family %s cloud %d %s: a blob beyond the reach of every neighbour got %r, not 0.0" % (label, size, variant, got[lon][bits.any(axis=1)])
  return ratio


def run_case(Ctx, name, size, variant):
  fam = BY_NAME[name]
  r, L = pf.cloud(size, variant)
  radii = pf.radii_of(size) if fam.law == "radii" else None
  ctx = open_context(Ctx, fam.options, r, A if fam.law == "contact" else 1.0, L, fam.target_range)
  try:
    got = launch(ctx, fam, size, radii)
  finally:
    ctx.close()
  # a fallen-back kernel (fp32 asked for in a box) is the fp64 kernel: its bound, its reach
  return compare(name, fam.law, size, variant, got, fam.bound_precision, fam.target_range)


# ---------------------------------------------------------------------------------------------------------------------
# energies
# ---------------------------------------------------------------------------------------------------------------------
def energy_key(form, L):
  return ("yukawa_energy" if form == "yukawa" else form, L is not None)


def device_energy(ctx, form, eps, b, a):
  """The pair energy of the resident points through the form's entry; the one-blob sum of the blob forms must be 0.0."""
  if form == "body":
    U = ctx.body_body_potential(eps, b)
  else:
    U_one, U = ctx.blob_potential(eps, b, a, repulsion_strength_wall=0.0, potential=form)
    assert pf.is_positive_zero(U_one)
  return U


def compare_energy(label, form, L, got, U, S, floor):
  c = pf.C[energy_key(form, L)]
  ratio = pf.energy_ratio(got, U, S, floor, c)
  key = (label, form, _boundary(L))
  RESULTS[key] = max(RESULTS.get(key, 0.0), ratio)
  assert np.isfinite(got)
  assert ratio <= pf.MARGIN, ("%s form %s %s: energy off by %.3g C (bound %g C); got %.17g, extended precision %s, weighted term sum %s"
                              % (label, form, _boundary(L), ratio, pf.MARGIN, got, np.format_float_scientific(U, precision=20),
                                 np.format_float_scientific(S, precision=6)))
  return ratio


def run_slab(Ctx, band, form):
  """Every option of the energy sweep on the clouds of one band: 136 blobs open and in a box with culling off and on; 2176
  blobs with "force_sort" 0 / 1, culling on / off, and "potential_resort" 1 and 4 with a second evaluation."""
  eps, b, a = pf.SLAB["eps"], pf.SLAB["b"][form], pf.SLAB["a"]
  zero = band[0] > 750
  for big, box, runs in ((False, False, [dict(force_cull=0), dict(force_cull=1)]),
                         (False, True, [dict(force_cull=0), dict(force_cull=1)]),
                         (True, False, [dict(force_cull=1, force_sort=0), dict(force_cull=0, force_sort=1),
                                        dict(force_cull=1, force_sort=1, potential_resort=1), dict(force_cull=1, force_sort=1, potential_resort=4)]),
                         (True, True, [dict(force_cull=1, force_sort=1)])):
    r, L = pf.slab_cloud(band, form, big, box)
    U, S, floor = pf.slab_reference(band, form, big, box)
    for options in runs:
      ctx = open_context(Ctx, options, r, a if form != "body" else 1.0, L)
      try:
        for again in range(2 if "potential_resort" in options else 1):
          got = device_energy(ctx, form, eps, b, a)
          label = "slab%s_%s" % ("_big" if big else "", "_".join("%s%d" % (k.split("_")[-1], v) for k, v in sorted(options.items())))
          if zero:
            assert pf.is_positive_zero(got), (label, form, band, got)
          compare_energy(label, form, L, got, U, S, floor)
      finally:
        ctx.close()


def run_ladder_energy(Ctx, form, box):
  for x in pf.ladder("yukawa" if form != "soft" else "contact"):
    r = pf.ladder_pair(x, 2 * A if form == "soft" else 0.0, B, box)
    L = None
    if box:
      L = pf.LADDER_BOX.copy()
      if form == "body":
        L[2] = 64.0
    U, S, floor, _ = pf.energy(form, r, L, EPS, B, A)
    ctx = open_context(Ctx, {}, r, A if form != "body" else 1.0, L)
    try:
      got = device_energy(ctx, form, EPS, B, A)
    finally:
      ctx.close()
    if x > 750:
      assert pf.is_positive_zero(got), (form, x, got)
    compare_energy("ladder_n2", form, L, got, U, S, floor)


WALL = dict(eps_w=2.3, b_w=0.05)


def run_wall_ladder(Ctx, form):
  """One blob at (z - a)/b_w over the ladder: the one-blob wall term alone (no weight, no pair), U_pair = 0.0.  Bound as for
  a pair term with the conditioning 1 + z/b_w of the exponent; C of the form's open pair energy."""
  worst = 0.0
  for x in pf.ladder("contact" if form == "soft" else "yukawa"):
    z = A + x * WALL["b_w"]
    r = np.array([[0.25, 0.5, z]])
    ctx = open_context(Ctx, {}, r, A, None)
    try:
      U_one, U_pair = ctx.blob_potential(EPS, B, A, repulsion_strength_wall=WALL["eps_w"], debye_length_wall=WALL["b_w"], weight=0.0, potential=form)
    finally:
      ctx.close()
    assert pf.is_positive_zero(U_pair)
    ref = pf.wall_term(z, WALL["eps_w"], WALL["b_w"], A, form)[0]
    S = abs(ref) * (EXT(1) + EXT(z) / EXT(WALL["b_w"]))
    m = EXT(1) if form == "soft" else EXT(A) / abs(EXT(z) - EXT(A))
    floor = pf.TINY[64] * (EXT(WALL["eps_w"]) * m + EXT(1))
    worst = max(worst, compare_energy("wall_ladder_n1", form, None, U_one, ref, S, floor))
  return worst


def run_body_delta(Ctx, band, form, box):
  """mcmc_body_delta_device on a slab pair: tile B moved by 1.5 b along x, inside its band; against the EXT difference of the
  touched terms (every non-zero term of the cloud is one) under the bound of the two sums."""
  import torch
  eps, b, a = pf.SLAB["eps"], pf.SLAB["b"][form], pf.SLAB["a"]
  r, L = pf.slab_cloud(band, form, False, box)
  new = r[64:128] + np.array([1.5 * b, 0.0, 0.0])
  r_new = r.copy()
  r_new[64:128] = new
  U0, S0, f0, _ = pf.energy(form, r, L, eps, b, a)
  U1, S1, f1, _ = pf.energy(form, r_new, L, eps, b, a)
  ctx = open_context(Ctx, {}, r, a, L)
  try:
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).cuda()      # noqa: E731
    out = ctx.mcmc_body_delta_device(t(r), 64, 64, t(new), np.zeros(3) if L is None else L, eps, b, a, potential=form).cpu().numpy()
  finally:
    ctx.close()
  assert pf.is_positive_zero(out[0])
  if band[0] > 750:
    assert pf.is_positive_zero(out[1])
  return compare_energy("body_delta", form, L, float(out[1]), U1 - U0, S0 + S1, f0 + f1)
