"""The extended-precision restatement of the pair laws (tests/_pair_forces_numpy.py) on the CPU: the designed clouds hold
every class, the yardsticks C / C32 that tests/test_gpu_pair_forces.py holds the HIP kernels to are measured here from the
reference side alone, and mutants of an fp64 restatement of the laws show what the per-blob bound sees and the norm
tests of the suite do not: a culling reach ten times too short, one dropped far pair, 2 a_i for a_i + a_j, no image in z.

Units: one rounding unit of a force component is 2^-53 S_ik (2^-24 S_ik in single precision) with the per-blob scale of
_pair_forces_numpy (every pair weighted by its conditioning 1 + rho/b), beyond a floor of one result-denormal per pair."""
import numpy as np
import pytest

import _body_forces_numpy as bfn
import _pair_forces_numpy as pf
import _potential_numpy as pn
from _pair_forces_numpy import A, B, EPS, EXT

KW = dict(repulsion_strength=EPS, debye_length=B, blob_radius=A)
SMALL = [(pf.N_CLOUD, v) for v in pf.VARIANTS] + [(pf.N_SUB, "open"), (pf.N_SUB, "box")]
BIG = [(pf.N_BIG, "open"), (pf.N_BIG, "box")]
MEASURED = {}


@pytest.fixture(autouse=True)
def _ieee_and_one_oracle_thread():
  """Gradual underflow in this thread (see _pair_forces_numpy.ieee_denormals) and the oracle on this thread alone: its
  OpenMP workers keep the environment of the thread that created them."""
  from oracle import oracle
  threads = oracle.num_threads()
  oracle.set_num_threads(1)
  try:
    with pf.ieee_denormals():
      yield
  finally:
    oracle.set_num_threads(threads)


def test_long_double_is_the_extended_format():
  assert pf.LONG_DOUBLE and EXT is np.longdouble and np.finfo(np.longdouble).nmant >= 63
  assert pf.MARGIN == 4.0


@pytest.mark.parametrize("size,variant", SMALL + BIG, ids=str)
def test_designed_cloud_holds_every_class(size, variant):
  r, L = pf.cloud(size, variant)          # asserts the coverage
  assert r.shape == (size, 3)
  c = pf.coverage("contact", r, L)
  absent = pf.VARIANTS[variant][4]
  assert all(c[k] >= 1 for k in pf.CLASSES if k not in absent), c
  assert c["tail"] - c["loner"] >= 8 and c["loner"] >= 4 and c["coincident"] == 0 and c["oblique"] == 0, c
  assert (L is None) == (variant in ("open", "offset"))
  if size == pf.N_CLOUD:
    assert size % 64 == 8 and size // 64 == 3          # three full 64-blob tiles and one of eight
  if size == pf.N_BIG:
    assert size // 64 == 33 and size % 64               # 33 full tiles and a partial one: "force_sort" applies from 32 on
  if size == pf.N_SUB:
    assert size < 128
  if size == pf.N_BIG:
    return
  # the radii law and the Yukawa law (x = r/b) on the same positions
  cr = pf.coverage("radii", r, L, radii=pf.radii_of(size))
  assert all(cr[k] >= 1 for k in ("x<=0", "0<x<1", "1..30", "30..110", "110..700", "700..745", ">750")) and cr["loner"] >= 4 and cr["oblique"] == 0, cr
  cy = pf.coverage("yukawa", r, L)
  assert all(cy[k] >= 1 for k in ("1..30", "30..110", "110..700", "700..745", ">750")) and cy["loner"] >= 4 and cy["oblique"] == 0, cy
  assert len(pf.loners("contact", r, L, precision=32)) > len(pf.loners("contact", r, L)) >= 4


@pytest.mark.parametrize("form", pf.ENERGY_FORMS)
@pytest.mark.parametrize("band", pf.BANDS, ids=str)
def test_slab_clouds_hold_one_band(band, form):
  for big in (False, True):
    for box in (False, True):
      r, L = pf.slab_cloud(band, form, big, box)
      assert len(r) == (pf.N_SLAB_BIG if big else pf.N_SLAB) and np.all(r[:, 2] > 0)
      facing = pf.slab_coverage(band, form, big, box)          # asserts the design
      assert len(facing) == (0 if band[0] > 750 else 16 * (17 if big else 1))
      if not big:
        U, S, floor = pf.slab_reference(band, form, False, box)
        b = pf.SLAB["b"][form]
        terms = np.array([float(np.exp(-EXT(x)) / ((EXT(x) * EXT(b)) if form != "soft" else 1)) for _, _, x in facing])
        if len(terms):
          assert terms.min() >= np.exp(-21.0) * terms.max()          # the sum is sensitive to each term
          assert U > 0
        else:
          assert U < floor and U < EXT(2.0) ** -1070        # the band that must give exactly 0 on the device


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against what pins it
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_existing_numpy_references():
  r, L = pf.cloud(pf.N_CLOUD, "box3")
  F = pf.forces("yukawa", r, L)
  Fb = bfn.forces(r, L, EPS, B)
  assert np.abs(F - Fb).max() <= 2.0 ** -60 * np.abs(Fb).max()
  for form in ("soft", "yukawa"):
    for box in (False, True):
      rs, Ls = pf.slab_cloud(pf.BANDS[0], form, False, box)
      U = pf.energy(form, rs, Ls, pf.SLAB["eps"], pf.SLAB["b"][form], pf.SLAB["a"])[0]
      _, Up, _ = pn.energy(rs, periodic_length=Ls, repulsion_strength=pf.SLAB["eps"], debye_length=pf.SLAB["b"][form],
                           blob_radius=pf.SLAB["a"], potential=form)
      assert abs(U - Up) <= 2.0 ** -58 * abs(Up), (form, box)
  rs, Ls = pf.slab_cloud(pf.BANDS[1], "body", False, True)
  U = pf.energy("body", rs, Ls, pf.SLAB["eps"], pf.SLAB["b"]["body"])[0]
  Ub = bfn.energy(rs, Ls, pf.SLAB["eps"], pf.SLAB["b"]["body"])
  assert abs(U - Ub) <= 2.0 ** -58 * abs(Ub)


# ---------------------------------------------------------------------------------------------------------------------
# yardsticks
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_forces(oracle, law, r, L, radii):
  Lz = np.zeros(3) if L is None else L
  if law == "contact":
    return oracle.calc_blob_blob_forces_oracle(r, periodic_length=Lz, **KW)
  if law == "radii":
    return oracle.calc_blob_blob_forces_radii_oracle(r, radii, periodic_length=Lz, repulsion_strength=EPS, debye_length=B)
  return pf.yukawa_float64(r, L)


def _measure_force(oracle, law):
  out = {False: 0.0, True: 0.0}
  for size, variant in SMALL + (BIG if law != "radii" else []):      # the radii law runs on the small clouds only
    r, L = pf.cloud(size, variant)
    radii = pf.radii_of(size) if law == "radii" else None
    F, S, floor = pf.reference(law, size, variant)
    got = _oracle_forces(oracle, law, r, L, radii)
    q, i, k = pf.worst(got, F, S, floor, 1.0)
    assert pf.rel_err(got, F) < 1e-12
    out[L is not None] = max(out[L is not None], q)
  return out


def _measure_force32(law):
  worst = 0.0
  for size, variant in [(pf.N_CLOUD, "open"), (pf.N_CLOUD, "offset"), (pf.N_SUB, "open")] + ([(pf.N_BIG, "open")] if law == "contact" else []):
    r, L = pf.cloud(size, variant)
    radii = pf.radii_of(size) if law == "radii" else None
    F, S, floor = pf.reference(law, size, variant, precision=32)
    got = pf.forces(law, r, L, radii=radii, dtype=np.float32)
    worst = max(worst, pf.worst(got, F, S, floor, 1.0, 32)[0])
  return worst


def _measure_energy(form):
  out = {False: 0.0, True: 0.0}
  for band in pf.BANDS:
    for big in (False, True):
      for box in (False, True):
        r, L = pf.slab_cloud(band, form, big, box)
        U, S, floor = pf.slab_reference(band, form, big, box)
        got = pf.energy(form, r, L, pf.SLAB["eps"], pf.SLAB["b"][form], pf.SLAB["a"], dtype=np.float64)[0]
        if S > 0:
          out[box] = max(out[box], pf.energy_ratio(got, U, S, floor, 1.0))
        else:
          assert pf.is_positive_zero(got)
  return out


def _check(name, key, measured):
  stored = pf.C[key] if name == "C" else pf.C32[key]
  MEASURED[name, key] = measured
  print("%s[%r]: measured %.3f, stored %.1f" % (name, key, measured, stored))
  assert measured <= stored <= 2.0 * measured + 1.0, (name, key, measured, stored)


@pytest.mark.parametrize("law", pf.FORCE_LAWS)
def test_yardstick_force(oracle, law):
  """C[law, periodic]: the fp64 oracle's own worst ratio (contact, radii: oracle/oracle_mobility.c; yukawa:
  _body_forces_numpy.forces in float64).  Stored = measured rounded up, never tuned to a kernel."""
  m = _measure_force(oracle, law)
  for periodic in (False, True):
    _check("C", (law, periodic), m[periodic])


@pytest.mark.parametrize("law", ("contact", "radii"))
def test_yardstick_force_single_precision(law):
  _check("C32", law, _measure_force32(law))


@pytest.mark.parametrize("form", pf.ENERGY_FORMS)
def test_yardstick_energy(form):
  m = _measure_energy(form)
  for periodic in (False, True):
    _check("C", ("yukawa_energy" if form == "yukawa" else form, periodic), m[periodic])


# ---------------------------------------------------------------------------------------------------------------------
# mutants: what the per-blob bound sees
# ---------------------------------------------------------------------------------------------------------------------
def _mutant_excess(law, size, variant, mutant):
  r, L = pf.cloud(size, variant)
  radii = pf.radii_of(size) if law == "radii" else None
  F, S, floor = pf.reference(law, size, variant)
  got = pf.forces(law, r, L, radii=radii, dtype=np.float64, mutant=mutant)
  clean = pf.forces(law, r, L, radii=radii, dtype=np.float64)
  c = pf.C[law, L is not None]
  assert pf.worst(clean, F, S, floor, c)[0] <= pf.MARGIN          # the same restatement without the mutation passes
  return pf.worst(got, F, S, floor, c)[0] / pf.MARGIN, pf.rel_err(got, F)


@pytest.mark.parametrize("size,variant", [(pf.N_CLOUD, "open"), (pf.N_CLOUD, "box"), (pf.N_BIG, "open")], ids=str)
@pytest.mark.parametrize("reach", [75.0, 110.0])
def test_mutant_short_reach_passes_the_norm_and_fails_per_blob(size, variant, reach):
  excess, norm = _mutant_excess("contact", size, variant, {"reach": reach})
  print("reach %g b on %d %s: %.3g times the per-blob bound, rel_err %.2e" % (reach, size, variant, excess, norm))
  assert norm < 1e-12          # the documented gap: every norm test of the suite passes this law
  assert excess >= 10.0


def test_mutant_one_far_pair_of_a_tail_blob_dropped():
  r, L = pf.cloud(pf.N_CLOUD, "open")
  X, _, _ = pf.pair_x("contact", r, L)
  tails = np.nonzero((X.min(axis=1) > 30) & (X.min(axis=1) < 110))[0]
  i = int(tails[0])
  j = int(np.argmin(X[i]))          # its nearest neighbour: beyond x = 30
  assert X[i, j] > 30
  excess, norm = _mutant_excess("contact", pf.N_CLOUD, "open", {"drop": (i, j)})
  assert norm < 1e-12 and excess >= 10.0, (excess, norm)


@pytest.mark.parametrize("variant", ["open", "box"])
def test_mutant_contact_at_twice_the_own_radius(variant):
  excess, _ = _mutant_excess("radii", pf.N_CLOUD, variant, {"two_a_i": 1})
  assert excess >= 10.0
  # ... also for a blob that has far neighbours only
  r, L = pf.cloud(pf.N_CLOUD, variant)
  radii = pf.radii_of(pf.N_CLOUD)
  F, S, floor = pf.reference("radii", pf.N_CLOUD, variant)
  got = pf.forces("radii", r, L, radii=radii, dtype=np.float64, mutant={"two_a_i": 1})
  X, _, _ = pf.pair_x("radii", r, L, radii=radii)
  far = np.nonzero((X.min(axis=1) > 30) & (X.min(axis=1) < 600))[0]
  q = pf.ratios(got, F, S, floor, pf.C["radii", L is not None])
  assert len(far) >= 8 and q[far].max(axis=1).min() >= 10.0 * pf.MARGIN


@pytest.mark.parametrize("variant", ["pow2", "box3"])
def test_mutant_no_image_in_z(variant):
  for law in ("contact", "yukawa"):
    excess, _ = _mutant_excess(law, pf.N_CLOUD, variant, {"no_z_image": 1})
    assert excess >= 10.0, (law, excess)


@pytest.mark.parametrize("form", pf.ENERGY_FORMS)
@pytest.mark.parametrize("box", [False, True])
def test_energy_mutants(form, box):
  """Reach 110 b zeroes the bands 400..420 and 700..740; one facing pair dropped from any band that has terms."""
  key = ("yukawa_energy" if form == "yukawa" else form, box)
  kw = dict(eps=pf.SLAB["eps"], b=pf.SLAB["b"][form], a=pf.SLAB["a"], dtype=np.float64)
  for band in pf.BANDS[:4]:
    r, L = pf.slab_cloud(band, form, False, box)
    U, S, floor = pf.slab_reference(band, form, False, box)
    assert pf.energy_ratio(pf.energy(form, r, L, **kw)[0], U, S, floor, pf.C[key]) <= pf.MARGIN
    facing = pf.slab_coverage(band, form, False, box)
    for i, j, _ in (facing[0], facing[-1]):
      got = pf.energy(form, r, L, mutant={"drop": (i, j)}, **kw)[0]
      assert pf.energy_ratio(got, U, S, floor, pf.C[key]) >= 10.0 * pf.MARGIN, (band, i, j)
    if band[0] >= 400:
      got = pf.energy(form, r, L, mutant={"reach": 110.0}, **kw)[0]
      assert pf.is_positive_zero(got) and pf.energy_ratio(got, U, S, floor, pf.C[key]) >= 10.0 * pf.MARGIN, band
