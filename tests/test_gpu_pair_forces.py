"""The pair laws -- blob-blob contact force (uniform and per-blob radii, fp64 and fp32, symmetric and one-sided sweep, pair
shards), body-body Yukawa force, blob and body pair energies -- blob by blob against the extended-precision restatement of
tests/_pair_forces_numpy.py:

    |got - EXT| <= MARGIN * C[law, periodic] * eps_prec * S + floor          (MARGIN = 4)

with the per-blob scale S (every pair weighted by its conditioning 1 + rho/b), the floor of one result-denormal per pair and
the yardstick C of that module (the fp64 oracle's own worst ratio, measured on the CPU by tests/test_pair_forces_host.py;
`precision` = 32 in units of 2^-24 S against C32).  The norm tests of the suite see the pairs within ~27 b of contact; these
see the tail: exp_nonpositive below -30, its gradual underflow and the clamp at -750, the culling reach 2a + 750 b (110 b
for the float kernel) and its exact zeros, the tile gap under periodic images, the Morton permutation for blobs that only
have far neighbours, a_i + a_j for far pairs, the minimal image in z.  The families and the kernel each one pins
(`last_path`, asserted after every launch) are listed in tests/_pair_forces_gpu.py; tools/pair_forces_report.py runs this
file and writes the worst ratio per (family, law, boundary)."""
import numpy as np
import pytest

import _pair_forces_gpu as pg
import _pair_forces_numpy as pf
from _pair_forces_numpy import A, B, EPS, EXT

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _ieee():
  with pf.ieee_denormals():          # host-side float64 work on denormal results must not depend on the tests before
    yield


@pytest.fixture(scope="module")
def Ctx():
  from rigidmultiblobswall_amd import MobilityContext
  return MobilityContext


def test_the_reference_is_extended_precision_and_the_clouds_hold_every_class():
  assert pf.LONG_DOUBLE, "np.longdouble has no 64-bit mantissa here: fp64 would be compared with fp64"
  for size, variant in sorted(set((s, v) for _, s, v in pg.all_cases())):
    pf.cloud(size, variant)          # asserts the coverage


@pytest.mark.parametrize("family,size,variant", pg.all_cases(), ids=lambda v: str(v))
def test_forces_per_blob(Ctx, family, size, variant):
  pg.run_case(Ctx, family, size, variant)


def _ladder_bound(law, got, r, L, radii=None, a=A):
  F, S, floor = pf.forces(law, r, L, EPS, B, a, radii, scale=True)
  ratio, i, k = pf.worst(got, F, S, floor, pf.C[law, L is not None])
  key = ("host_wrapper_n2", law, "open" if L is None else "box")
  pg.RESULTS[key] = max(pg.RESULTS.get(key, 0.0), ratio)
  assert ratio <= pf.MARGIN, (law, r.tolist(), ratio, got.tolist(), F.astype(np.float64).tolist())


@pytest.mark.parametrize("box", [False, True], ids=["open", "box"])
def test_host_wrappers_two_blobs_over_the_ladder(box):
  """forces.calc_*_hip at N = 2 (the C ABI and the one-sided sweep; the body law its symmetric sweep) at
  x = -1, 0 exactly, 0.5, 30.5, 109, 111, 700, 744, 751: exact 0.0 at 751."""
  from rigidmultiblobswall_amd import forces

  class Body(object):
    def __init__(self, location):
      self.location = location

  L = pf.LADDER_BOX.copy() if box else None
  L3 = np.array([128.0, 128.0, 64.0]) if box else None
  kw = dict(periodic_length=L, repulsion_strength=EPS, debye_length=B, blob_radius=A)
  for x in pf.LADDER:
    r = pf.ladder_pair(x, 2 * A, B, box)
    zero = x > 750
    for fn in (forces.calc_blob_blob_forces_hip, forces.calc_blob_blob_forces_tree_hip):
      got = fn(r, **kw)
      assert forces._context(2).get_option("last_path") == 0
      _ladder_bound("contact", got, r, L)
      assert not zero or not np.ascontiguousarray(got).view(np.uint64).any(), (x, got)
    got = forces.calc_blob_blob_forces_radii_hip(r, np.array(pf.LADDER_RADII), **kw)
    assert forces._context(2).get_option("last_path") == 0
    _ladder_bound("radii", got, r, L, radii=np.array(pf.LADDER_RADII))
    assert not zero or not np.ascontiguousarray(got).view(np.uint64).any(), (x, got)
    if x > 0:
      ry = pf.ladder_pair(x, 0.0, B, box)
      got = forces.calc_body_body_forces_torques_hip([Body(ry[0]), Body(ry[1])], None, periodic_length=L3, repulsion_strength=EPS, debye_length=B)
      assert forces._context(2).get_option("last_path") == 1
      assert not got[1::2].any()          # no torque
      _ladder_bound("yukawa", got[0::2], ry, L3)
      assert not zero or not np.ascontiguousarray(got).view(np.uint64).any(), (x, got)
  forces.reset()


@pytest.mark.parametrize("form", pf.ENERGY_FORMS)
@pytest.mark.parametrize("band", pf.BANDS, ids=lambda b: "%d_%d" % b)
def test_slab_pair_energies(Ctx, band, form):
  pg.run_slab(Ctx, band, form)


@pytest.mark.parametrize("form", pf.ENERGY_FORMS)
@pytest.mark.parametrize("box", [False, True], ids=["open", "box"])
def test_energies_two_blobs_over_the_ladder(Ctx, form, box):
  pg.run_ladder_energy(Ctx, form, box)


@pytest.mark.parametrize("form", ("soft", "yukawa"))
def test_wall_term_one_blob_over_the_ladder(Ctx, form):
  pg.run_wall_ladder(Ctx, form)


@pytest.mark.parametrize("form", ("soft", "yukawa"))
@pytest.mark.parametrize("box", [False, True], ids=["open", "box"])
@pytest.mark.parametrize("band", pf.BANDS, ids=lambda b: "%d_%d" % b)
def test_body_delta_of_a_moved_slab(Ctx, band, box, form):
  pg.run_body_delta(Ctx, band, form, box)
