"""The seven wave-owned symmetric kernels with one target blob per lane under every cut of their step range: the walk of
csrc/sym_walk.h, and the same loop where a kernel still writes it out.  Cases and inputs are those of
tools/sym_walk_bits.py (257 blobs: 5 tiles, the last one partial): mobility products with the force and torque on one blob,
pair forces of isolated dimers -- every target's sum has one non-zero term, so the result words do not depend on the order
in which the atomics land, and every plan must give the SAME WORDS as the default one:
  `sym_chunk_steps` 16 with `sym_min_steps` 7, `sym_order` flipped, `sym_xcd` flipped, the sum of three pair shards.
Each kernel is reached through the options that select it (`last_path` asserted after every launch; the DET variant of
symx_kernel is what "deterministic" = 2 selects -- 1 is the one-sided sweep).

Against the references, at the bounds the kernels' own tests use, nothing new: 1e-12 relative L2 against the CPU oracle in
fp64 (tests/test_gpu_parity.py: TOL_D2), between 1e-9 and 1e-5 / 2e-5 for the fp32 twins (tests/test_gpu_ops.py: below
1e-9 the fp64 kernel would have run), MARGIN C 2^-53 S per component against the extended-precision restatement for the table law (tests/test_gpu_pair_table.py)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

sys.path.insert(0, os.path.join(ROOT, "tools"))
import sym_walk_bits as bits      # noqa: E402
import _pair_forces_numpy as pf   # noqa: E402
import _pair_table_numpy as pt    # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = bits.groups()


@pytest.fixture(scope="module")
def Ctx():
  from rigidmultiblobswall_amd import MobilityContext
  return MobilityContext


def _only_partners(forces_of, r, pairs):
  """The float64 restatement on the whole cloud equals, bit for bit, the restatement on each dimer alone: every non-partner
  term is exactly +-0 (x + 0 = x).  A condition on the inputs, not a tolerance."""
  full = np.asarray(forces_of(r, np.arange(len(r))), dtype=np.float64)
  alone = np.zeros_like(full)
  for i, j in pairs:
    alone[[i, j]] = np.asarray(forces_of(r[[i, j]], np.array([i, j])), dtype=np.float64)
  assert np.array_equal(full.view(np.uint64), alone.view(np.uint64))
  paired = np.zeros(len(r), dtype=bool)
  paired[np.array(pairs).reshape(-1)] = True
  assert np.all(np.any(full[paired] != 0.0, axis=1)) and not full[~paired].any()
  tiles = np.array(pairs) // 64
  assert (tiles[:, 0] == tiles[:, 1]).sum() >= 4 and (tiles[:, 0] != tiles[:, 1]).sum() >= 4      # diagonal and off-diagonal units


def test_dimers_are_isolated():
  eps, b, a = bits.FORCE["eps"], bits.FORCE["b"], bits.FORCE["a"]
  rad = bits.radii()
  r, pairs = bits.dimers(a, 3 * a)
  _only_partners(lambda x, idx: pf.forces("contact", x, None, eps, b, a, dtype=np.float64), r, pairs)
  _only_partners(lambda x, idx: pf.forces("radii", x, None, eps, b, a, radii=rad[idx], dtype=np.float64), r, pairs)
  # the fp32 kernel culls at 2a + 110 b and its exponential is zero long before the next dimer
  x = pf.pair_x("contact", r, None, b, a)[0]
  partner = np.zeros((bits.N, bits.N), dtype=bool)
  for i, j in pairs:
    partner[i, j] = partner[j, i] = True
  assert x[~partner].min() > 2000.0 and x[partner].max() < 7.0
  T = bits.pair_table()
  rt, pairs_t = bits.dimers(0.9, 2.4)
  _only_partners(lambda x, idx: pt.forces(T, x, None, dtype=np.float64)[0], rt, pairs_t)


@pytest.mark.parametrize("group", GROUPS, ids=[g.name.replace(" ", "_") for g in GROUPS])
def test_every_plan_gives_the_words_of_the_default_plan(Ctx, oracle, group):
  if group.name.startswith("forces"):
    test_dimers_are_isolated()          # before anything is launched
  res = bits.run_group(Ctx, group)
  for case in group.cases:
    base = res[case.name, "default"]
    assert np.all(np.isfinite(base)) and base.any(), case.name
    for plan in bits.PLANS[1:] + (("shards3",) if case.shards else ()):
      other = res[case.name, plan]
      same = base.view(np.uint64) == other.view(np.uint64)
      assert same.all(), "%s: plan %s differs from the default plan in %d of %d words, first at %d: %r vs %r" % (
          case.name, plan, (~same).sum(), same.size, int(np.argmin(same)), other[np.argmin(same)], base[np.argmin(same)])
    if case.ref == "table":
      rt, _ = bits.dimers(0.9, 2.4)
      F, S = pt.forces(bits.pair_table(), rt, None)
      q = pt.ratios(base.reshape(-1, 3), F, S, pt.C["force", False])
      print("%-48s worst %.3f C" % (case.name, float(q.max())))
      assert q.max() <= pt.MARGIN, (case.name, float(q.max()))
    else:
      ref = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in case.ref(oracle)])
      e = rel_err(base, ref)
      print("%-48s rel L2 %.3e (bound %g)" % (case.name, e, case.tol))
      assert e < case.tol, (case.name, e)
      if "32" in case.kernel:      # last_path is 1 for the fp64 kernel too: single-precision error shows that the fp32 twin ran
        assert e > 1e-9, (case.name, e)
