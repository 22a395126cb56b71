"""Every 3 x 3 pair block of the mobility, element by element, through every HIP kernel family, against the
extended-precision restatement of tests/_mobility_numpy.py:

    |got - EXT| <= MARGIN * C_ORACLE[kind, boundary, periodic] * 2^-53 * s_ij          (MARGIN = 4)

with the scale s_ij and the yardstick C_ORACLE of that module (the fp64 oracle's own worst error in the same units,
measured on the CPU by tests/test_pair_blocks_host.py -- 7 to 25 rounding units in open boundaries, 110 to 255 in a box,
where the oracle's fp64 wrap is the larger part); `precision` = 32 in units of 2^-24 s_ij against C_ORACLE32.  The margin
covers what the kernels do differently from the formulas as written -- rsqrt plus one cubic step for sqrt and the divide,
powers of a folded into constants, the wall terms reassociated into closed-form polynomials: a few roundings each.  A
dropped or mis-signed term, a wrong branch at r = 2a or a wrong coefficient is off by 1e-13 of the scale or more:
hundreds of units.

The blocks are extracted with the 3N unit vectors on the designed clouds of _mobility_numpy.regime_cloud (N = 200: three
full 64-blob tiles and one of eight; open, shifted to 1e6 a, and in a non-power-of-two and a power-of-two box); the families
and the kernel each one pins (`last_path`, asserted after every launch) are listed in tests/_pair_blocks_gpu.py.
tools/pair_blocks_report.py runs this file and writes the worst ratio per (family, kind, boundary)."""
import numpy as np
import pytest

import _mobility_numpy as mn
import _pair_blocks_gpu as pb
from _mobility_numpy import A, ETA
from conftest import KERNEL_KEYS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Ctx():
  from rigidmultiblobswall_amd import MobilityContext
  return MobilityContext


@pytest.fixture(scope="module")
def eye():
  import torch
  return torch.eye(3 * mn.N_CLOUD, dtype=torch.float64, device="cuda")


def test_the_reference_is_extended_precision_and_the_clouds_hold_every_class():
  assert mn.LONG_DOUBLE, "np.longdouble has no 64-bit mantissa here: fp64 would be compared with fp64"
  for name, (periodic, offset, classes) in mn.CLOUDS.items():
    r, L = mn.cloud(name)          # asserts the coverage of `classes`, no coincident blobs, no ties
    c = mn.coverage(r, A, L)
    assert all(c[k] >= 1 for k in classes) and c["ties"] == 0 and c["exactly_coincident"] == 0, (name, c)
    assert len(r) == mn.N_CLOUD and len(r) % 64 and (len(r) + 63) // 64 >= 4       # a partial tile; sym2t needs four tiles


@pytest.mark.parametrize("family,boundary,cloud", pb.all_cases(), ids=lambda v: str(v))
def test_blocks_elementwise(Ctx, eye, family, boundary, cloud):
  pb.run_case(Ctx, family, boundary, cloud, eye)


_HOST_KEYS = {"no_wall_tt": ("tt", "none", False), "wall_tt": ("tt", "wall", False), "in_plane_tt": ("tt", "wall", True),
              "no_wall_tr": ("tr", "none", False), "wall_tr": ("tr", "wall", False), "in_plane_tr": ("tr", "wall", True),
              "no_wall_rt": ("rt", "none", False), "wall_rt": ("rt", "wall", False), "no_wall_rr": ("rr", "none", False),
              "wall_rr": ("rr", "wall", False), "free_surface_tt": ("tt", "free", False)}
# three designed pairs (a = 1/2): r = 2a exactly in the plane z = a;  overlapping and oblique with one blob below z = a
# (clamped and damped);  1000 a apart, both low (the far-field cancellation with the image)
_PAIRS = {"contact_at_2a": [[0.0, 0.0, 0.5], [1.0, 0.0, 0.5]],
          "overlap_one_damped": [[0.125, 0.25, 0.15], [0.125 + 0.6 * 0.25, 0.25, 0.15 + 0.8 * 0.25]],
          "far_low": [[0.0, 0.0, 1.5], [500.25, 3.5, 0.75]]}


@pytest.mark.parametrize("pair", sorted(_PAIRS))
def test_host_wrappers_two_blobs(pair):
  """mobility.*_hip at N = 2: the smallest launch, through the C ABI and the one-sided sweep."""
  from rigidmultiblobswall_amd import mobility as mob
  assert set(_HOST_KEYS) == set(KERNEL_KEYS)
  r = np.array(_PAIRS[pair])
  for key, (kind, boundary, in_plane) in sorted(_HOST_KEYS.items()):
    fn = getattr(mob, KERNEL_KEYS[key] + "_hip")
    M = np.empty((6, 6))
    e = np.zeros(6)
    for k in range(6):
      e[k] = 1.0
      M[:, k] = fn(r, e, ETA, A)
      e[k] = 0.0
      assert mob._context(2).get_option("last_path") == 0
    E = mn.blocks(kind, boundary, r, A, ETA, in_plane=in_plane)
    s = mn.scale(kind, boundary, r, A, ETA)
    c = mn.C_ORACLE[kind, boundary, False] * pb.EPS[64]
    ratio, i, j, p, q = mn.worst_ratio(mn.from_dense(M), E, s, c)
    pb.RESULTS["host_wrapper_n2", kind, boundary] = max(pb.RESULTS.get(("host_wrapper_n2", kind, boundary), 0.0), ratio)
    assert ratio <= mn.MARGIN, ("host wrapper %s, pair %s: block (%d, %d) element (%d, %d) off by %.1f C; regime %s"
                                % (key, pair, i, j, p, q, ratio, mn.regime_of(r, A, i, j)))
