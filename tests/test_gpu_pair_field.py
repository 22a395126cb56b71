"""The HIP pair correlation of a quantised per-point field (rmb_pair_field_frames_device, bond_order_kernels.h) against the int64
numpy restatement (_bond_order_numpy.pair_field) and the pair histogram.

Every comparison is EXACT equality of integers.  That is a fair demand because every input satisfies, and every case asserts, the
edge-margin precondition of the pair histogram's tests: in long double no pair has r / dr within 1e-9 of an integer, so every
correct implementation bins every pair alike; the sums are integer arithmetic on the same terms."""
import numpy as np
import pytest
import torch

import _bond_order_numpy as bo
from rigidmultiblobswall_amd import bondorder
from rigidmultiblobswall_amd._lib import RmbError

pytestmark = pytest.mark.gpu

BOX = np.array([7.0, 5.0, 3.0])
R_MAX = 2.5
BINS = (1, 7, 4096)
PLANES = ("xy", "xyz")


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _dev(a, dtype=np.float64):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


_CASES = {}


def _case(n, F, periodic):
  """frames (F, n, 3) with +-2 periods of offset per point, an int32 field with +-2^30 and 0 planted, and L: once per shape; the
  bin margin holds for every bin count and both planes"""
  if (n, F, periodic) not in _CASES:
    L = BOX * (1.0 if periodic else 0.0)
    span = BOX if n > 2 else np.array([0.7, 0.7, 0.3])
    for seed in range(50 * n + F, 50 * n + F + 20):
      rng = np.random.RandomState(seed)
      frames = rng.uniform(0, 1, (F, n, 3)) * span + rng.randint(-2, 3, (F, n, 3)) * L
      if all(bo.bin_margin(frames, L, R_MAX, b, plane) > bo.MARGIN for b in BINS for plane in PLANES):
        break
    else:
      pytest.fail("no seed keeps every pair off the bin edges")
    _CASES[(n, F, periodic)] = (frames, bo.random_field(rng, (F, n)), L)
  return _CASES[(n, F, periodic)]


def _run(ctx, frames, field, L, n_bins, plane, r_max=R_MAX, **kw):
  counts, sums = ctx.pair_field_correlation_frames_device(_dev(frames), _dev(field, np.int32), L, r_max, n_bins, plane=plane, **kw)
  assert counts.dtype == torch.int64 and sums.dtype == torch.int64 and counts.is_cuda and tuple(counts.shape) == tuple(sums.shape) == (n_bins,)
  return counts.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("F", [1, 7])
@pytest.mark.parametrize("n", [1, 2, 64, 65, 129])
def test_counts_and_sums_equal_the_restatement(ctx, n, F, periodic):
  frames, field, L = _case(n, F, periodic)
  for plane in PLANES:
    for n_bins in BINS:
      counts, sums = _run(ctx, frames, field, L, n_bins, plane)
      ref_c, ref_s = bo.pair_field(frames, field, L, R_MAX, n_bins, plane)
      assert np.array_equal(counts, ref_c) and np.array_equal(sums, ref_s)
      if n == 1:
        assert not counts.any() and not sums.any()
      if n >= 2 and n_bins == 1:
        assert counts[0] >= F and (n < 64 or sums[0] != 0)


@pytest.mark.parametrize("periodic", [False, True])
def test_unit_field_is_the_pair_histogram(ctx, periodic):
  """the field (2^30, 0): every term is exactly 2^30, and the counts are pair_histogram_frames_device's, bit for bit"""
  frames, _, L = _case(129, 7, periodic)
  unit = np.zeros((7, 129, 2), dtype=np.int32)
  unit[..., 0] = 2 ** 30
  for plane in PLANES:
    f3, L3 = bo._in_plane(frames, L, plane)      # in the plane: the same points with z = 0, open in z
    for n_bins in BINS:
      counts, sums = _run(ctx, frames, unit, L, n_bins, plane)
      hist = ctx.pair_histogram_frames_device(_dev(f3), L3, R_MAX, n_bins).cpu().numpy()
      assert np.array_equal(sums, counts * 2 ** 30) and np.array_equal(counts, hist) and counts.sum() > 0
  # the other corner: (-2^30, -2^30) against itself is 2^31 per pair
  low = np.full((7, 129, 2), -2 ** 30, dtype=np.int32)
  counts, sums = _run(ctx, frames, low, L, 7, "xyz")
  assert np.array_equal(sums, counts * 2 ** 31)


def test_permutation_accumulation_and_plans(ctx):
  frames, field, L = _case(129, 7, True)
  c0, s0 = _run(ctx, frames, field, L, 7, "xy")
  perm = np.random.RandomState(8).permutation(129)
  c1, s1 = _run(ctx, frames[:, perm], field[:, perm], L, 7, "xy")
  assert np.array_equal(c0, c1) and np.array_equal(s0, s1)
  # two half-trajectories accumulated into one out= equal one call; the tensors handed in are handed back
  counts = torch.zeros(7, dtype=torch.int64, device="cuda")
  sums = torch.zeros(7, dtype=torch.int64, device="cuda")
  for part in (slice(0, 3), slice(3, 7)):
    a, b = ctx.pair_field_correlation_frames_device(_dev(frames[part]), _dev(field[part], np.int32), L, R_MAX, 7, plane="xy", counts=counts, sums=sums)
    assert a is counts and b is sums
  assert np.array_equal(counts.cpu().numpy(), c0) and np.array_equal(sums.cpu().numpy(), s0)
  # a reach beyond every separation of an open box: every unordered pair is met exactly once
  fo, fld, L0 = _case(129, 7, False)
  c, s = _run(ctx, fo, fld, L0, 1, "xyz", r_max=1e3)
  assert c[0] == 7 * 129 * 128 // 2


def test_capacity_guard(ctx):
  """a bin whose accumulated count reaches 2^32 is refused (synthetic: the accumulator is set just below)"""
  acc = bondorder.BondOrder(2, np.zeros(3), orders=(6,), r_cut=1.0, r_max=1.0, n_bins=1, ctx=ctx)
  pair = np.array([[[0.0, 0.0, 0.0], [0.25, 0.0, 0.0]]])
  acc.add_frames(pair)
  assert acc.pair_counts().tolist() == [[1]] and acc.pair_sums().tolist() == [[2 ** 30]]      # psi_6 = 1 for both
  acc._counts[0, 0] = 2 ** 32 - 2
  acc.add_frames(pair)
  with pytest.raises(OverflowError, match="2\\^32"):
    acc.add_frames(pair)
  acc.close()


def test_refused_calls(ctx):
  frames, field, L = _case(65, 7, True)
  dev, fld = _dev(frames), _dev(field, np.int32)
  with pytest.raises(ValueError, match="frames must be"):
    ctx.pair_field_correlation_frames_device(dev.float(), fld, L, 1.0, 4)
  for bad in (fld.long(), fld.cpu(), fld[:, :64].contiguous(), fld.transpose(0, 1)):
    with pytest.raises(ValueError, match="field must be"):
      ctx.pair_field_correlation_frames_device(dev, bad, L, 1.0, 4)
  with pytest.raises(ValueError, match="plane must be"):
    ctx.pair_field_correlation_frames_device(dev, fld, L, 1.0, 4, plane="xz")
  with pytest.raises(ValueError, match="counts must be"):
    ctx.pair_field_correlation_frames_device(dev, fld, L, 1.0, 4, counts=torch.zeros(5, dtype=torch.int64, device="cuda"))
  with pytest.raises(ValueError, match="sums must be"):
    ctx.pair_field_correlation_frames_device(dev, fld, L, 1.0, 4, sums=torch.zeros(4, dtype=torch.float64, device="cuda"))
  for kw in (dict(r_max=0.0, n_bins=4), dict(r_max=float("inf"), n_bins=4), dict(r_max=1.0, n_bins=0), dict(r_max=1.0, n_bins=4097)):
    with pytest.raises(RmbError):
      ctx.pair_field_correlation_frames_device(dev, fld, L, **kw)
  # nothing to count leaves the accumulators as they are
  counts, sums = torch.full((4,), 7, dtype=torch.int64, device="cuda"), torch.full((4,), -7, dtype=torch.int64, device="cuda")
  for f, q in ((dev[:0], fld[:0]), (dev[:, :0].contiguous(), fld[:, :0].contiguous()), (dev[:, :1].contiguous(), fld[:, :1].contiguous())):
    ctx.pair_field_correlation_frames_device(f, q, L, 1.0, 4, counts=counts, sums=sums)
  assert counts.tolist() == [7] * 4 and sums.tolist() == [-7] * 4
