"""The HIP neighbour sweep of the bond-orientational order (rmb_bond_order_frames_device, bond_order_kernels.h) against the
long-double restatement with true trigonometry (_bond_order_numpy.py).

N_i is compared EXACTLY.  That is a fair demand because every input satisfies, and every case asserts through
frames_with_margin / cut_margin, the precondition: in long double no pair has d / r_cut within 1e-9 of 1, while the fp64 error
of d is ~1e-15 relative (1e-12 for the lattice shifted by 1000 periods).

Every sum is held to the DERIVED bound of DESIGN.md 3.9.4, computed from the data (_bond_order_numpy.sum_bound):
|S - S_ext| <= N_i E_m + N_i (N_i - 1) 2^-53,  E_m = m (eps_rsqrt + c 2^-53 max_j |d_raw| / rho) + 2 floor(log2 m) sqrt(5) 2^-53.
Each case prints its worst fraction of the bound (run with -s); the worst of all is recorded in profiles/r28_bond_order.json."""
import numpy as np
import pytest
import torch

import _bond_order_numpy as bo
from rigidmultiblobswall_amd._lib import RmbError

pytestmark = pytest.mark.gpu

BOX = np.array([7.0, 5.0, 3.0])
MODES = {"open": (0, 0, 0), "xy": (1, 1, 0), "xyz": (1, 1, 1)}
R_CUT = 1.1
ALL_ORDERS = (1, 4, 6, 12, 16)
ORDER_SETS = ((6,), (1, 4, 12, 16))      # K = 1 and K = 4


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


_CASES, _REFS = {}, {}


def _case(n, mode, F):
  """frames (F, n, 3) and L, computed once and shared: uniform points, +-2 periods of offset per point in the periodic
  directions; one or two points sit within the cutoff of each other; the cutoff margin holds in both planes"""
  if (n, mode, F) not in _CASES:
    periods = np.asarray(MODES[mode], dtype=np.float64)
    L = BOX * periods
    span = BOX if n > 2 else np.array([0.7, 0.7, 0.3])

    def make(rng):
      return rng.uniform(0, 1, (F, n, 3)) * span + rng.randint(-2, 3, (F, n, 3)) * L
    for seed in range(100 * n + F, 100 * n + F + 20):
      frames = make(np.random.RandomState(seed))
      if min(bo.cut_margin(frames, L, R_CUT, "xy"), bo.cut_margin(frames, L, R_CUT, "xyz")) > bo.MARGIN:
        break
    else:
      pytest.fail("no seed keeps every pair off the cutoff")
    _CASES[(n, mode, F)] = (frames, L)
  return _CASES[(n, mode, F)]


def _ref(key, frames, L, r_cut, plane):
  """long-double N, S (all orders of ALL_ORDERS), ratio: once per input and plane"""
  if (key, plane) not in _REFS:
    _REFS[(key, plane)] = bo.neighbour_sums(frames, L, r_cut, ALL_ORDERS, plane)
  return _REFS[(key, plane)]


def _run(ctx, frames, L, r_cut, orders, plane, source_chunk=0):
  f = np.asarray(frames, dtype=np.float64)
  f = f.reshape(-1, f.shape[-2], 3)
  out = ctx.bond_order_frames_device(_dev(f), L, r_cut, orders, plane=plane, source_chunk=source_chunk)
  assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (f.shape[0], f.shape[1], 1 + 2 * len(orders))
  return out.cpu().numpy()


def _check(out, ref, orders):
  """N exactly, every sum within the derived bound; -> the worst fraction of the bound"""
  N, S, ratio = ref
  cols = [ALL_ORDERS.index(m) for m in orders]
  assert np.array_equal(out[..., 0], N.astype(np.float64))
  got = out[..., 1:].reshape(out.shape[0], out.shape[1], len(orders), 2)
  bound = bo.sum_bound(N, ratio, orders)
  err = np.abs(got.astype(bo.EXT) - S[:, :, cols, :]).max(axis=-1).astype(np.float64)
  assert np.all(err <= bound), (float(err.max()), float((err / np.where(bound > 0, bound, 1)).max()))
  ok = bound > 0
  return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 513])
def test_sums_against_long_double(ctx, n, mode):
  worst = 0.0
  for F in ((1,) if n == 513 else (1, 5)):
    frames, L = _case(n, mode, F)
    for plane in ("xy", "xyz"):
      ref = _ref((n, mode, F), frames, L, R_CUT, plane)
      for orders in ORDER_SETS:
        out = _run(ctx, frames, L, R_CUT, orders, plane)
        worst = max(worst, _check(out, ref, orders))
        if n == 1:
          assert not out.any()
      if n >= 2:
        assert ref[0].max() >= 1
  print("bond order: worst fraction of the bound, n = %d, %s: %.3g" % (n, mode, worst))


def test_fp64_numpy_restatement_sits_inside_the_bound_on_these_inputs():
  frames, L = _case(65, "xy", 5)
  for plane in ("xy", "xyz"):
    N, S, ratio = _ref((65, "xy", 5), frames, L, R_CUT, plane)
    N64, S64 = bo.neighbour_sums_fp64(frames, L, R_CUT, ALL_ORDERS, plane)
    assert np.array_equal(N, N64)
    assert np.all(np.abs(S64.astype(bo.EXT) - S).max(axis=-1).astype(np.float64) <= bo.sum_bound(N, ratio, ALL_ORDERS))


@pytest.mark.parametrize("mode", ["open", "xy"])
def test_source_chunks(ctx, mode):
  """2 and 3 chunks of sources through the workspace and the finishing launch, against one chunk: the same N, sums within the bound"""
  frames, L = _case(130, mode, 2)
  for plane in ("xy", "xyz"):
    ref = _ref((130, mode, 2), frames, L, R_CUT, plane)
    orders = (1, 4, 12, 16)
    one = _run(ctx, frames, L, R_CUT, orders, plane, source_chunk=132)
    _check(one, ref, orders)
    bound = bo.sum_bound(ref[0], ref[2], orders)
    for chunk in (68, 44, 43):      # 68 + 62; 44 + 44 + 42; 43 is rounded up to 44
      out = _run(ctx, frames, L, R_CUT, orders, plane, source_chunk=chunk)
      _check(out, ref, orders)
      assert np.array_equal(out[..., 0], one[..., 0])
      diff = np.abs(out[..., 1:] - one[..., 1:]).reshape(2, 130, 4, 2).max(axis=-1)
      assert np.all(diff <= 2 * bound)
    assert np.array_equal(_run(ctx, frames, L, R_CUT, orders, plane, source_chunk=43), out)      # the same plan: the same bits


def _lattice_tol(pts, a, m):
  """the lattice's own fp64 coordinates: a bond vector is off by at most 4 u max|x|, its angle by that over a, z^m by m times"""
  return m * 8 * bo.U * np.abs(pts).max() / a


def _psi(out, K):
  N = out[..., 0]
  S = out[..., 1:].reshape(out.shape[0], out.shape[1], K, 2)
  return N, bo.psi_of(N, S)


@pytest.mark.parametrize("shift", [0.0, 1000.0])
def test_lattices(ctx, shift):
  """triangular: N = 6, |psi_6| = |psi_12| = 1, psi_4 = 0; square: N = 4, |psi_4| = |psi_12| = 1, psi_6 = 0 -- also shifted by
  1000 periods with every point a few more periods away (unwrapped)"""
  rng = np.random.RandomState(3)
  for kind, (pts, L), a, n_nb, one, zero in (("triangular", bo.triangular_lattice(8, 10, 1.25), 1.25, 6, (1, 2), 0),
                                            ("square", bo.square_lattice(9, 7, 0.75), 0.75, 4, (0, 2), 1)):
    x = pts + shift * L + (rng.randint(-3, 4, pts.shape) * L if shift else 0.0)
    r_cut, orders = 1.3 * a, (4, 6, 12)
    assert bo.cut_margin(x, L, r_cut) > 1e-3
    out = _run(ctx, x, L, r_cut, orders, "xy")
    ref = bo.neighbour_sums(x, L, r_cut, ALL_ORDERS, "xy")
    frac = _check(out, ref, orders)
    N, psi = _psi(out, 3)
    assert np.all(N == n_nb)
    # within the bound (per component, so sqrt(2) of it on the modulus) and the lattice's own rounding
    tol = np.sqrt(2) * bo.sum_bound(ref[0], ref[2], orders)[0] / n_nb + np.array([_lattice_tol(x, a, m) for m in orders])
    for k in one:
      assert np.all(np.abs(np.abs(psi[0, :, k]) - 1.0) <= tol[:, k]), kind
    assert np.all(np.abs(psi[0, :, zero]) <= tol[:, zero]), kind
    print("bond order: %s lattice, shift %g: fraction of the bound %.3g" % (kind, shift, frac))


def test_edge_pair_stacked_points_and_planes(ctx):
  L = np.array([4.0, 4.0, 0.0])
  # a pair across the box edge, several periods apart
  pts = np.array([[0.125, 2.0, 0.0], [3.875 + 3 * 4.0, 2.0 - 5 * 4.0, 0.0]])
  out = _run(ctx, pts, L, 0.5, (1, 4), "xy")
  _check(out, bo.neighbour_sums(pts, L, 0.5, ALL_ORDERS, "xy"), (1, 4))
  assert out[0, :, 0].tolist() == [1.0, 1.0] and np.allclose(out[0, 0, 1:], [1, 0, 1, 0], rtol=0, atol=1e-13)
  assert np.allclose(out[0, 1, 1:], [-1, 0, 1, 0], rtol=0, atol=1e-13)
  assert not _run(ctx, pts, np.zeros(3), 0.5, (1, 4), "xy").any()      # open box: 25 apart
  # two stacked points and a third: the stacked pair is left out under xy, and under xyz too although 0.5 < r_cut (rho = 0)
  pts = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.5], [1.75, 1.0, 0.0]])
  for plane in ("xy", "xyz"):
    out = _run(ctx, pts, L, 1.0, (1,), plane)
    assert out[0, :, 0].tolist() == [1.0, 1.0, 2.0] and np.all(np.isfinite(out))
    assert np.allclose(out[0, 0, 1:], [-1.0, 0.0], rtol=0, atol=1e-15) and np.allclose(out[0, 2, 1:], [2.0, 0.0], rtol=0, atol=1e-15)
  assert _run(ctx, pts, L, 0.8, (1,), "xyz")[0, :, 0].tolist() == [1.0, 0.0, 1.0]      # |(0.75, 0, 0.5)| = 0.90
  # a height-staggered square layer: in the plane every point has 4 neighbours, in 3-D only the 2 of its own row
  sq, Ls = bo.square_lattice(8, 8, 1.0)
  sq[:, 2] = 0.9 * ((np.arange(64) % 8) % 2)      # alternate rows of constant j
  for plane in ("xy", "xyz"):
    assert bo.cut_margin(sq, Ls, 1.2, plane) > 1e-3
    out = _run(ctx, sq, Ls, 1.2, (4,), plane)
    _check(out, bo.neighbour_sums(sq, Ls, 1.2, ALL_ORDERS, plane), (4,))
    assert np.all(out[0, :, 0] == (4 if plane == "xy" else 2))


def test_same_call_same_bits_and_out(ctx):
  frames, L = _case(513, "xy", 1)
  dev = _dev(frames)
  a = ctx.bond_order_frames_device(dev, L, R_CUT, (4, 6), plane="xy")
  b = ctx.bond_order_frames_device(dev, L, R_CUT, (4, 6), plane="xy")
  assert torch.equal(a.view(torch.int64), b.view(torch.int64))
  out = torch.full((1, 513, 5), 7.0, dtype=torch.float64, device="cuda")      # out= is overwritten, and handed back
  c = ctx.bond_order_frames_device(dev, L, R_CUT, (4, 6), plane="xy", out=out)
  assert c is out and torch.equal(out.view(torch.int64), a.view(torch.int64))
  # an order's sums do not depend on the orders next to it
  d = ctx.bond_order_frames_device(dev, L, R_CUT, (6,), plane="xy")
  assert torch.equal(d[..., 1:].contiguous().view(torch.int64), a[..., 3:].contiguous().view(torch.int64)) and torch.equal(d[..., 0], a[..., 0])


def test_refused_calls(ctx):
  frames, L = _case(65, "xy", 5)
  dev = _dev(frames)
  for bad in (dev.float(), dev.cpu(), dev[:, :, :2], dev.transpose(0, 1)):
    with pytest.raises(ValueError, match="frames must be"):
      ctx.bond_order_frames_device(bad, L, 1.0)
  with pytest.raises(ValueError, match="plane must be"):
    ctx.bond_order_frames_device(dev, L, 1.0, plane="xz")
  for orders in ((), (1, 2, 3, 4, 5), (0,), (17,), (6.0,)):
    with pytest.raises(ValueError, match="orders must be"):
      ctx.bond_order_frames_device(dev, L, 1.0, orders)
  for out in (torch.zeros((5, 65, 3), dtype=torch.float32, device="cuda"), torch.zeros((5, 65, 5), dtype=torch.float64, device="cuda"),
              torch.zeros((5, 65, 3), dtype=torch.float64)):
    with pytest.raises(ValueError, match="out must be"):
      ctx.bond_order_frames_device(dev, L, 1.0, out=out)
  for r_cut in (0.0, -1.0, float("inf"), float("nan")):
    with pytest.raises(RmbError, match="r_cut must be positive"):
      ctx.bond_order_frames_device(dev, L, r_cut)
  with pytest.raises(RmbError, match="source_chunk"):
    ctx.bond_order_frames_device(dev, L, 1.0, source_chunk=-4)
  # nothing to do leaves the output as it is
  out = torch.full((0, 65, 3), 7.0, dtype=torch.float64, device="cuda")
  assert ctx.bond_order_frames_device(dev[:0], L, 1.0, out=out) is out
  assert tuple(ctx.bond_order_frames_device(dev[:, :0].contiguous(), L, 1.0).shape) == (5, 0, 3)


def test_resident_configuration_is_left_alone():
  """a wall M_tt f of the resident blobs before and after, on the atomic-free sweep (which shares the workspace of chunk partials)"""
  from rigidmultiblobswall_amd import MobilityContext
  rng = np.random.RandomState(4)
  r = rng.uniform(0, 6, (500, 3)) + np.array([0, 0, 0.5])
  f = rng.randn(1500)
  frames, L = _case(130, "xy", 2)
  c = MobilityContext(0)
  try:
    c.set_option("deterministic", 1)
    c.set_positions(r, 0.2, wall=True)
    before, again = c.matvec("tt", f, 1.0), c.matvec("tt", f, 1.0)
    assert np.array_equal(before, again)
    c.bond_order_frames_device(_dev(frames), L, R_CUT, (4, 6), source_chunk=44)
    c.pair_field_correlation_frames_device(_dev(frames), torch.zeros((2, 130, 2), dtype=torch.int32, device="cuda"), L, 2.0, 16)
    torch.cuda.synchronize()
    assert np.array_equal(before, c.matvec("tt", f, 1.0)) and c.n == 500
  finally:
    c.close()


def test_multi_device_context_refuses():
  from rigidmultiblobswall_amd import bondorder
  from rigidmultiblobswall_amd.multi import MultiContext
  m = MultiContext([0])
  try:
    assert not hasattr(m, "bond_order_frames_device") and not hasattr(m, "pair_field_correlation_frames_device")
    with pytest.raises(ValueError, match="single-GPU MobilityContext"):
      bondorder.BondOrder(2, BOX, r_cut=1.0, ctx=m)
  finally:
    m.close()
