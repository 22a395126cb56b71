"""The HIP van Hove sweeps (rmb_van_hove_self_frames_device, rmb_van_hove_distinct_frames_device, van_hove_kernels.h) and
rigidmultiblobswall_amd.vanhove against the numpy restatement (_van_hove_numpy.py) and the pair histogram.

Every comparison of counts is EXACT equality.  That is a fair demand because every input satisfies, and every test asserts, the
edge-margin precondition: in long double no term has r / dr within 1e-9 of an integer, while fp64 evaluation errors of r are
~1e-15 relative -- so every correct implementation bins every term alike.  Inputs that fail get another seed; terms at exactly
r = 0 (lag 0 of the self part, coincident points built on purpose) are exempt.

The moments are held to a derived bound, not a measured one: against the long-double evaluation of the same fp64 inputs,
|M - M_ext| <= (n_terms + 16) 2^-53 M_ext per lag and moment (_van_hove_numpy.moment_bound: all terms are non-negative, so any
summation order stays within n_terms - 1 units; a term carries at most 5 roundings in r^2 and 11 in r^4).  The worst fraction of
the bound met by the cases below is printed by each case (run with -s) and recorded in DESIGN.md 3.9.3."""
import io
import os

import numpy as np
import pytest
import torch

import _pair_hist_numpy as phnp
import _van_hove_numpy as vh
from conftest import golden_files, load_golden
from rigidmultiblobswall_amd import correlation, vanhove
from rigidmultiblobswall_amd._lib import RmbError

pytestmark = pytest.mark.gpu

BOX = np.array([7.0, 5.0, 3.0])
MODES = {"open": (0, 0, 0), "xy": (1, 1, 0), "xyz": (1, 1, 1)}
SIZES = (1, 2, 63, 64, 65, 130, 257)      # tile edges, two and five tiles (25 tile pairs per origin: many workgroups per lag)
F = 6
R_MAX, N_BINS, SELF_R_MAX, SELF_BINS = 2.5, 500, 0.6, 300


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


_CASES = {}


def _case(n, mode):
  """(frames (F, n, 3), L) of a random walk with +-2 periods of offset per point in the periodic directions, computed once and
  shared; the margin precondition holds for 4 lags from every origin, in both planes"""
  if (n, mode) not in _CASES:
    periods = MODES[mode]
    L = BOX * np.asarray(periods, dtype=np.float64)
    make = vh.random_walk(n, F, BOX, 0.05, periods if any(periods) else None)
    frames = vh.trajectory_with_margin(make, L, 4, R_MAX, N_BINS, SELF_R_MAX, SELF_BINS, 100 * n + len(mode))
    _CASES[(n, mode)] = (frames, L)
  return _CASES[(n, mode)]


def _both(ctx, frames, L, n_lags, plane="xyz", origins="window", o_begin=0, o_end=None, r_max=R_MAX, n_bins=N_BINS, self_r_max=SELF_R_MAX,
          self_bins=SELF_BINS):
  dev = frames if isinstance(frames, torch.Tensor) else _dev(frames)
  Hs, M = ctx.van_hove_self_frames_device(dev, n_lags, self_r_max, self_bins, origins=origins, plane=plane, o_begin=o_begin, o_end=o_end)
  Hd = ctx.van_hove_distinct_frames_device(dev, L, n_lags, r_max, n_bins, origins=origins, plane=plane, o_begin=o_begin, o_end=o_end)
  assert Hs.dtype == torch.int64 and Hs.is_cuda and tuple(Hs.shape) == (n_lags, self_bins)
  assert M.dtype == torch.float64 and tuple(M.shape) == (n_lags, 2) and tuple(Hd.shape) == (n_lags, n_bins)
  return Hs.cpu().numpy(), M.cpu().numpy(), Hd.cpu().numpy()


def _check_moments(M, frames, n_lags, o0, o1, plane):
  """the derived bound; -> the worst fraction of it"""
  M_ext, terms = vh.moments(frames, n_lags, o0, o1, plane, vh.EXT)
  bound = vh.moment_bound(M_ext, terms)
  err = np.abs(M.astype(vh.EXT) - M_ext)
  assert np.all(err <= bound), (err, bound)
  ok = bound > 0
  return float(np.max(err[ok] / bound[ok])) if ok.any() else 0.0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", SIZES)
def test_counts_and_moments_equal_the_restatement(ctx, n, mode):
  frames, L = _case(n, mode)
  dev = _dev(frames)
  worst = 0.0
  for n_lags in (1, 4):
    for plane in ("xyz", "xy"):
      for origins, (o0, o1) in (("window", (0, None)), ("all", (0, None)), ("all", (1, 4))):
        b0, b1 = vh.origin_range(F, n_lags, origins) if o1 is None else (o0, o1)
        # the terms of these origins and lags are among those whose margin _case() has asserted
        Hs, M, Hd = _both(ctx, dev, L, n_lags, plane, origins, o0, o1)
        assert np.array_equal(Hs, vh.self_counts(frames, n_lags, b0, b1, SELF_R_MAX, SELF_BINS, plane))
        assert np.array_equal(Hd, vh.distinct_counts(frames, L, n_lags, b0, b1, R_MAX, N_BINS, plane))
        worst = max(worst, _check_moments(M, frames, n_lags, b0, b1, plane))
        if n == 1:
          assert Hd.sum() == 0
        if n >= 65 and plane == "xy":
          assert Hd.sum() > 0 and Hs[-1].sum() > 0
  print("moments: worst fraction of the bound, n = %d, %s: %.3g" % (n, mode, worst))


GOLDENS = golden_files("g17_gr_*.npz")


def test_lag_zero_is_twice_the_pair_histogram(ctx):
  """bit for bit, whatever the margins: the image is odd in the separation, both entries share the bin arithmetic"""
  for n, mode in ((130, "open"), (257, "xy"), (65, "xyz")):
    frames, L = _case(n, mode)
    dev = _dev(frames)
    pairs = ctx.pair_histogram_frames_device(dev, L, R_MAX, N_BINS)
    Hd = ctx.van_hove_distinct_frames_device(dev, L, 3, R_MAX, N_BINS, origins="all")
    assert torch.equal(Hd[0], 2 * pairs) and int(pairs.sum()) > 0


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[7:-4] for p in GOLDENS])
def test_lag_zero_on_the_reference_frames(ctx, path):
  """the frames of the reference program's g(r) goldens: Hd[0] is the program's integer column"""
  d = load_golden(path)
  frames, L, n_bins = d["frames"], d["periodic_length"], int(d["n_bins"])
  hist = phnp.parse_gr(str(d["output"]))[2]
  dev = _dev(frames)
  Hd = ctx.van_hove_distinct_frames_device(dev, L, 2, 0.5 * L[0], n_bins, origins="all")
  pairs = ctx.pair_histogram_frames_device(dev, L, 0.5 * L[0], n_bins)
  assert torch.equal(Hd[0], 2 * pairs) and np.array_equal(Hd[0].cpu().numpy(), hist)
  assert int(Hd[1].sum()) > 0


def test_lag_and_flush_paths(ctx):
  L = BOX * np.array([1.0, 1.0, 0.0])
  # 7 lags over 8 frames of 5 points: one tile pair per origin, a handful of units per lag
  make = vh.random_walk(5, 8, BOX, 0.05, (1, 1, 0))
  frames = vh.trajectory_with_margin(make, L, 7, R_MAX, N_BINS, SELF_R_MAX, SELF_BINS, 31, planes=("xyz",))
  for origins in ("window", "all"):
    o0, o1 = vh.origin_range(8, 7, origins)
    Hs, M, Hd = _both(ctx, frames, L, 7, origins=origins)
    assert np.array_equal(Hs, vh.self_counts(frames, 7, o0, o1, SELF_R_MAX, SELF_BINS))
    assert np.array_equal(Hd, vh.distinct_counts(frames, L, 7, o0, o1, R_MAX, N_BINS))
    _check_moments(M, frames, 7, o0, o1, "xyz")
  # more lags than frames: the lags without an origin stay zero
  Hs, M, Hd = _both(ctx, frames[:3], L, 7, origins="all")
  assert np.array_equal(Hs, vh.self_counts(frames[:3], 7, 0, 3, SELF_R_MAX, SELF_BINS)) and not Hs[3:].any() and Hs[2].sum() == 5
  assert np.array_equal(Hd, vh.distinct_counts(frames[:3], L, 7, 0, 3, R_MAX, N_BINS)) and not Hd[3:].any() and not M[3:].any()
  Hs, M, Hd = _both(ctx, frames[:3], L, 7, origins="window")      # no origin has every lag
  assert not Hs.any() and not Hd.any() and not M.any()
  # 257 points, open, a reach beyond every separation: many workgroups add to the same bins, every ordered pair is met once
  frames, L0 = _case(257, "open")
  reach = 4.0 * float(np.linalg.norm(frames.max(axis=(0, 1)) - frames.min(axis=(0, 1))))
  Hs, M, Hd = _both(ctx, frames, L0, 4, origins="all", r_max=reach, n_bins=8, self_r_max=reach, self_bins=8)
  assert np.array_equal(Hd.sum(axis=1), 257 * 256 * vh.n_origins(F, 4, 0, F))
  assert np.array_equal(Hs.sum(axis=1), 257 * vh.n_origins(F, 4, 0, F))


@pytest.mark.parametrize("n_bins", [1, 8192])
def test_bin_counts(ctx, n_bins):
  L = BOX * np.array([1.0, 1.0, 1.0])
  make = vh.random_walk(130, 4, BOX, 0.05, (1, 1, 1))
  frames = vh.trajectory_with_margin(make, L, 3, R_MAX, n_bins, SELF_R_MAX, n_bins, 500 + n_bins, planes=("xyz",))
  Hs, M, Hd = _both(ctx, frames, L, 3, origins="all", n_bins=n_bins, self_bins=n_bins)
  assert np.array_equal(Hs, vh.self_counts(frames, 3, 0, 4, SELF_R_MAX, n_bins))
  assert np.array_equal(Hd, vh.distinct_counts(frames, L, 3, 0, 4, R_MAX, n_bins)) and Hd.sum() > 0


def test_edge_values(ctx):
  L = BOX * np.array([1.0, 1.0, 0.0])
  # a reach below most displacements: dropped from the counts, present in the moments
  make = vh.random_walk(65, 5, BOX, 0.05, (1, 1, 0))
  frames = vh.trajectory_with_margin(make, L, 3, 0.4, 20, 0.05, 10, 900, planes=("xyz",))
  Hs, M, Hd = _both(ctx, frames, L, 3, origins="all", r_max=0.4, n_bins=20, self_r_max=0.05, self_bins=10)
  assert np.array_equal(Hs, vh.self_counts(frames, 3, 0, 5, 0.05, 10)) and np.array_equal(Hd, vh.distinct_counts(frames, L, 3, 0, 5, 0.4, 20))
  assert Hs[2].sum() < 65 * 3 and Hs[0].sum() == 65 * 5
  _check_moments(M, frames, 3, 0, 5, "xyz")
  assert M[2, 0] > 0.05 ** 2 * 65 * 3
  # points that sit at lag 1 exactly where OTHER points sat: r = 0, i != j, bin 0 of Hd[1] (across a tile edge)
  for seed in range(40, 60):
    rng = np.random.RandomState(seed)
    f = vh.random_walk(70, 2, BOX, 0.05, None)(rng)
    f[1, 60:68] = f[0, 50:58]
    if vh.edge_margin_distinct(f, L, 2, 0, 2, R_MAX, N_BINS) > vh.MARGIN:
      break
  else:
    pytest.fail("no seed keeps the cross-frame terms off the bin edges")
  ref = vh.distinct_counts(f, L, 2, 0, 2, R_MAX, N_BINS)
  Hd = ctx.van_hove_distinct_frames_device(_dev(f), L, 2, R_MAX, N_BINS, origins="all").cpu().numpy()
  assert np.array_equal(Hd, ref) and ref[1, 0] >= 8
  # the i = j term never appears: one moving point gives nothing, two give two ordered pairs per origin and lag
  one = vh.random_walk(1, 5, BOX, 0.05, None)(np.random.RandomState(1))
  out = torch.full((3, 16), 7, dtype=torch.int64, device="cuda")
  ctx.van_hove_distinct_frames_device(_dev(one), np.zeros(3), 3, 100.0, 16, origins="all", out=out)
  assert torch.equal(out, torch.full((3, 16), 7, dtype=torch.int64, device="cuda"))
  two = vh.random_walk(2, 5, BOX, 0.05, None)(np.random.RandomState(1))
  Hd = ctx.van_hove_distinct_frames_device(_dev(two), np.zeros(3), 3, 100.0, 16, origins="all").cpu().numpy()
  assert np.array_equal(Hd.sum(axis=1), 2 * vh.n_origins(5, 3, 0, 5))


def test_accumulation_determinism_permutation(ctx):
  frames, L = _case(130, "xy")
  dev = _dev(frames)
  Hs, M = ctx.van_hove_self_frames_device(dev, 4, SELF_R_MAX, SELF_BINS, origins="all")
  Hd = ctx.van_hove_distinct_frames_device(dev, L, 4, R_MAX, N_BINS, origins="all")
  Hs1, M1, Hd1 = Hs.clone(), M.clone(), Hd.clone()
  # the same call into new tensors: the same bits
  Hs2, M2 = ctx.van_hove_self_frames_device(dev, 4, SELF_R_MAX, SELF_BINS, origins="all")
  assert torch.equal(Hs2, Hs1) and torch.equal(M2.view(torch.int64), M1.view(torch.int64))
  # two calls add
  a, b = ctx.van_hove_self_frames_device(dev, 4, SELF_R_MAX, SELF_BINS, origins="all", out=Hs, moments=M)
  c = ctx.van_hove_distinct_frames_device(dev, L, 4, R_MAX, N_BINS, origins="all", out=Hd)
  assert a is Hs and b is M and c is Hd
  assert torch.equal(Hs, 2 * Hs1) and torch.equal(Hd, 2 * Hd1) and torch.equal(M, 2 * M1)
  # the points in another order: the same counts
  perm = np.random.RandomState(8).permutation(130)
  Hs3, M3, Hd3 = _both(ctx, frames[:, perm], L, 4, origins="all")
  assert np.array_equal(Hs3, Hs1.cpu().numpy()) and np.array_equal(Hd3, Hd1.cpu().numpy())
  _check_moments(M3, frames, 4, 0, F, "xyz")


def test_resident_configuration_is_left_alone():
  """a wall M_tt f of the resident blobs before and after, on the atomic-free sweep (option "deterministic")"""
  from rigidmultiblobswall_amd import MobilityContext
  rng = np.random.RandomState(4)
  r = rng.uniform(0, 6, (500, 3)) + np.array([0, 0, 0.5])
  f = rng.randn(1500)
  frames, L = _case(130, "xy")
  c = MobilityContext(0)
  try:
    c.set_option("deterministic", 1)
    c.set_positions(r, 0.2, wall=True)
    before, again = c.matvec("tt", f, 1.0), c.matvec("tt", f, 1.0)
    assert np.array_equal(before, again)      # the yardstick itself repeats
    dev = _dev(frames)
    c.van_hove_self_frames_device(dev, 4, SELF_R_MAX, SELF_BINS, origins="all")
    c.van_hove_distinct_frames_device(dev, L, 4, R_MAX, N_BINS, origins="all")
    c.van_hove_distinct_frames_device(dev, np.zeros(3), 4, R_MAX, N_BINS, plane="xy")
    torch.cuda.synchronize()
    after = c.matvec("tt", f, 1.0)
    assert np.array_equal(before, after) and c.n == 500
  finally:
    c.close()


@pytest.mark.parametrize("origins", ["window", "all"])
def test_streamed_in_pieces(ctx, origins):
  n, n_frames, n_lags = 65, 12, 4
  L = BOX * np.array([1.0, 1.0, 0.0])
  make = vh.random_walk(n, n_frames, BOX, 0.05, (1, 1, 0))
  frames = vh.trajectory_with_margin(make, L, n_lags, R_MAX, N_BINS, SELF_R_MAX, SELF_BINS, 70, planes=("xyz",))
  o0, o1 = vh.origin_range(n_frames, n_lags, origins)
  kw = dict(r_max=R_MAX, n_bins=N_BINS, self_r_max=SELF_R_MAX, self_n_bins=SELF_BINS, origins=origins, dt=0.5, ctx=ctx)
  shot = vanhove.VanHove(n, L, n_lags, **kw).add_frames(frames).finish()
  pieces = vanhove.VanHove(n, L, n_lags, **kw)
  k = 0
  for size in (1, 2, 3, 4, 2):      # numpy and device pieces, shorter and longer than the lags
    piece = frames[k:k + size]
    pieces.add_frames(piece if size % 2 else _dev(piece))
    k += size
  assert k == n_frames
  pieces.finish()
  Hs_ref, Hd_ref = vh.self_counts(frames, n_lags, o0, o1, SELF_R_MAX, SELF_BINS), vh.distinct_counts(frames, L, n_lags, o0, o1, R_MAX, N_BINS)
  for acc in (shot, pieces):
    assert acc.n_frames == n_frames
    assert np.array_equal(acc.n_origins(), vh.n_origins(n_frames, n_lags, o0, o1))
    assert np.array_equal(acc.counts(), n * vh.n_origins(n_frames, n_lags, o0, o1))
    assert np.array_equal(acc.self_counts(), Hs_ref) and np.array_equal(acc.distinct_counts(), Hd_ref)
    _check_moments(acc.moments(), frames, n_lags, o0, o1, "xyz")
    assert np.array_equal(acc.times(), 0.5 * np.arange(n_lags))
  # G_s: sum_b G_s shell_b is the fraction of displacements below self_r_max
  shell = vanhove.shell_volumes(SELF_R_MAX, SELF_BINS, "xyz")
  assert np.allclose((shot.Gs() * shell).sum(axis=1), Hs_ref.sum(axis=1) / shot.counts(), rtol=1e-13)
  M_ext, terms = vh.moments(frames, n_lags, o0, o1, "xyz", vh.EXT)
  assert np.allclose(shot.msd(), (M_ext[:, 0] / terms).astype(np.float64), rtol=1e-12)
  a2 = (0.6 * (M_ext[1:, 1] / terms[1:]) / (M_ext[1:, 0] / terms[1:]) ** 2 - 1).astype(np.float64)
  assert np.isnan(shot.alpha2()[0]) and np.allclose(shot.alpha2()[1:], a2, rtol=0, atol=1e-11)
  # G_d(r, 0) is g(r): the same integer counts through the same fp64 normalisation
  rd = correlation.RadialDistribution(n, L, r_max=R_MAX, n_bins=N_BINS, normalisation="pseudo2d", ctx=ctx)
  rd.add_frames(frames[o0:o1])
  g, Gd0 = rd.g(), shot.Gd("pseudo2d")[0]
  assert np.array_equal(shot.distinct_counts()[0], 2 * rd.counts.astype(np.int64))
  assert np.all(np.abs(Gd0 - g) <= 1e-14 * np.abs(g)) and g.max() > 0
  with pytest.raises(ValueError, match="three positive periods"):
    shot.Gd()
  with pytest.raises(ValueError, match="after finish"):
    shot.add_frames(frames[:1])
  rd.close()
  shot.close()
  pieces.close()
  assert ctx._h.value      # a caller's context stays open


def test_command_line(ctx, tmp_path):
  n, L = 12, np.array([7.0, 5.0, 0.0])
  make = vh.random_walk(n, 4, BOX, 0.08, (1, 1, 0))
  used = vh.trajectory_with_margin(make, L, 3, 2.0, 40, 0.5, 25, 210, planes=("xy",))      # the frames --skip 1 --every 2 keeps
  frames = vh.random_walk(n, 9, BOX, 0.05, None)(np.random.RandomState(0))
  frames[1::2] = used
  traj = tmp_path / "run.config"
  traj.write_text(phnp.config_text(frames))
  base = [str(traj), str(n), "7.0", "5.0", "0", "--lags", "3", "--dt", "0.5", "--rmax", "2.0", "--bins", "40", "--self-rmax", "0.5",
          "--self-bins", "25", "--plane", "xy", "--skip", "1", "--every", "2", "--origins", "all"]
  buf = io.StringIO()      # the module's main(), which `python -m rigidmultiblobswall_amd.vanhove` runs
  assert vanhove.main(base, out=buf) == 0
  blocks = vanhove.parse(buf.getvalue())
  Hs, Hd = vh.self_counts(used, 3, 0, 4, 0.5, 25, "xy"), vh.distinct_counts(used, L, 3, 0, 4, 2.0, 40, "xy")
  assert len(blocks) == 3
  for l, b in enumerate(blocks):
    assert b["t"] == 1.0 * l and b["n_origins"] == 4 - l
    assert np.array_equal(b["Hs"], Hs[l]) and np.array_equal(b["Hd"], Hd[l])
    assert np.allclose(b["Gd"], Hd[l] / ((4 - l) * n * (n / 35.0) * vanhove.shell_volumes(2.0, 40, "xy")), rtol=1e-13)
    assert np.allclose(b["Gs"], Hs[l] / ((4 - l) * n * vanhove.shell_volumes(0.5, 25, "xy")), rtol=1e-13)
  buf = io.StringIO()
  assert vanhove.main(base + ["--no-distinct"], out=buf) == 0
  blocks = vanhove.parse(buf.getvalue())
  assert len(blocks) == 3 and all("Hd" not in b and np.array_equal(b["Hs"], Hs[l]) for l, b in enumerate(blocks))


def test_refused_calls(ctx):
  frames, L = _case(65, "xy")
  dev = _dev(frames)
  for bad in (dev.float(), dev.cpu(), dev[:, :, :2], dev.transpose(0, 1)):
    with pytest.raises(ValueError, match="frames must be"):
      ctx.van_hove_self_frames_device(bad, 2, 1.0, 10)
    with pytest.raises(ValueError, match="frames must be"):
      ctx.van_hove_distinct_frames_device(bad, L, 2, 1.0, 10)
  for kw in (dict(plane="xz"), dict(origins="some")):
    with pytest.raises(ValueError, match="must be one of"):
      ctx.van_hove_self_frames_device(dev, 2, 1.0, 10, **kw)
    with pytest.raises(ValueError, match="must be one of"):
      ctx.van_hove_distinct_frames_device(dev, L, 2, 1.0, 10, **kw)
  with pytest.raises(ValueError, match="n_lags"):
    ctx.van_hove_self_frames_device(dev, 0, 1.0, 10)
  for out in (torch.zeros((2, 10), dtype=torch.float64, device="cuda"), torch.zeros((2, 11), dtype=torch.int64, device="cuda"),
              torch.zeros((2, 10), dtype=torch.int64)):
    with pytest.raises(ValueError, match="out must be"):
      ctx.van_hove_self_frames_device(dev, 2, 1.0, 10, out=out)
    with pytest.raises(ValueError, match="out must be"):
      ctx.van_hove_distinct_frames_device(dev, L, 2, 1.0, 10, out=out)
  with pytest.raises(ValueError, match="moments must be"):
    ctx.van_hove_self_frames_device(dev, 2, 1.0, 10, moments=torch.zeros((2, 3), dtype=torch.float64, device="cuda"))
  for kw in (dict(r_max=0.0, n_bins=10), dict(r_max=float("inf"), n_bins=10), dict(r_max=1.0, n_bins=8193), dict(r_max=1.0, n_bins=0)):
    with pytest.raises(RmbError):
      ctx.van_hove_self_frames_device(dev, 2, **kw)
    with pytest.raises(RmbError):
      ctx.van_hove_distinct_frames_device(dev, L, 2, **kw)
  with pytest.raises(RmbError, match="o_begin <= o_end <= n_frames"):
    ctx.van_hove_self_frames_device(dev, 2, 1.0, 10, o_begin=3, o_end=2)
  with pytest.raises(RmbError, match="o_begin <= o_end <= n_frames"):
    ctx.van_hove_distinct_frames_device(dev, L, 2, 1.0, 10, o_end=F + 1)
  # nothing to count leaves the outputs as they are
  out, mom = torch.full((2, 10), 7, dtype=torch.int64, device="cuda"), torch.full((2, 2), 0.5, dtype=torch.float64, device="cuda")
  for empty, kw in ((dev[:0], {}), (dev[:, :0].contiguous(), {}), (dev, dict(o_begin=2, o_end=2))):
    ctx.van_hove_self_frames_device(empty, 2, 1.0, 10, out=out, moments=mom, **kw)
    ctx.van_hove_distinct_frames_device(empty, L, 2, 1.0, 10, out=out, **kw)
  ctx.van_hove_distinct_frames_device(dev[:, :1].contiguous(), L, 2, 1.0, 10, out=out)
  assert torch.equal(out, torch.full((2, 10), 7, dtype=torch.int64, device="cuda")) and torch.equal(mom, torch.full_like(mom, 0.5))


def test_multi_device_context_refuses(ctx):
  from rigidmultiblobswall_amd.multi import MultiContext
  m = MultiContext([0])
  try:
    assert not hasattr(m, "van_hove_self_frames_device")
    with pytest.raises(ValueError, match="single-GPU MobilityContext"):
      vanhove.VanHove(2, BOX, 2, ctx=m)
  finally:
    m.close()
