"""The van Hove functions without a GPU: the numpy restatement's own identities (_van_hove_numpy.py), the argument checks of the
two C entries with a null context, the Python and command-line argument errors, the normalisations on hand-made counts and the
table's write / parse round trip."""
import ctypes
import os

import numpy as np
import pytest

import _pair_hist_numpy as phnp
import _van_hove_numpy as vh
from rigidmultiblobswall_amd import vanhove

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = np.array([7.0, 5.0, 3.0])
R_MAX, N_BINS, SELF_R_MAX, SELF_BINS = 2.5, 500, 0.6, 300


def _trajectory(n, n_frames, n_lags, periods, seed):
  L = BOX * np.asarray(periods, dtype=np.float64)
  make = vh.random_walk(n, n_frames, BOX, 0.05, periods if any(periods) else None)
  return vh.trajectory_with_margin(make, L, n_lags, R_MAX, N_BINS, SELF_R_MAX, SELF_BINS, seed), L


@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 0), (1, 1, 1)])
def test_lag_zero_is_twice_the_pair_histogram(periods):
  """Hd[0] over the origins is exactly 2 x the unordered counts of the same frames, and the margins hold for both statements"""
  frames, L = _trajectory(65, 5, 3, periods, 11)
  assert phnp.edge_margin(frames, L, R_MAX, N_BINS) > phnp.MARGIN
  Hd = vh.distinct_counts(frames, L, 3, 0, 5, R_MAX, N_BINS)
  assert np.array_equal(Hd[0], 2 * phnp.counts(frames, L, R_MAX, N_BINS).astype(np.int64)) and Hd[0].sum() > 0
  # ordered pairs: every lag of every origin meets n (n - 1) of them when nothing is beyond reach
  far = vh.distinct_counts(frames, np.zeros(3), 3, 0, 5, 1e3, 7)
  assert np.array_equal(far.sum(axis=1), 65 * 64 * vh.n_origins(5, 3, 0, 5))


def test_rigid_drift():
  """x0 + f d: every self term of lag l sits in the bin of l |d|, alpha2 = d / (d + 2) - 1; a drift of whole periods leaves the
  distinct counts of a periodic box independent of the lag"""
  rng = np.random.RandomState(3)
  x0 = rng.uniform(0, 1, (40, 3)) * BOX
  d = np.array([0.031, -0.052, 0.017])
  frames = x0[None] + np.arange(6)[:, None, None] * d[None, None, :]
  for plane, dim in (("xyz", 3), ("xy", 2)):
    step = np.linalg.norm(d if plane == "xyz" else d[:2])
    assert vh.edge_margin_self(frames, 4, 0, 6, SELF_R_MAX, SELF_BINS, plane) > vh.MARGIN
    Hs = vh.self_counts(frames, 4, 0, 6, SELF_R_MAX, SELF_BINS, plane)
    n_or = vh.n_origins(6, 4, 0, 6)
    for l in range(4):
      b = int(l * step / (SELF_R_MAX / SELF_BINS))
      assert Hs[l, b] == 40 * n_or[l] and Hs[l].sum() == 40 * n_or[l]
    M, terms = vh.moments(frames, 4, 0, 6, plane)
    msd, a2 = vanhove.alpha2_from_moments(M, terms, plane)
    assert np.allclose(msd, (np.arange(4) * step) ** 2, rtol=1e-12)
    assert np.isnan(a2[0]) and np.allclose(a2[1:], dim / (dim + 2.0) - 1.0, rtol=0, atol=1e-12)
  L = BOX * np.array([1.0, 1.0, 1.0])
  whole = np.array([1.0, -2.0, 1.0]) * BOX
  frames = x0[None] + np.arange(4)[:, None, None] * whole[None, None, :]
  assert vh.edge_margin_distinct(frames, L, 3, 0, 2, R_MAX, N_BINS) > vh.MARGIN
  Hd = vh.distinct_counts(frames, L, 3, 0, 2, R_MAX, N_BINS)      # origins 0 and 1 have all three lags
  assert np.array_equal(Hd[1], Hd[0]) and np.array_equal(Hd[2], Hd[0]) and Hd[0].sum() > 0


def test_self_counts_sum_to_the_number_of_terms():
  frames, _ = _trajectory(65, 6, 4, (1, 1, 0), 5)
  for origins in ("window", "all"):
    o0, o1 = vh.origin_range(6, 4, origins)
    Hs = vh.self_counts(frames, 4, o0, o1, 50.0, 64)
    assert np.array_equal(Hs.sum(axis=1), 65 * vh.n_origins(6, 4, o0, o1))
    from rigidmultiblobswall_amd.msd import counts_per_lag
    assert np.array_equal(65 * vh.n_origins(6, 4, o0, o1), counts_per_lag(6, 65, 4, origins))
  # a reach below some displacements drops them from the counts, never from the moments
  Hs = vh.self_counts(frames, 4, 0, 6, 0.05, 10)
  M, terms = vh.moments(frames, 4, 0, 6)
  assert Hs[3].sum() < terms[3] and M[3, 0] > terms[3] * 0.05 ** 2 * 0.5


def test_fp64_numpy_meets_the_moment_bound():
  """the bound the GPU test demands is reachable: plain fp64 numpy against the long-double evaluation of the same inputs"""
  worst = 0.0
  for n, seed in ((65, 1), (130, 2), (257, 3)):
    frames = vh.random_walk(n, 6, BOX, 0.05, (1, 1, 0))(np.random.RandomState(seed))
    for plane in ("xyz", "xy"):
      M, terms = vh.moments(frames, 4, 0, 6, plane)
      M_ext, terms_ext = vh.moments(frames, 4, 0, 6, plane, vh.EXT)
      bound = vh.moment_bound(M_ext, terms_ext)
      assert np.array_equal(terms, terms_ext) and np.all(terms == n * vh.n_origins(6, 4, 0, 6))
      err = np.abs(M.astype(vh.EXT) - M_ext)
      assert np.all(err <= bound)
      worst = max(worst, float(np.max(err[1:] / bound[1:])))
  assert worst < 1.0


def test_c_entries_refuse_bad_arguments_without_a_device():
  """Every argument check comes before the context is looked at: with a null context each bad argument is named, and only
  a call whose arguments are in order is refused for the context."""
  from rigidmultiblobswall_amd import _lib
  lib, ARG = _lib.load(), -1      # RMB_ERR_ARG
  header = open(os.path.join(ROOT, "include", "rmb_mobility.h")).read()
  buf, L = np.zeros(3 * 2 * 3), np.array([4.0, 3.0, 0.0])
  hist, mom = np.zeros(2 * 16, dtype=np.uint64), np.zeros(4)
  p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
  good = dict(frames=p(buf), n_frames=3, n=2, L=p(L), n_lags=2, o_begin=0, o_end=2, plane=0, r_max=1.5, n_bins=16, hist=p(hist), mom=p(mom))
  bad = [(dict(hist=None), "null histogram"), (dict(n_frames=-1), "negative size"), (dict(n=-1), "negative size"),
         (dict(n_lags=0), "n_lags must be at least 1"), (dict(n_lags=-2), "n_lags must be at least 1"),
         (dict(o_end=4), "o_begin <= o_end <= n_frames"), (dict(o_begin=-1), "o_begin <= o_end <= n_frames"),
         (dict(o_begin=2, o_end=1), "o_begin <= o_end <= n_frames"), (dict(plane=2), "plane must be"), (dict(plane=-1), "plane must be"),
         (dict(r_max=0.0), "r_max must be positive and finite"), (dict(r_max=-1.0), "r_max must be positive and finite"),
         (dict(r_max=float("inf")), "r_max must be positive and finite"), (dict(r_max=float("nan")), "r_max must be positive and finite"),
         (dict(n_bins=0), "n_bins must be 1 ... 8192"), (dict(n_bins=8193), "n_bins must be 1 ... 8192"), (dict(frames=None), "null frames")]
  huge = dict(n_frames=2 ** 40, o_end=2 ** 40, n=2 ** 20)      # 2^28 tile pairs x 2^40 origins x 64 steps
  calls = {
      "rmb_van_hove_self_frames_device": (lambda a: (a["frames"], a["n_frames"], a["n"], a["n_lags"], a["o_begin"], a["o_end"], a["plane"],
                                                     a["r_max"], a["n_bins"], a["hist"], a["mom"]), bad + [(huge, "too many frames")]),
      "rmb_van_hove_distinct_frames_device": (lambda a: (a["frames"], a["n_frames"], a["n"], a["L"], a["n_lags"], a["o_begin"], a["o_end"],
                                                         a["plane"], a["r_max"], a["n_bins"], a["hist"]),
                                              bad + [(dict(L=None), "null periodic_length"), (huge, "too many frames"),
                                                     (dict(n_frames=2 ** 34, o_end=2 ** 34, n=2 ** 19), "too many pairs for one launch")]),
  }
  for name, (args, cases) in calls.items():
    assert name in _lib.SYMBOLS and ("int %s(" % name) in header
    fn = getattr(lib, name)
    for change, message in cases + [(dict(), "null context")]:
      rc = fn(None, *args(dict(good, **change)))
      assert rc == ARG, (name, change)
      assert message in lib.rmb_last_error().decode(), (name, change, lib.rmb_last_error())
  assert np.all(hist == 0) and np.all(mom == 0)


def test_python_argument_errors():
  L = (4.0, 3.0, 0.0)
  VH = vanhove.VanHove
  with pytest.raises(ValueError, match="n_lags"):
    VH(3, L, 0)
  with pytest.raises(ValueError, match="origins must be"):
    VH(3, L, 2, origins="every")
  with pytest.raises(ValueError, match="n_points"):
    VH(-1, L, 2)
  with pytest.raises(ValueError, match="three lengths"):
    VH(3, (4.0, 3.0), 2)
  with pytest.raises(ValueError, match="plane must be"):
    VH(3, L, 2, plane="xz")
  with pytest.raises(ValueError, match="positive period in the plane"):
    VH(3, (0.0, 0.0, 5.0), 2, plane="xy")
  with pytest.raises(ValueError, match="positive period in the plane"):
    VH(3, (0.0, 0.0, 0.0), 2)
  with pytest.raises(ValueError, match="r_max must be positive"):
    VH(3, L, 2, r_max=-1.0)
  with pytest.raises(ValueError, match="self_r_max must be positive"):
    VH(3, L, 2, self_r_max=float("inf"))
  with pytest.raises(ValueError, match="number of bins"):
    VH(3, L, 2, n_bins=8193)
  with pytest.raises(ValueError, match="number of bins"):
    VH(3, L, 2, self_n_bins=0)
  with pytest.raises(ValueError, match="single-GPU MobilityContext"):
    VH(3, L, 2, ctx=object())
  with pytest.raises(ValueError, match="normalisation must be"):
    vanhove.normalise_distinct(np.zeros((1, 4)), np.ones(1), 3, L, 1.0, "4d")
  with pytest.raises(ValueError, match="three positive periods"):
    vanhove.normalise_distinct(np.zeros((1, 4)), np.ones(1), 3, L, 1.0, "3d")
  with pytest.raises(ValueError, match="positive lx and ly"):
    vanhove.normalise_distinct(np.zeros((1, 4)), np.ones(1), 3, (4.0, 0.0, 2.0), 1.0, "pseudo2d")


def test_command_line_argument_errors(tmp_path, capsys):
  traj = tmp_path / "run.config"
  traj.write_text(phnp.config_text(np.zeros((3, 2, 3))))
  base = [str(traj), "2", "4.0", "3.0", "0.0"]
  cases = [(base, "--lags"), (base + ["--lags", "0"], "at least 1"), (base + ["--lags", "2", "--every", "0"], "at least 1"),
           (base + ["--lags", "2", "--plane", "xz"], "invalid choice"), (base + ["--lags", "2", "--origins", "some"], "invalid choice"),
           (base + ["--lags", "2", "--bins", "9000"], "1 ... 8192"), (base + ["--lags", "2", "--self-bins", "0"], "1 ... 8192"),
           (base + ["--lags", "2", "--rmax", "-1"], "--rmax must be positive"), (base + ["--lags", "2", "--self-rmax", "0"], "--self-rmax must be positive"),
           (base + ["--lags", "2"], "three positive periods"),      # plane xyz wants lz for G_d
           ([str(traj), "2", "0.0", "0.0", "0.0", "--lags", "2", "--no-distinct"], "--rmax is needed"),
           ([str(traj), "3", "4.0", "3.0", "0.0", "--lags", "2", "--plane", "xy"], "whole number of frames"),
           (base + ["--lags", "2", "--plane", "xy", "--skip", "3"], "no frame left")]
  for argv, message in cases:
    with pytest.raises(SystemExit) as exc:
      vanhove.main(argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err, argv


def test_normalisations_on_hand_made_counts():
  # self: 10 terms of lag 0 in bin 0, 10 terms of lag 1 spread over two of four bins up to 2.0
  Hs = np.array([[10, 0, 0, 0], [0, 4, 6, 0], [0, 0, 0, 0]])
  counts = np.array([10, 10, 0])
  for plane in ("xyz", "xy"):
    shell = vanhove.shell_volumes(2.0, 4, plane)
    e = 0.5 * np.arange(5)
    want = 4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3) if plane == "xyz" else np.pi * (e[1:] ** 2 - e[:-1] ** 2)
    assert np.allclose(shell, want, rtol=1e-15)
    Gs = vanhove.normalise_self(Hs, counts, 2.0, plane)
    assert np.allclose((Gs[:2] * shell).sum(axis=1), 1.0, rtol=1e-15) and np.all(np.isnan(Gs[2]))
    assert np.isclose(Gs[1, 2], 0.6 / shell[2], rtol=1e-15)
  # distinct: an ideal gas has G_d = 1 -- counts = n_origins N rho shell
  N, L, n_or = 50, np.array([4.0, 5.0, 2.0]), np.array([3, 2, 0])
  for form, rho, plane in (("3d", N / 40.0, "xyz"), ("2d", N / 20.0, "xy"), ("pseudo2d", N / 20.0, "xy")):
    shell = vanhove.shell_volumes(2.0, 4, plane)
    Hd = n_or[:, None] * N * rho * shell[None, :]
    Gd = vanhove.normalise_distinct(Hd, n_or, N, L, 2.0, form)
    assert np.allclose(Gd[:2], 1.0, rtol=1e-14) and np.all(np.isnan(Gd[2]))
  # at lag 0 "pseudo2d" is correlation.normalise on half the (ordered) counts, bit for bit
  from rigidmultiblobswall_amd import correlation
  Hd = np.array([[0, 12, 30, 44]])
  assert np.array_equal(vanhove.normalise_distinct(Hd, [3], N, L, 2.0, "pseudo2d")[0], correlation.normalise(Hd[0] // 2, 3, N, L, 2.0, "pseudo2d"))
  # moments
  msd, a2 = vanhove.alpha2_from_moments(np.array([[0.0, 0.0], [8.0, 40.0], [0.0, 0.0]]), np.array([4, 4, 0]), "xyz")
  assert msd[0] == 0.0 and np.isnan(a2[0]) and msd[1] == 2.0 and np.isclose(a2[1], 0.6 * 10.0 / 4.0 - 1.0) and np.isnan(msd[2]) and np.isnan(a2[2])
  assert np.isclose(vanhove.alpha2_from_moments(np.array([[8.0, 40.0]]), np.array([4]), "xy")[1][0], 0.5 * 10.0 / 4.0 - 1.0)


def test_table_round_trip(tmp_path):
  rng = np.random.RandomState(2)
  times, n_or = 0.25 * np.arange(3), np.array([4, 3, 0])
  a2, msd = np.array([np.nan, 0.125, np.nan]), np.array([0.0, 0.3, np.nan])
  r, Hs, Hd = 0.1 * (np.arange(5) + 0.5), rng.randint(0, 2 ** 40, (3, 5)), rng.randint(0, 2 ** 40, (3, 5))
  Gs, Gd = rng.uniform(0, 3, (3, 5)), rng.uniform(0, 3, (3, 5))
  r2, Hd2, Gd2 = 0.3 * (np.arange(2) + 0.5), Hd[:, :2], Gd[:, :2]
  for kw in (dict(r=r, Gd=Gd, Hd=Hd), dict(r=r2, Gd=Gd2, Hd=Hd2), dict()):
    path = tmp_path / "table.dat"
    path.write_text(vanhove.format_table(times, n_or, a2, msd, r, Gs, Hs, **kw))
    blocks = vanhove.parse(path.read_text())
    assert len(blocks) == 3
    for l, b in enumerate(blocks):
      assert b["t"] == times[l] and b["n_origins"] == n_or[l]
      assert np.array_equal([b["alpha2"], b["msd"]], [a2[l], msd[l]], equal_nan=True)
      assert np.array_equal(b["r_self"], r) and np.array_equal(b["Gs"], Gs[l]) and np.array_equal(b["Hs"], Hs[l])
      if kw:
        assert np.array_equal(b["r"], kw["r"]) and np.array_equal(b["Gd"], kw["Gd"][l]) and np.array_equal(b["Hd"], kw["Hd"][l])
      else:
        assert "Gd" not in b
  with pytest.raises(ValueError, match="not a van Hove table"):
    vanhove.parse("1 2 3\n")
