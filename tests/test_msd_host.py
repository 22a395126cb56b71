"""Host side of the mean-square displacement: the numpy restatement (tests/_msd_numpy.py, the reference's rotation-matrix
form) against the reference's recorded output (tests/golden/g18_msd_reference.npz, tools/gen_golden_msd.py), the frame
selection, a closed form, the error bound of the GPU tests checked on the fp64 restatement itself, and the argument checks of
the C entries and of rigidmultiblobswall_amd.msd.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import _msd_numpy as mnp
from conftest import GOLDEN, ROOT, load_golden
from rigidmultiblobswall_amd import msd

CASES = ("plain", "interval", "tracked")


@pytest.fixture(scope="module")
def golden():
  return load_golden(os.path.join(GOLDEN, "g18_msd_reference.npz"))


def _case(g, name):
  keys = ("locations", "orientations", "dt", "end", "burn_in", "trajectory_length", "offset", "has_offset", "msd", "n_kept", "n_origins")
  c = {k: g["%s_%s" % (name, k)] for k in keys}
  c["offset"] = c["offset"] if bool(c["has_offset"]) else None
  for k in ("burn_in", "trajectory_length", "n_kept", "n_origins"):
    c[k] = int(c[k])
  c["dt"], c["end"] = float(c["dt"]), float(c["end"])
  return c


def test_golden_covers_the_cases(golden):
  assert list(golden["cases"]) == list(CASES)
  cs = [_case(golden, n) for n in CASES]
  assert all(c["locations"].shape == (400, 3) and c["orientations"].shape == (400, 4) for c in cs)
  assert [c["burn_in"] for c in cs] == [0, 7, 25] and [c["offset"] is not None for c in cs] == [False, False, True]
  assert os.path.getsize(os.path.join(GOLDEN, "g18_msd_reference.npz")) < 200 * 1024


@pytest.mark.parametrize("name", CASES)
def test_selection_reproduces_the_reference_counts(golden, name):
  c = _case(golden, name)
  kept, interval, origins, divisor = msd.reference_selection(400, c["dt"], c["end"], c["burn_in"], c["trajectory_length"])
  assert len(kept) == c["n_kept"] and len(origins) == c["n_origins"]
  assert interval == {"plain": 1, "interval": 3, "tracked": 2}[name]
  assert origins[0] == 1 and origins[-1] == len(kept) - c["trajectory_length"]
  assert kept[0] > c["burn_in"] and np.all(kept % interval == 0)
  assert divisor == 400 / interval - c["trajectory_length"] - c["burn_in"] / interval
  if name == "interval":
    assert len(kept) == 131


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(golden, name):
  c = _case(golden, name)
  kept, _, origins, divisor = msd.reference_selection(400, c["dt"], c["end"], c["burn_in"], c["trajectory_length"])
  frames = np.concatenate([c["locations"], c["orientations"]], axis=1)[kept[1:]][:, None, :]
  S, n = mnp.sums(frames, c["trajectory_length"], offsets=c["offset"], origins="window")
  assert np.all(n == len(origins))
  assert c["msd"].shape == (c["trajectory_length"], 6, 6)
  assert np.abs(S / divisor - c["msd"]).max() <= 1e-13 * np.abs(c["msd"]).max()


def test_selection_refuses_a_run_that_is_too_short():
  with pytest.raises(ValueError, match="Trajectory length is longer"):
    msd.reference_selection(50, 0.1, 10.0, 0, 30)      # data_interval 4: 120 steps needed


@pytest.mark.parametrize("origins", ["window", "all"])
def test_closed_form(origins):
  """constant velocity and constant angular velocity about a fixed axis: Delta = [v l tau; sin(w l tau) n] exactly"""
  F, N, L = 40, 5, 17
  frames, exact = mnp.screw_motion(F, N, seed=3)
  S, n = mnp.sums(frames, L, origins=origins)
  for lag in range(L):
    D = exact(lag)
    want = n[lag] // N * np.einsum("bi,bj->ij", D, D)
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    assert np.all(np.abs(S[lag] - want) <= 1e-13 * scale), lag
  assert np.array_equal(n, msd.counts_per_lag(F, N, L, origins))
  assert n[0] == N * (F - L + 1 if origins == "window" else F)


def test_sign_of_a_quaternion_does_not_matter():
  frames = mnp.random_walk(30, 4, seed=8)
  flipped = frames.copy()
  flip = np.random.RandomState(9).rand(30, 4) < 0.5
  flipped[..., 3:][flip] *= -1.0
  assert flip.any() and not flip.all()
  for origins in ("window", "all"):
    a, b = mnp.sums(frames, 9, offsets=(0.2, 0.1, -0.3), origins=origins)[0], mnp.sums(flipped, 9, offsets=(0.2, 0.1, -0.3), origins=origins)[0]
    assert np.array_equal(a, b)      # R(q) is even in q, term by term


CASES_BOUND = [(65, 3, 300, "window", True), (130, 1, 131, "all", False), (7, 65, 5, "all", True), (64, 3, 64, "window", False)]


@pytest.mark.parametrize("n_lags, N, F, origins, off", CASES_BOUND)
def test_the_bound_of_the_gpu_tests_is_reachable_in_double(n_lags, N, F, origins, off):
  """The fp64 restatement against the long-double one, under the bound the kernel is held to (mnp.bound; test_gpu_msd.py
  derives its constants): a bound plain double arithmetic could not meet would say nothing about the kernel."""
  frames = mnp.random_walk(F, N, seed=100 + n_lags)
  offsets = np.random.RandomState(5).uniform(-0.5, 0.5, (N, 3)) if off else None
  assert np.abs(np.sum(frames[..., 3:].astype(np.longdouble) ** 2, axis=-1) - 1).max() <= 8 * mnp.U      # the bound's precondition
  S_ld, n, A, B = mnp.sums(frames, n_lags, offsets=offsets, origins=origins, dtype=np.longdouble, absolute=True)
  S, n64 = mnp.sums(frames, n_lags, offsets=offsets, origins=origins)
  assert np.array_equal(n, n64) and np.array_equal(n, msd.counts_per_lag(F, N, n_lags, origins))
  tol = mnp.bound(frames, offsets, n, A, B)
  err = np.abs(S.astype(np.longdouble) - S_ld).astype(np.float64)
  print("max err / bound = %.3f" % np.max(err[tol > 0] / tol[tol > 0]))
  assert np.all(err <= tol)
  assert np.all(S[n == 0] == 0) and np.all(S[0, :3] == 0)      # lag 0: no translation, and R e_i x R e_i = 0 exactly


def test_counts_per_lag():
  assert np.array_equal(msd.counts_per_lag(10, 3, 4, "window"), [21, 21, 21, 21])
  assert np.array_equal(msd.counts_per_lag(10, 3, 4, "all"), [30, 27, 24, 21])
  assert np.array_equal(msd.counts_per_lag(3, 2, 5, "window"), [0] * 5)
  assert np.array_equal(msd.counts_per_lag(3, 2, 5, "all"), [6, 4, 2, 0, 0])
  with pytest.raises(ValueError, match="n_lags"):
    msd.counts_per_lag(3, 2, 0)
  with pytest.raises(ValueError, match="origins must be"):
    msd.counts_per_lag(3, 2, 1, "some")


def test_load_trajectory_round_trip(tmp_path):
  frames = mnp.random_walk(4, 3, seed=2)
  p = tmp_path / "run.config"
  p.write_text(mnp.config_text(frames))
  assert np.array_equal(msd.load_trajectory(str(p), 3), frames)
  assert np.array_equal(msd.load_trajectory([p, p], 3, skip=5), frames[1:])
  with pytest.raises(ValueError, match="whole number of frames"):
    msd.load_trajectory(str(p), 2)
  with pytest.raises(ValueError, match="no frame left"):
    msd.load_trajectory(str(p), 3, skip=4)
  with pytest.raises(ValueError, match="skip"):
    msd.load_trajectory(str(p), 3, skip=-1)


def test_format_round_trip():
  m = np.random.RandomState(1).randn(3, 6, 6)
  m = m + m.transpose(0, 2, 1)
  t, n, tri = mnp.parse_msd(msd.format_msd([0.0, 0.5, 1.0], [7, 6, 5], m))
  assert np.array_equal(t, [0.0, 0.5, 1.0]) and np.array_equal(n, [7, 6, 5])
  assert tri.shape == (3, 21) and np.array_equal(tri, m[:, msd.TRIU[0], msd.TRIU[1]])


def test_c_entries_refuse_bad_arguments_without_a_device():
  """Every argument check comes before the context is looked at: with a null context each bad argument is named, and only
  a call whose arguments are in order is refused for the context."""
  from rigidmultiblobswall_amd import _lib
  lib, ARG = _lib.load(), -1      # RMB_ERR_ARG
  header = open(os.path.join(ROOT, "include", "rmb_mobility.h")).read()
  buf = np.zeros(7 * 6)
  sums = np.zeros(2 * 36)
  f, s = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(sums.ctypes.data)
  good = dict(frames=f, n_frames=3, n_bodies=2, offsets=None, n_lags=2, o_begin=0, o_end=2, origin_chunk=0, sums=s)
  bad = [(dict(sums=None), "null sums"), (dict(n_frames=-1), "negative size"), (dict(n_bodies=-1), "negative size"),
         (dict(n_lags=0), "n_lags must be at least 1"), (dict(n_lags=-3), "n_lags must be at least 1"),
         (dict(o_end=4), "o_begin <= o_end <= n_frames"), (dict(o_begin=-1), "o_begin <= o_end <= n_frames"),
         (dict(o_begin=2, o_end=1), "o_begin <= o_end <= n_frames"), (dict(origin_chunk=-1), "origin_chunk"),
         (dict(frames=None), "null frames"), (dict(), "null context")]
  for name in ("rmb_msd_frames", "rmb_msd_frames_device"):
    assert name in _lib.SYMBOLS and ("int %s(" % name) in header
    fn = getattr(lib, name)
    for change, message in bad:
      a = dict(good, **change)
      rc = fn(None, a["frames"], a["n_frames"], a["n_bodies"], a["offsets"], a["n_lags"], a["o_begin"], a["o_end"], a["origin_chunk"], a["sums"])
      assert rc == ARG, (name, change)
      assert message in lib.rmb_last_error().decode(), (name, change, lib.rmb_last_error())
  assert np.all(sums == 0)


def test_python_argument_errors():
  with pytest.raises(ValueError, match="n_lags"):
    msd.MeanSquareDisplacement(3, 0)
  with pytest.raises(ValueError, match="origins must be"):
    msd.MeanSquareDisplacement(3, 4, origins="every")
  with pytest.raises(ValueError, match="offsets"):
    msd.MeanSquareDisplacement(3, 4, offsets=[1.0, 2.0])
  with pytest.raises(ValueError, match="n_bodies"):
    msd.MeanSquareDisplacement(-1, 4)
  with pytest.raises(ValueError, match="one row per step"):
    msd.reference_msd(np.zeros((5, 3)), np.zeros((4, 4)), 0.1, 1.0)
