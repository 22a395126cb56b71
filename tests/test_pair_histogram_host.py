"""Host side of the radial distribution function: the numpy restatement of the pair-distance histogram against the reference
program's recorded output (tests/golden/g17_gr_*.npz, tools/gen_golden_pair_histogram.py), the trajectory reader, the
normalisations and the argument checks of rigidmultiblobswall_amd.correlation.  No GPU."""
import os

import numpy as np
import pytest

import _pair_hist_numpy as phnp
from conftest import golden_files, load_golden
from rigidmultiblobswall_amd import correlation

GOLDENS = golden_files("g17_gr_*.npz")


def _golden(path):
  d = load_golden(path)
  L = d["periodic_length"]
  return d["frames"], int(d["n_points"]), L, 0.5 * L[0], int(d["n_bins"]), phnp.parse_gr(str(d["output"]))


def test_goldens_present():
  assert sorted(os.path.basename(p) for p in GOLDENS) == ["g17_gr_quasi2d.npz", "g17_gr_shifted.npz"]


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[7:-4] for p in GOLDENS])
def test_restatement_equals_reference_program(path):
  frames, n, L, r_max, n_bins, (r, g, hist) = _golden(path)
  assert frames.shape == (4, 150, 3) and n_bins == 2000 and len(r) == n_bins
  assert phnp.edge_margin(frames, L, r_max, n_bins) > phnp.MARGIN      # the precondition of exact equality
  c = phnp.counts(frames, L, r_max, n_bins)
  assert np.array_equal(2 * c.astype(np.int64), hist)
  assert hist.sum() > 50000
  # the program prints 6 significant digits: a rounding error of at most 5e-6 relative
  g_mine = phnp.g_pseudo2d(c, frames.shape[0], n, L[0], L[1], r_max)
  assert np.all(np.abs(g_mine - g) <= 1e-5 * np.abs(g))
  assert np.all(np.abs((np.arange(n_bins) + 0.5) * (r_max / n_bins) - r) <= 1e-5 * r)
  # and the package's normalisation is the same statement
  g_pkg = correlation.normalise(c, frames.shape[0], n, L, r_max, "pseudo2d")
  assert np.all(np.abs(g_pkg - g) <= 1e-5 * np.abs(g))


def test_shifted_golden_has_points_outside_the_primary_cell():
  frames, n, L, r_max, n_bins, _ = _golden([p for p in GOLDENS if "shifted" in p][0])
  assert frames[:, :, 0].min() < -L[0] and frames[:, :, 0].max() > 2 * L[0]
  assert frames[:, :, 1].min() < -L[1] and frames[:, :, 1].max() > 2 * L[1]


def test_format_is_the_programs():
  frames, n, L, r_max, n_bins, (r, g, hist) = _golden(GOLDENS[0])
  c = phnp.counts(frames, L, r_max, n_bins)
  rd_r = (np.arange(n_bins) + 0.5) * (r_max / n_bins)
  text = correlation.format_gr(rd_r, correlation.normalise(c, 4, n, L, r_max), c)
  r2, g2, h2 = phnp.parse_gr(text)
  assert np.array_equal(h2, hist)
  assert np.all(np.abs(g2 - g) <= 1e-5 * np.abs(g)) and np.all(np.abs(r2 - r) <= 1e-5 * r)
  assert text.splitlines()[0] == "0.005 0 0"
  # a count above 10^6 keeps every digit in the third column
  assert correlation.format_gr([0.5], [1.0], [1234567]) == "0.5 1 2469134\n"


@pytest.mark.parametrize("final_newline", [True, False])
def test_read_frames_config_round_trip(tmp_path, final_newline):
  rng = np.random.RandomState(5)
  frames = rng.uniform(-50, 50, (3, 7, 3))
  p = tmp_path / "run.config"
  p.write_text(phnp.config_text(frames, final_newline=final_newline))
  got = correlation.read_frames(str(p), 7)
  assert got.shape == (3, 7, 3) and np.array_equal(got, frames)
  assert np.array_equal(correlation.read_frames(p, 7), frames)      # a path object too
  assert np.array_equal(correlation.load_trajectory(str(p), 7, skip=2), frames[2:])


def test_read_frames_clones_list(tmp_path):
  rng = np.random.RandomState(6)
  frames = rng.uniform(-5, 5, (4, 5, 3))
  paths = []
  for k, frame in enumerate(frames):
    p = tmp_path / ("run.shell.%08d.clones" % k)
    p.write_text(phnp.config_text(frame[None]))
    paths.append(str(p))
  assert np.array_equal(correlation.read_frames(paths, 5), frames)
  assert correlation.read_frames([], 5).shape == (0, 5, 3)


def test_read_frames_errors(tmp_path):
  p = tmp_path / "run.config"
  p.write_text(phnp.config_text(np.zeros((2, 4, 3))))
  with pytest.raises(ValueError, match="whole number of frames"):
    correlation.read_frames(str(p), 5)
  q = tmp_path / "other.config"
  q.write_text(phnp.config_text(np.zeros((8, 3, 3))))      # 8 * 22 numbers: also a whole number of 8-number blocks
  with pytest.raises(ValueError, match="announces 3 bodies"):
    correlation.read_frames(str(q), 1)
  with pytest.raises(ValueError, match="skip"):
    correlation.load_trajectory(str(p), 4, skip=-1)
  with pytest.raises(ValueError, match="no frame left"):
    correlation.load_trajectory(str(p), 4, skip=2)


def _ideal_counts(n_frames, n, L, r_max, n_bins, dim):
  e = (r_max / n_bins) * np.arange(n_bins + 1)
  if dim == 2:
    shell, rho = np.pi * (e[1:] ** 2 - e[:-1] ** 2), n / (L[0] * L[1])
  else:
    shell, rho = 4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3), n / (L[0] * L[1] * L[2])
  return 0.5 * n_frames * n * rho * shell      # unordered pairs


def test_normalisations_closed_forms():
  """an ideal gas' expected counts give g = 1 in every bin, under either normalisation; --skip K normalises by F - K"""
  n, L, r_max, n_bins, F, K = 1875, np.array([40.0, 16.0, 9.0]), 7.5, 300, 11, 4
  for dim, name in ((2, "pseudo2d"), (3, "3d")):
    c = _ideal_counts(F - K, n, L, r_max, n_bins, dim)
    assert np.allclose(correlation.normalise(c, F - K, n, L, r_max, name), 1.0, rtol=1e-13, atol=0)
    assert np.allclose(correlation.normalise(c, F, n, L, r_max, name), (F - K) / F, rtol=1e-13, atol=0)
  # the two differ by the ratio of shell volume per height to ring area: (4/3)(r_up^3 - r_low^3) / ((r_up^2 - r_low^2) lz)
  c = _ideal_counts(1, n, L, r_max, n_bins, 3)
  e = (r_max / n_bins) * np.arange(n_bins + 1)
  ratio = 4.0 / 3.0 * (e[1:] ** 3 - e[:-1] ** 3) / ((e[1:] ** 2 - e[:-1] ** 2) * L[2])
  assert np.allclose(correlation.normalise(c, 1, n, L, r_max, "pseudo2d"), ratio, rtol=1e-13, atol=0)


def test_argument_errors():
  L2, L3 = (40.0, 16.0, 0.0), (40.0, 16.0, 9.0)
  with pytest.raises(ValueError, match="three positive periods"):
    correlation.RadialDistribution(10, L2, normalisation="3d")
  with pytest.raises(ValueError, match="positive lx and ly"):
    correlation.RadialDistribution(10, (40.0, 0.0, 0.0), r_max=3.0)
  with pytest.raises(ValueError, match="normalisation must be"):
    correlation.RadialDistribution(10, L3, normalisation="2d")
  with pytest.raises(ValueError, match="r_max must be positive"):
    correlation.RadialDistribution(10, (0.0, 16.0, 0.0))      # r_max=None needs lx
  with pytest.raises(ValueError, match="r_max must be positive"):
    correlation.RadialDistribution(10, L2, r_max=0.0)
  for bins in (0, 8193):
    with pytest.raises(ValueError, match="n_bins must be"):
      correlation.RadialDistribution(10, L2, n_bins=bins)
  with pytest.raises(ValueError, match="n_points"):
    correlation.RadialDistribution(-1, L2)
  with pytest.raises(ValueError):
    correlation.normalise(np.zeros(4), 1, 10, L2, 1.0, "3d")


def test_restatement_properties():
  """the restatement itself: total count without reach limit, coincident points in bin 0, images of whole periods"""
  rng = np.random.RandomState(2)
  x = rng.uniform(0, 3, (40, 3))
  assert phnp.counts(x, (0, 0, 0), 100.0, 7).sum() == 40 * 39 // 2
  y = np.concatenate([x, np.tile(x[:1], (4, 1))])      # 5 coincident points: 10 pairs at r = 0
  assert phnp.counts(y, (0, 0, 0), 1e-9, 3)[0] == 10
  L = (3.0, 3.0, 0.0)
  shifted = x + np.array([6.0, -9.0, 0.0]) * rng.randint(0, 2, (40, 1))
  a, b = phnp.counts(x, L, 1.5, 5), phnp.counts(shifted, L, 1.5, 5)
  assert np.array_equal(a, b)
