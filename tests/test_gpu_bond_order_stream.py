"""rigidmultiblobswall_amd.bondorder.BondOrder on the GPU: a trajectory fed in pieces, C_m against a numpy lag loop, and g_6(r) of
a thermal triangular lattice and of an ideal gas.

Pieces: counts, sums and the neighbour distribution are integers, psi comes from one fixed chunk plan per frame, the means are
integer sums of rint(. 2^30) and the lag sweep runs in blocks of ORIGIN_BLOCK origins counted from the first frame -- so EVERY
result has the same bits however the trajectory is cut.
C_m: the lag sums of the psi the GPU produced (taken as exact fp64 inputs) against the same sums in long double, under the bound
test_gpu_scattering.py uses for the collective lag sums, u (n_o + 3) A per series, plus u (n - 1) A for the sum over the n series
(A = sum of the terms' absolute values): u (n_o + n + 2) A."""
import io

import numpy as np
import pytest
import torch

import _bond_order_numpy as bo
import _pair_hist_numpy as phnp
from rigidmultiblobswall_amd import bondorder

pytestmark = pytest.mark.gpu

BOX = np.array([7.0, 5.0, 0.0])
R_CUT, R_MAX, N_BINS = 1.1, 2.4, 48


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _walk(n, F, step, seed):
  """a random walk in the periodic box (unwrapped), every frame off the cutoff and the bin edges"""
  def make(rng):
    return rng.uniform(0, 1, (1, n, 3)) * np.array([7.0, 5.0, 0.5]) + np.cumsum(step * rng.randn(F, n, 3), axis=0)
  return bo.frames_with_margin(make, BOX, R_CUT, "xy", R_MAX, N_BINS, seed=seed)


@pytest.mark.parametrize("origins", ["window", "all"])
def test_pieces_give_identical_results(ctx, origins, monkeypatch):
  monkeypatch.setattr(bondorder, "ORIGIN_BLOCK", 2)      # several blocks of origins in 9 frames
  n, F, n_lags, orders = 65, 9, 3, (4, 6)
  frames = _walk(n, F, 0.05, 40)
  kw = dict(orders=orders, r_cut=R_CUT, r_max=R_MAX, n_bins=N_BINS, n_lags=n_lags, dt=0.5, origins=origins, ctx=ctx)
  runs = []
  for size in (1, 3, F):
    acc = bondorder.BondOrder(n, BOX, **kw)
    for k in range(0, F, size):
      piece = frames[k:k + size]
      acc.add_frames(piece if (k // size) % 2 else torch.from_numpy(piece.copy()).cuda())      # numpy and device pieces
    runs.append(acc.finish())
  one = runs[-1]
  # against the restatement: integers exactly, psi within the bound
  N, S, ratio = bo.neighbour_sums(frames, BOX, R_CUT, orders, "xy")
  assert np.array_equal(one.neighbour_counts(), np.bincount(N.reshape(-1)))
  psi_ext = S[-1] / np.maximum(N[-1], 1)[:, None, None]
  err = np.abs(np.stack([one.psi_last().real, one.psi_last().imag], axis=-1).astype(bo.EXT) - psi_ext).max(axis=-1).astype(np.float64)
  assert np.all(err <= bo.sum_bound(N[-1], ratio[-1], orders) / np.maximum(N[-1], 1)[:, None] + bo.U)
  psi = bo.psi_of(N, S)      # (F, n, K), fp64-rounded long-double values
  for k in range(len(orders)):
    counts, sums = bo.pair_field(frames, bondorder.quantise(psi[:, :, k]), BOX, R_MAX, N_BINS, "xy")
    assert np.array_equal(one.pair_counts()[k], counts)
    # psi on the GPU differs from the restatement's in the last bits: where that moves a rounded component by a unit, the term
    # moves by at most one unit per component, and one more for the shift
    assert np.all(np.abs(one.pair_sums()[k] - sums) <= 5 * counts)
  n_or = np.array([F - n_lags + 1] * n_lags) if origins == "window" else F - np.arange(n_lags)
  assert np.array_equal(one.n_origins(), n_or) and one.n_frames == F
  for acc in runs[:-1]:
    assert np.array_equal(acc.pair_counts(), one.pair_counts()) and np.array_equal(acc.pair_sums(), one.pair_sums())
    assert np.array_equal(acc.neighbour_counts(), one.neighbour_counts()) and np.array_equal(acc.n_origins(), one.n_origins())
    for a, b in ((acc.psi_last().view(np.float64), one.psi_last().view(np.float64)), (acc.lag_sums(), one.lag_sums()),
                 (acc.mean_abs_psi(), one.mean_abs_psi()), (acc.global_order(), one.global_order()), (acc.C_n()[1], one.C_n()[1])):
      assert np.array_equal(a.view(np.int64), b.view(np.int64))
  # the means against numpy on the restatement's psi: sums of rint(. 2^30) -- a frame's mean field is within sqrt(2) 2^-31 of the
  # unquantised one, the rounding of its modulus adds 2^-31, psi's own error is ~1e-15: inside 2^-29
  tol = 2.0 ** -29
  assert np.all(np.abs(one.mean_abs_psi() - np.abs(psi).mean(axis=(0, 1))) <= tol)
  assert np.all(np.abs(one.global_order() - np.abs(psi.mean(axis=1)).mean(axis=0)) <= tol)
  assert np.array_equal(one.C_n()[0], 0.5 * np.arange(n_lags)) and np.all(one.C_n()[1][:, 0] == 1.0)
  with pytest.raises(ValueError, match="after finish"):
    one.add_frames(frames[:1])
  for acc in runs:
    acc.close()
  assert ctx._h.value      # a caller's context stays open


@pytest.mark.parametrize("origins", ["window", "all"])
def test_time_correlation_against_a_numpy_lag_loop(ctx, origins):
  n, F, n_lags, orders = 130, 12, 5, (6, 12)
  frames = _walk(n, F, 0.03, 60)
  acc = bondorder.BondOrder(n, BOX, orders=orders, r_cut=R_CUT, n_lags=n_lags, origins=origins, ctx=ctx)
  acc.add_frames(frames[:5]).add_frames(frames[5:]).finish()
  out = ctx.bond_order_frames_device(torch.from_numpy(frames).cuda(), BOX, R_CUT, orders, source_chunk=bondorder.SOURCE_CHUNK).cpu().numpy()
  psi = bo.psi_of(out[..., 0], out[..., 1:].reshape(F, n, 2, 2))      # the GPU's psi: the inputs of the lag sums
  assert np.array_equal(acc.psi_last().view(np.float64), psi[-1].view(np.float64))
  C, A, n_or = bo.lag_sums(psi, n_lags, origins)
  assert np.array_equal(acc.n_origins(), n_or)
  bound = bo.U * (n_or[None, :] + n + 2.0) * A.astype(np.float64)
  err = np.abs(acc.lag_sums().astype(bo.EXT) - C).astype(np.float64)
  assert np.all(err <= bound), (err / bound).max()
  print("C_n %s: max err / bound = %.3f" % (origins, (err / bound).max()))
  per = (C / n_or[None, :]).astype(np.float64)
  assert np.allclose(acc.C_n()[1], per / per[:, :1], rtol=1e-12, atol=0)
  acc.close()


def test_thermal_triangular_lattice_is_ordered(ctx):
  """small thermal noise on a periodic triangular lattice: g_6(r) > 0.9 at every populated bin"""
  pts, L = bo.triangular_lattice(24, 24, 1.0)
  rng = np.random.RandomState(7)
  frames = pts[None] + 0.01 * rng.randn(3, pts.shape[0], 3) * np.array([1.0, 1.0, 0.0])
  acc = bondorder.BondOrder(pts.shape[0], L, orders=(6,), r_cut=1.35, r_max=8.0, n_bins=64, ctx=ctx).add_frames(frames).finish()
  r, g, counts = acc.g_n()
  assert counts.sum() > 0 and (counts == 0).any()      # a lattice: shells, and gaps between them
  assert np.all(g[0][counts > 0] > 0.9) and np.all(np.isnan(g[0][counts == 0]))
  assert acc.mean_abs_psi()[0] > 0.9 and acc.global_order()[0] > 0.9 and acc.neighbour_counts().tolist() == [0] * 6 + [3 * 576]
  acc.close()


def test_ideal_gas_has_no_orientational_correlation(ctx):
  """4096 independent points: |g_6(r)| <= 6 / sqrt(counts) in every bin beyond r_cut (below it a pair shares a bond: not asserted).
  The seed was checked against the CPU restatement first."""
  n, L = 4096, np.array([64.0, 64.0, 0.0])
  frame = np.random.RandomState(2028).uniform(0, 1, (1, n, 3)) * np.array([64.0, 64.0, 0.0])
  acc = bondorder.BondOrder(n, L, orders=(6,), r_cut=1.5, r_max=8.0, n_bins=16, ctx=ctx).add_frames(frame).finish()
  r, g, counts = acc.g_n()
  far = r - 0.25 >= 1.5      # bins that lie wholly beyond the cutoff
  assert far.sum() == 13 and np.all(counts[far] > 1000)
  assert np.all(np.abs(g[0][far]) <= 6.0 / np.sqrt(counts[far])), (g[0], counts)
  assert acc.global_order()[0] < 0.05 and 0.2 < acc.mean_abs_psi()[0] < 0.7
  acc.close()


def test_command_line(ctx, tmp_path):
  n, L = 30, np.array([7.0, 5.0, 0.0])
  used = _walk(n, 4, 0.05, 80)      # the frames --skip 1 --every 2 keeps
  frames = np.random.RandomState(0).uniform(0, 1, (9, n, 3)) * np.array([7.0, 5.0, 0.5])
  frames[1::2] = used
  traj = tmp_path / "run.config"
  traj.write_text(phnp.config_text(frames))
  argv = [str(traj), str(n), "7.0", "5.0", "0", "--orders", "4,6", "--rcut", str(R_CUT), "--rmax", str(R_MAX), "--bins", str(N_BINS), "--lags", "3",
          "--dt", "0.5", "--skip", "1", "--every", "2", "--origins", "all"]
  buf = io.StringIO()      # the module's main(), which `python -m rigidmultiblobswall_amd.bondorder` runs
  assert bondorder.main(argv, out=buf) == 0
  d = bondorder.parse(buf.getvalue())
  acc = bondorder.BondOrder(n, L, orders=(4, 6), r_cut=R_CUT, r_max=R_MAX, n_bins=N_BINS, n_lags=3, dt=1.0, origins="all", ctx=ctx)
  acc.add_frames(used).finish()
  assert d["orders"] == (4, 6) and d["n_frames"] == 4 and d["n_points"] == n and d["plane"] == "xy" and d["r_cut"] == R_CUT
  assert np.array_equal(d["neighbours"], acc.neighbour_counts()) and np.array_equal(d["mean_abs_psi"], acc.mean_abs_psi())
  assert np.array_equal(d["global_order"], acc.global_order())
  assert np.array_equal(d["counts"], acc.g_n()[2]) and np.array_equal(d["g"], acc.g_n()[1], equal_nan=True) and np.array_equal(d["r"], acc.r())
  assert np.array_equal(d["t"], [0.0, 1.0, 2.0]) and d["n_origins"].tolist() == [4, 3, 2] and np.array_equal(d["C"], acc.C_n()[1])
  N = bo.neighbour_sums(used, L, R_CUT, (4,), "xy")[0]
  assert np.array_equal(d["neighbours"], np.bincount(N.reshape(-1)))
  acc.close()
