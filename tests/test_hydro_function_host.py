"""Host-side tests of the hydrodynamic function: the bound of tests/_hydro_function_numpy.py is reachable (plain fp64 numpy
meets it on every shape the GPU test uses), the polarisation helpers, the refusals of the Python layer, the command line's
parsing and the write / shells round trip on synthetic sums.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hydro_function_numpy as hn  # noqa: E402
from _mobility_numpy import EXT, LONG_DOUBLE  # noqa: E402

from rigidmultiblobswall_amd import hydrofunction as hf  # noqa: E402
from rigidmultiblobswall_amd.context import MobilityContext  # noqa: E402

KC = 8
N_LIST = (1, 2, 63, 64, 65, 129, 200)
K_LIST = (1, KC, KC + 1, 2 * KC + 3)


# ---- the bound is reachable ------------------------------------------------------------------------------------------
@pytest.mark.skipif(not LONG_DOUBLE, reason="needs an 80-bit long double as the reference")
@pytest.mark.parametrize("case,shift", [(c, 0.0) for c in hn.CASES] + [("wall_periodic", 1000.0)])
def test_fp64_numpy_meets_the_bound(case, shift):
  ref = hn.reference(case, shift)
  assert hn.K_MAX == K_LIST[-1] and hn.N_FRAMES == 3 and ref["frames"].shape[1] == N_LIST[-1]
  plain = [hn.terms(fr, hn.A, hn.ETA, ref["boundary"], ref["mob_L"], ref["L"], ref["kint"], ref["pol"], dtype=np.float64) for fr in ref["frames"]]
  worst = 0.0
  for n in N_LIST:
    for K in K_LIST:
      S, B = hn.expected(ref, n, K, 3)
      got = np.zeros((3, K, 2))
      for f, (st, pt) in enumerate(plain):
        got[f, :, 0] = st[:n, :K].sum(axis=0)
        got[f, :, 1] = pt[:n, :n, :K].sum(axis=(0, 1))
      assert np.all(B > 0) or n == 1      # one point: no pair, the distinct bound is 0 and the sum exactly 0
      ratio = np.abs(got.astype(EXT) - S).astype(np.float64) / np.where(B > 0, B, 1.0)
      assert np.all((B > 0) | (got == 0))
      worst = max(worst, float(ratio.max()))
  print("%s shift %g: plain fp64 numpy worst error / bound %.3g" % (case, shift, worst))
  assert worst <= 1.0


def test_special_heights_and_regimes_are_in_the_trajectory():
  frames, L, mob_L = hn.trajectory("wall_periodic")
  z = frames[0, :, 2]
  for h in hn.SPECIAL_Z:
    assert np.any(z == h), h
  d = np.sqrt(((frames[0][:, None, :] - frames[0][None, :, :]) ** 2).sum(axis=2)) + 10.0 * np.eye(len(z))
  assert d.min() > 0 and (d < 1e-6 * hn.A).any() and ((d > 0.1 * hn.A) & (d < 1.9 * hn.A)).any()      # a coincident pair, overlaps
  assert mob_L[2] == 0 and np.all(mob_L[:2] == L[:2])


def test_c_sum_counts_the_tiles():
  assert hn.c_sum(1) == 64 + 9 and hn.c_sum(64) == 64 + 9 and hn.c_sum(65) == 3 * 64 + 9 and hn.c_sum(200) == 10 * 64 + 9


# ---- polarisations -----------------------------------------------------------------------------------------------------
def test_polarisation_helpers():
  L = (10.0, 20.0, 5.0)
  n = np.array([[1, 0, 0], [0, 2, 0], [3, 4, 0], [1, 1, 1], [0, 0, 2]], dtype=np.int32)
  e = hf.polarisations(L, n[:4], "longitudinal")
  k = n[:4] / np.array(L)
  assert np.allclose(e, k / np.linalg.norm(k, axis=1)[:, None], rtol=0, atol=2e-16)
  assert np.all(np.abs(np.linalg.norm(e, axis=1) - 1) < 3e-16)
  t = hf.polarisations(L, n[:4], "transverse")
  assert np.all(np.abs((t * e).sum(axis=1)) < 3e-16) and np.all(t[:, 2] == 0) and np.all(np.abs(np.linalg.norm(t, axis=1) - 1) < 3e-16)
  assert np.array_equal(t[0], [0.0, 1.0, 0.0]) or np.allclose(t[0], [0.0, 1.0, 0.0], atol=1e-17)
  v = hf.polarisations(L, n, "vertical")
  assert np.array_equal(v, np.tile([0.0, 0.0, 1.0], (5, 1)))
  given = np.arange(15.0).reshape(5, 3)
  assert np.array_equal(hf.polarisations(L, n, given), given)
  with pytest.raises(ValueError, match="longitudinal polarisation of n = 0"):
    hf.polarisations(L, np.array([[1, 0, 0], [0, 0, 0]]), "longitudinal")
  with pytest.raises(ValueError, match="k_xy != 0"):
    hf.polarisations(L, n, "transverse")
  with pytest.raises(ValueError, match="polarisation must be one of"):
    hf.polarisations(L, n, "circular")
  with pytest.raises(ValueError, match="one finite vector per wavevector"):
    hf.polarisations(L, n, np.zeros((4, 3)))
  with pytest.raises(ValueError, match="one finite vector per wavevector"):
    hf.polarisations(L, n, np.full((5, 3), np.nan))


# ---- refusals of the Python layer ----------------------------------------------------------------------------------------
class _NotAContext(object):      # what a MultiContext looks like to the analysis: no frames entry
  device = 0

  def close(self):
    pass


def test_python_layer_refusals():
  L, wv = (10.0, 10.0, 0.0), np.array([[1, 0, 0], [1, 1, 0]], dtype=np.int32)
  ctx = _NotAContext()
  with pytest.raises(ValueError, match="single-GPU MobilityContext"):
    hf.HydrodynamicFunction(10, L, wv, 0.5, 1.0, ctx=ctx)
  with pytest.raises(ValueError, match="per-blob radii"):
    hf.HydrodynamicFunction(10, L, wv, np.full(10, 0.5), 1.0, ctx=ctx)
  with pytest.raises(ValueError, match="no free surface"):
    hf.HydrodynamicFunction(10, L, wv, 0.5, 1.0, wall="free_surface", ctx=ctx)
  with pytest.raises(ValueError, match="positive lengths in x and y"):
    hf.HydrodynamicFunction(10, (10.0, 0.0, 0.0), wv[:1], 0.5, 1.0, ctx=ctx)
  with pytest.raises(ValueError, match="longitudinal polarisation of n = 0"):
    hf.HydrodynamicFunction(10, L, np.array([[0, 0, 0]], dtype=np.int32), 0.5, 1.0, ctx=ctx)
  with pytest.raises(ValueError, match="positive and finite"):
    hf.HydrodynamicFunction(10, L, wv, 0.0, 1.0, ctx=ctx)
  with pytest.raises(ValueError, match="at least 1"):
    hf.HydrodynamicFunction(0, L, wv, 0.5, 1.0, ctx=ctx)
  with pytest.raises(ValueError, match="integer array"):
    hf.HydrodynamicFunction(10, L, wv.astype(np.float64), 0.5, 1.0, ctx=ctx)
  # the context's own argument checks (before anything touches the library)
  pol = np.tile([1.0, 0.0, 0.0], (2, 1))
  args = MobilityContext._hydro_args
  with pytest.raises(ValueError, match="no in_plane variant"):
    args(0.5, L, wv, pol, True, 0, 1)
  with pytest.raises(ValueError, match="pair shards"):
    args(0.5, L, wv, pol, False, 1, 2)
  with pytest.raises(ValueError, match="per-blob radii"):
    args(np.full(10, 0.5), L, wv, pol, False, 0, 1)
  with pytest.raises(ValueError, match=r"shape \(K, 3\)"):
    args(0.5, L, wv, pol[:1], False, 0, 1)
  Lk, k, e = args(0.5, L, wv, pol, False, 0, 1)
  assert k.dtype == np.int32 and e.dtype == np.float64 and Lk.shape == (3,)


# ---- command line ----------------------------------------------------------------------------------------------------
def test_command_line_parsing(capsys):
  a = hf.parse_args(["run.config", "65", "10", "12", "0", "--radius", "0.5", "--eta", "1.3"])
  assert (a.np, a.lx, a.ly, a.lz, a.radius, a.eta) == (65, 10.0, 12.0, 0.0, 0.5, 1.3)
  assert a.wall and a.periodic and not a.with_S and a.plane == "xy" and a.polarisation == "longitudinal" and a.every == 1 and a.shells == 0
  b = hf.parse_args(["run.config", "65", "10", "12", "3", "--radius", "0.5", "--eta", "1", "--no-wall", "--open", "--with-S", "--kmax", "2.5",
                     "--plane", "xyz", "--polarisation", "vertical", "--every", "2", "--skip", "1", "--shells", "4"])
  assert not b.wall and not b.periodic and b.with_S and b.kmax == 2.5 and b.plane == "xyz" and b.polarisation == "vertical"
  assert (b.every, b.skip, b.shells) == (2, 1, 4)
  for bad in (["run.config", "65", "10", "12", "0", "--eta", "1"],                                       # no radius
              ["run.config", "65", "10", "12", "0", "--radius", "0.5", "--eta", "-1"],
              ["run.config", "65", "10", "12", "0", "--radius", "0.5", "--eta", "1", "--every", "0"],
              ["run.config", "65", "10", "12", "0", "--radius", "0.5", "--eta", "1", "--polarisation", "circular"]):
    with pytest.raises(SystemExit):
      hf.parse_args(bad)
  capsys.readouterr()


# ---- sums, shells, write -----------------------------------------------------------------------------------------------
def _synthetic():
  L = (11.0, 20.0, 0.0)
  wv = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0], [0, 3, 0]], dtype=np.int32)
  rng = np.random.RandomState(3)
  values = rng.uniform(0.2, 1.0, (7, 5, 2))
  return L, wv, values


def test_sums_do_not_depend_on_the_cut():
  L, wv, values = _synthetic()
  whole = hf.HydroSums(L, wv).add_values(values)
  for cut in (1, 3):
    parts = hf.HydroSums(L, wv).add_values(values[:cut]).add_values(values[cut:])
    for name in ("H", "H_self", "H_distinct", "stderr"):
      assert np.array_equal(getattr(parts, name)(), getattr(whole, name)()), (cut, name)
  h = values.sum(axis=2)
  assert np.allclose(whole.H(), h.mean(axis=0), rtol=1e-15) and np.allclose(whole.H_self(), values[..., 0].mean(axis=0), rtol=1e-15)
  assert np.allclose(whole.stderr(), h.std(axis=0, ddof=1) / np.sqrt(7.0), rtol=1e-12)
  assert np.array_equal(whole.H(), whole.H_self() + whole.H_distinct()) or np.allclose(whole.H(), whole.H_self() + whole.H_distinct(), rtol=4e-16)
  assert np.all(np.isnan(hf.HydroSums(L, wv).add_values(values[:1]).stderr()))
  with pytest.raises(ValueError, match=r"\(frames, K, 2\)"):
    whole.add_values(values[:, :4])


def test_write_and_shells_round_trip(tmp_path):
  L, wv, values = _synthetic()
  acc = hf.HydroSums(L, wv).add_values(values)
  S = np.linspace(0.5, 1.5, 5)
  path = str(tmp_path / "h.txt")
  acc.write(path, S=S)
  rows = np.loadtxt(path)
  assert rows.shape == (5, 10)
  assert np.array_equal(rows[:, :3], acc.k) and np.array_equal(rows[:, 3], acc.k_norm)
  assert np.array_equal(rows[:, 4], acc.H_self()) and np.array_equal(rows[:, 5], acc.H_distinct()) and np.array_equal(rows[:, 6], acc.H())
  assert np.array_equal(rows[:, 7], acc.stderr()) and np.array_equal(rows[:, 8], S) and np.array_equal(rows[:, 9], acc.H() / S)
  assert np.array_equal(acc.D_short(S), acc.H() / S)
  acc.write(path)
  assert np.loadtxt(path).shape == (5, 8)
  # shells: |k| / 2 pi = 0.091, 0.05, 0.104, 0.189, 0.15 in two shells of equal width up to the largest
  k_mean, n_k, avg = acc.shells(2)
  low = acc.k_norm < 0.5 * acc.k_norm.max()
  assert list(n_k) == [int(low.sum()), int((~low).sum())]
  assert np.allclose(avg, [acc.H()[low].mean(), acc.H()[~low].mean()], rtol=1e-15)
  assert np.allclose(k_mean, [acc.k_norm[low].mean(), acc.k_norm[~low].mean()], rtol=1e-15)
  acc.write(path, shells=2, S=S)
  rows = np.loadtxt(path)
  assert rows.shape == (2, 8) and np.array_equal(rows[:, 1], n_k) and np.allclose(rows[:, 4], avg, rtol=1e-15)
  with pytest.raises(ValueError, match="at least 1"):
    acc.shells(0)
  with pytest.raises(ValueError, match="one value per wavevector"):
    acc.D_short(S[:3])
