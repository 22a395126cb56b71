"""Host side of the scattering functions: the numpy restatement's own identities (tests/_scattering_numpy.py: lattice, pair
identity, rigid drift), that plain fp64 numpy meets each bound the GPU tests hold the kernels to (so the bounds are
reachable), wavevectors(), and the argument checks of the C entries and of rigidmultiblobswall_amd.scattering.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import _scattering_numpy as snp
from conftest import GOLDEN, ROOT, load_golden
from rigidmultiblobswall_amd import msd, scattering

LD = np.longdouble


def lattice(shift=0.0):
  """8 x 8 square lattice of spacing 1 in the box 8 x 8, at height 0.3"""
  i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
  return np.stack([i.ravel() + 0.5 + shift, j.ravel() + 0.25 + shift, np.full(64, 0.3)], axis=-1)[None]


def test_lattice_modes():
  L = (8.0, 8.0, 0.0)
  wv = scattering.wavevectors(L, n_max=9)
  rho, T = snp.modes(lattice(), L, wv, absolute=True)
  tol = snp.modes_bound(64, T)[0]
  mag = np.hypot(rho[0, :, 0], rho[0, :, 1])
  bragg = np.all(wv % 8 == 0, axis=1)
  assert bragg.sum() == 4      # (8, 0), (0, 8), (8, 8), (8, -8)
  assert np.all(np.abs(mag[bragg] - 64.0) <= np.sqrt(2) * tol[bragg])
  assert np.all(mag[~bragg] <= np.sqrt(2) * tol[~bragg])
  print("largest off-lattice |rho| = %.2e" % mag[~bragg].max())


def test_pair_identity_on_the_quasi2d_golden():
  g = load_golden(os.path.join(GOLDEN, "g17_gr_quasi2d.npz"))
  frames, L = g["frames"], g["periodic_length"]
  wv = scattering.wavevectors(L, n_max=3)
  rho, T = snp.modes(frames, L, wv, absolute=True)
  tol = snp.modes_bound(frames.shape[1], T)
  for f in range(frames.shape[0]):
    want = snp.pair_sum(frames[f], L, wv).astype(np.float64)
    got = rho[f, :, 0] ** 2 + rho[f, :, 1] ** 2
    mag = np.sqrt(got)
    # |rho|^2 from components each within tol: 2 sqrt(2) |rho| tol + 2 tol^2; the pair sum of N (N - 1) / 2 cosines of differences
    # in long double, each off by a few u of the coordinates' own subtraction: 8 u T per pair at most
    slack = 2 * np.sqrt(2) * mag * tol[f] + 2 * tol[f] ** 2 + 8 * snp.U * frames.shape[1] * T[f] * 2 * np.pi
    assert np.all(np.abs(got - want) <= slack)


def test_rigid_drift():
  L, N, F, n_lags = (7.0, 5.0, 3.0), 5, 12, 6
  wv = snp.mixed_wavevectors(7, seed=3, n_max=4)
  d = np.array([0.031, -0.017, 0.011])
  x0 = snp.random_frames(1, N, L, seed=4)[0]
  frames = x0[None] + np.arange(F)[:, None, None] * d
  kd = (snp.coefficients(L, wv, LD) @ d.astype(LD))      # turns per frame
  rho = snp.modes(frames, L, wv, LD)
  for origins in ("window", "all"):
    C, n_o = snp.collective(rho, n_lags, origins=origins, dtype=LD)
    Sf, n = snp.self_sums(frames, L, wv, n_lags, origins=origins, dtype=LD)
    assert np.array_equal(n_o, msd.counts_per_lag(F, 1, n_lags, origins)) and np.array_equal(n, N * n_o)
    for lag in range(n_lags):
      c = np.cos(2 * snp.pi(LD) * lag * kd)
      sq = (rho[:n_o[lag], :, 0] ** 2 + rho[:n_o[lag], :, 1] ** 2).sum(axis=0)
      # the frames are the exact drift rounded to double: 1e-13 covers that
      assert np.allclose((Sf[lag] / n[lag]).astype(np.float64), c.astype(np.float64), rtol=0, atol=1e-13)
      assert np.allclose((C[lag] / sq).astype(np.float64), c.astype(np.float64), rtol=0, atol=1e-13)


CASES = [(1, 1, 3, 1, 0.0), (1, 2, 1, 1, 0.0), (1, 63, 65, 2, 0.0), (1, 257, 130, 1, 1000.0), (70, 5, 3, 65, 0.0), (9, 64, 4, 9, 1000.0)]


@pytest.mark.parametrize("F, N, K, n_lags, shift", CASES)
def test_the_bounds_of_the_gpu_tests_are_reachable_in_double(F, N, K, n_lags, shift):
  """The fp64 restatement against the long-double one under the bounds the kernels are held to: a bound plain double
  arithmetic could not meet would say nothing about the kernel."""
  L = (6.0, 4.5, 3.0)
  frames = snp.random_frames(F, N, L, seed=10 * N + K, shift=shift)
  wv = snp.mixed_wavevectors(K, seed=K)
  rho_ld, T = snp.modes(frames, L, wv, LD, absolute=True)
  rho = snp.modes(frames, L, wv)
  tol = snp.modes_bound(N, T)[..., None]
  err = np.abs(rho.astype(LD) - rho_ld).astype(np.float64)
  print("modes: max err / bound = %.3f" % np.max(err / tol))
  assert np.all(err <= tol)
  for origins in ("window", "all"):
    C_ld, n_o, A = snp.collective(rho, n_lags, origins=origins, dtype=LD, absolute=True)      # the fp64 modes as exact inputs
    C, _ = snp.collective(rho, n_lags, origins=origins)
    assert np.array_equal(n_o, msd.counts_per_lag(F, 1, n_lags, origins))
    assert np.all(np.abs(C.astype(LD) - C_ld).astype(np.float64) <= snp.collective_bound(n_o, A))
    S_ld, n, TT = snp.self_sums(frames, L, wv, n_lags, origins=origins, dtype=LD, absolute=True)
    S, _ = snp.self_sums(frames, L, wv, n_lags, origins=origins)
    tol_s = snp.self_bound(n, TT)
    err_s = np.abs(S.astype(LD) - S_ld).astype(np.float64)
    print("self %s: max err / bound = %.3f" % (origins, np.max(err_s[tol_s > 0] / tol_s[tol_s > 0]) if (tol_s > 0).any() else 0.0))
    assert np.all(err_s <= tol_s) and np.all(S[n == 0] == 0)


def test_wavevectors_order_and_selection():
  L = (10.0, 6.0, 4.0)
  wv = scattering.wavevectors(L, n_max=3)
  assert wv.dtype == np.int32 and wv.shape == ((7 * 7 - 1) // 2, 3) and np.all(wv[:, 2] == 0)
  as_set = {tuple(n) for n in wv}
  assert len(as_set) == len(wv) and (0, 0, 0) not in as_set
  assert all(tuple(-np.array(n)) not in as_set for n in as_set)      # one of every +-n pair
  for n in wv:      # the first nonzero component is positive
    assert n[np.nonzero(n)[0][0]] > 0
  k = np.linalg.norm(scattering.k_vectors(L, wv), axis=1)
  assert np.all(np.diff(k) >= -1e-12 * k.max())
  assert np.array_equal(wv, scattering.wavevectors(L, n_max=3))      # deterministic
  assert tuple(wv[0]) == (1, 0, 0)      # the longest period first
  # ties in |k| in lexicographic order: a square box, (0, 1) before (1, 0), (1, -1) before (1, 1)
  sq = scattering.wavevectors((5.0, 5.0, 0.0), n_max=1)
  assert [tuple(n) for n in sq] == [(0, 1, 0), (1, 0, 0), (1, -1, 0), (1, 1, 0)]
  # k_max selects by |k|, n_max by component; both together intersect
  km = scattering.wavevectors(L, k_max=2.0)
  kk = np.linalg.norm(scattering.k_vectors(L, km), axis=1)
  assert np.all(kk <= 2.0 * (1 + 1e-12)) and len(km) > 0
  every = scattering.wavevectors(L, n_max=8)
  inside = np.linalg.norm(scattering.k_vectors(L, every), axis=1) <= 2.0
  assert {tuple(n) for n in every[inside]} == {tuple(n) for n in km}
  both = scattering.wavevectors(L, n_max=1, k_max=2.0)
  assert {tuple(n) for n in both} == {tuple(n) for n in km if np.all(np.abs(n) <= 1)}
  # three dimensions: n_z too, and an open direction stays 0
  xyz = scattering.wavevectors(L, n_max=1, plane="xyz")
  assert len(xyz) == (27 - 1) // 2 and np.any(xyz[:, 2] != 0)
  assert np.all(scattering.wavevectors((10.0, 6.0, 0.0), n_max=1, plane="xyz")[:, 2] == 0)
  assert np.all(scattering.wavevectors((0.0, 6.0, 0.0), n_max=2)[:, 0] == 0)
  for bad in (dict(), dict(n_max=-1), dict(k_max=-1.0), dict(n_max=1, plane="yz")):
    with pytest.raises(ValueError):
      scattering.wavevectors(L, **bad)


def test_shell_average():
  k = np.array([0.5, 1.0, 1.0, 2.0, 4.0])
  v = np.array([[1.0, 2.0, 4.0, 8.0, 16.0], [0.0, 1.0, 1.0, 1.0, 2.0]])
  k_mean, n_k, avg = scattering.shell_average(k, v, 4)      # shells (0, 1), [1, 2), [2, 3), [3, 4]
  assert np.array_equal(n_k, [1, 2, 1, 1])
  assert np.array_equal(k_mean, [0.5, 1.0, 2.0, 4.0])
  assert np.array_equal(avg, [[1.0, 3.0, 8.0, 16.0], [0.0, 1.0, 1.0, 2.0]])
  assert np.isnan(scattering.shell_average(np.array([1.0, 4.0]), np.array([1.0, 2.0]), 4)[2][0])      # nobody in (0, 1)


def test_c_entries_refuse_bad_arguments_without_a_device():
  """Every argument check comes before the context is looked at: with a null context each bad argument is named, and only
  a call whose arguments are in order is refused for the context."""
  from rigidmultiblobswall_amd import _lib
  lib, ARG = _lib.load(), -1      # RMB_ERR_ARG
  header = open(os.path.join(ROOT, "include", "rmb_mobility.h")).read()
  buf, L, wv, big = np.zeros(64), np.array([4.0, 3.0, 0.0]), np.array([[1, 0, 0], [1, -2, 0]], dtype=np.int32), np.zeros((16385, 3), dtype=np.int32)
  out = np.zeros(64)
  p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
  good = dict(frames=p(buf), n_frames=3, n=2, L=p(L), kint=p(wv), K=2, n_lags=2, o_begin=0, o_end=2, out=p(out))
  wv_n = np.array([[1, 0, 0], [32769, 0, 0]], dtype=np.int32)
  wv_z = np.array([[1, 0, 0], [1, 0, -1]], dtype=np.int32)
  L_x = np.array([0.0, 3.0, 2.0])
  sizes = [(dict(n_frames=-1), "negative size"), (dict(K=-1), "negative size"), (dict(K=16385, kint=p(big)), "at most 16384")]
  waves = [(dict(n=-1), "negative size"), (dict(L=None), "null L"), (dict(kint=None), "null wavevector"), (dict(kint=p(wv_n)), "at most 32768"),
           (dict(kint=p(wv_z)), "positive length"), (dict(L=p(L_x)), "positive length"), (dict(frames=None), "null frames")]
  lags = [(dict(n_lags=0), "n_lags must be at least 1"), (dict(o_end=4), "o_begin <= o_end <= n_frames"),
          (dict(o_begin=-1), "o_begin <= o_end <= n_frames"), (dict(o_begin=2, o_end=1), "o_begin <= o_end <= n_frames")]
  calls = {
      "rmb_density_modes_frames_device": (lambda a: (a["frames"], a["n_frames"], a["n"], a["L"], a["kint"], a["K"], a["out"]),
                                          sizes + waves + [(dict(out=None), "null modes")]),
      "rmb_scattering_lags_device": (lambda a: (a["frames"], a["n_frames"], a["K"], a["n_lags"], a["o_begin"], a["o_end"], a["out"]),
                                     sizes + lags + [(dict(frames=None), "null modes"), (dict(out=None), "null sums")]),
      "rmb_self_scattering_frames_device": (lambda a: (a["frames"], a["n_frames"], a["n"], a["L"], a["kint"], a["K"], a["n_lags"], a["o_begin"],
                                                       a["o_end"], a["out"]), sizes + waves + lags + [(dict(out=None), "null sums")]),
  }
  for name, (args, bad) in calls.items():
    assert name in _lib.SYMBOLS and ("int %s(" % name) in header
    fn = getattr(lib, name)
    for change, message in bad + [(dict(), "null context")]:
      rc = fn(None, *args(dict(good, **change)))
      assert rc == ARG, (name, change)
      assert message in lib.rmb_last_error().decode(), (name, change, lib.rmb_last_error())
  assert np.all(out == 0)


def test_python_argument_errors():
  L, wv = (4.0, 3.0, 0.0), np.array([[1, 0, 0]], dtype=np.int32)
  IS = scattering.IntermediateScattering
  with pytest.raises(ValueError, match="n_lags"):
    IS(3, L, wv, n_lags=0)
  with pytest.raises(ValueError, match="origins must be"):
    IS(3, L, wv, origins="every")
  with pytest.raises(ValueError, match="n_points"):
    IS(-1, L, wv)
  with pytest.raises(ValueError, match="three lengths"):
    IS(3, (4.0, 3.0), wv)
  with pytest.raises(ValueError, match="integer array"):
    IS(3, L, np.array([[1.0, 0.0, 0.0]]))
  with pytest.raises(ValueError, match="integer array"):
    IS(3, L, np.array([1, 0, 0]))
  with pytest.raises(ValueError, match="positive length"):
    IS(3, L, np.array([[1, 0, 1]]))
  with pytest.raises(ValueError, match="at most 32768"):
    IS(3, L, np.array([[40000, 0, 0]]))
  with pytest.raises(ValueError, match="at most 16384 wavevectors"):
    IS(3, L, np.ones((16385, 3), dtype=np.int32))


def test_output_round_trip():
  blocks = snp.parse_output("# t 0 5\n1 0 0 1 2.5 1\n0 1 0 1 3.5 1\n# t 0.5 4\n1 0 0 1 2.25 0.5\n0 1 0 1 3.25 0.25\n")
  assert [b[:2] for b in blocks] == [(0.0, 5), (0.5, 4)]
  assert np.array_equal(blocks[1][2], [[1, 0, 0, 1, 2.25, 0.5], [0, 1, 0, 1, 3.25, 0.25]])
  only = snp.parse_output("1 0 0 1 2.5\n")
  assert only[0][:2] == (None, None) and only[0][2].shape == (1, 5)
  frames = snp.random_frames(2, 3, (4.0, 3.0, 0.0), seed=1)
  from rigidmultiblobswall_amd.correlation import read_frames
  import tempfile
  with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "run.config")
    with open(path, "w") as f:
      f.write(snp.config_text(frames))
    assert np.array_equal(read_frames(path, 3), frames)
