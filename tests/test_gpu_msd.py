"""The HIP mean-square displacement (rmb_msd_frames_device, rigidmultiblobswall_amd.msd) against the long-double restatement
(tests/_msd_numpy.py), under a bound derived from the kernel's arithmetic.

The bound, with u = 2^-53, per lag l and entry (i, j):

    |S_gpu - S_ld| <= u [ (n[l] + C0) A_ij[l] + C1 (X_i B_j[l] + X_j B_i[l]) ],
    A_ij = sum |Delta_i Delta_j|,  B_i = sum |Delta_i|,  X = max(|x| + |p|) (translational), 1 (rotational).

A computed displacement is d_i = Delta_i (1 + r_i) + e_i with |r_i| <= u and an ABSOLUTE error e_i that does not shrink with
Delta; a term's error is then |Delta_i| e_j + |Delta_j| e_i + (r_i + r_j) |Delta_i Delta_j| to first order, and summing gives
the two parts of the bound.

  C1, translational.  The tracked point c = x + 2 (M p), M = R / 2 from the unnormalised quaternion as in the reference.
    An entry of M is two products and one or two sums of numbers <= 1/2 .. 1: at most 3 u absolute.  Row times p: sum_j dM_ij
    p_j <= 9 u |p|, three products (|M_ij| <= 1/2: 1.5 u |p|) and two sums (2 u |p|): 12.5 u |p|, doubled 25 u |p|; the final sum
    adds u (|x| + sqrt(3) |p|): e_c <= u |x| + 27 u |p| <= 27 u X.  A displacement is the difference of two such points:
    e <= 54 u X, and r is the one rounding of the subtraction.  (No offset: c = x exactly, e = 0.)
  C1, rotational.  u = 2 s_rel v_rel.  s_rel: one product and three fused steps on partial sums <= 1 (Cauchy-Schwarz, unit
    quaternions): 4 u.  A component of v_rel: the differences b - a and s1 - s0 (relative, <= 2 u in all), one product (u / 2),
    two fused steps (u each), one more product and the final subtraction (u): <= 4 u.  The product 2 s_rel v_rel:
    2 (|s_rel| 4 u + |v_rel| 4 u) + u <= 17 u.  The kernel's quaternion form and the oracle's rotation-matrix form agree only
    for unit quaternions: with |q|^2 = 1 + eps the matrix is R^ + eps (R^ + 1), which moves the oracle's u by at most eps_0 +
    eps_1 in absolute terms.  The trajectories here are normalised in double, q / |q|: the computed norm is off by at most
    3 u relative (four squares, three sums, the root), each quotient by u more, so |eps| <= 2 (3 u + u) = 8 u (asserted), and
    the two forms differ by at most 16 u: 33 u.  (The fp64 restatement in matrix form: entries of R to 6 u, four of them per
    cross-product component, over three columns with Cauchy-Schwarz, halved: 21 u, a few u of its own sums: <= 33 u too.)
    C1 = max(54, 33) = 54.
  C0.  The relative part of a term: r_i + r_j = 2, one rounding of the product where it is not fused into the sum (the
    restatement), and 1 for the long-double oracle's own error and the second-order terms left out above: C0 = 4.  The
    summation itself is the n[l]: however the n[l] terms are grouped (lanes, waves, workgroups, the finishing launch), no
    chain of additions is longer than n[l], each step rounding a partial sum of at most A.

test_msd_host.py checks on the CPU that plain fp64 numpy meets this bound, so it is reachable."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _msd_numpy as mnp
from conftest import GOLDEN, ROOT, load_golden
from rigidmultiblobswall_amd import msd

pytestmark = pytest.mark.gpu

N_LAGS = (1, 63, 64, 65, 130)      # below, at and above a lag block of 64; three blocks with a masked tail
BODIES = (1, 3, 65)
CHUNKS = (1, 7, 0)                 # origins per staged window: one, a few (several chunks, partial last one), planned


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


_ORACLE = {}


def _dev(frames):
  return torch.tensor(frames, dtype=torch.float64, device="cuda")      # a copy: the shared arrays are read-only


def _offsets(N):
  return np.random.RandomState(40 + N).uniform(-0.5, 0.5, (N, 3))


def _oracle(F, N, n_lags, origins, off):
  """frames, offsets, long-double sums, counts and the bound: computed once per shape, shared, never modified"""
  key = (F, N, n_lags, origins, off)
  if key not in _ORACLE:
    frames = mnp.random_walk(F, N, seed=1000 + 7 * F + N)
    assert np.abs(np.sum(frames[..., 3:].astype(np.longdouble) ** 2, axis=-1) - 1).max() <= 8 * mnp.U      # the bound's precondition
    offsets = _offsets(N) if off else None
    S, n, A, B = mnp.sums(frames, n_lags, offsets=offsets, origins=origins, dtype=np.longdouble, absolute=True)
    for a in (frames, S, n):
      a.setflags(write=False)
    _ORACLE[key] = (frames, offsets, S, n, mnp.bound(frames, offsets, n, A, B))
  return _ORACLE[key]


def _within(got, S_ld, tol, what):
  err = np.abs(got.astype(np.longdouble) - S_ld).astype(np.float64)
  pos = tol > 0
  print("%s: max err / bound = %.3f" % (what, np.max(err[pos] / tol[pos]) if pos.any() else 0.0))
  assert np.all(err <= tol), what
  assert np.array_equal(got, got.transpose(0, 2, 1)), what      # both triangles, the same bits


@pytest.mark.parametrize("F_kind", ["one_origin", "two_origins", "long"])
@pytest.mark.parametrize("N", BODIES)
@pytest.mark.parametrize("n_lags", N_LAGS)
def test_sums_against_the_long_double_oracle(ctx, n_lags, N, F_kind):
  F = {"one_origin": n_lags, "two_origins": n_lags + 1, "long": 300 + n_lags % 7}[F_kind]
  # offsets with one convention, none with the other; which way round alternates with the lag count
  for origins, off in (("window", n_lags % 2 == 1), ("all", n_lags % 2 == 0)):
    frames, offsets, S_ld, n, tol = _oracle(F, N, n_lags, origins, off)
    dev = _dev(frames)
    for chunk in CHUNKS:
      sums, counts = ctx.msd_frames_device(dev, n_lags, offsets=offsets, origins=origins, origin_chunk=chunk)
      assert np.array_equal(counts, n) and counts.dtype == np.int64
      _within(sums.cpu().numpy(), S_ld, tol, "%s off=%s chunk=%d" % (origins, off, chunk))
  if F_kind == "one_origin":
    assert np.all(n[1:] == N * (F - np.arange(1, n_lags))) and n[0] == N * F      # the "all" counts of the last pass


@pytest.mark.parametrize("n_lags, F", [(65, 3), (130, 40), (64, 1)])
def test_all_origins_with_fewer_frames_than_lags(ctx, n_lags, F):
  frames, offsets, S_ld, n, tol = _oracle(F, 3, n_lags, "all", True)
  for chunk in CHUNKS:
    sums, counts = ctx.msd_frames_device(_dev(frames), n_lags, offsets=offsets, origins="all", origin_chunk=chunk)
    got = sums.cpu().numpy()
    assert np.array_equal(counts, n) and np.all(counts[F:] == 0) and counts[F - 1] == 3
    assert np.all(got[F:] == 0.0)      # lags without an origin: exactly zero
    _within(got, S_ld, tol, "chunk=%d" % chunk)
  # the window convention has no origin at all here: zeros, count 0
  sums, counts = ctx.msd_frames_device(_dev(frames), n_lags, origins="window")
  assert np.all(counts == 0) and np.all(sums.cpu().numpy() == 0.0)


def test_lag_zero_is_exact(ctx):
  frames, offsets, S_ld, n, tol = _oracle(130, 3, 65, "all", True)
  sums, _ = ctx.msd_frames_device(_dev(frames), 65, offsets=offsets, origins="all")
  assert np.all(sums[0].cpu().numpy() == 0.0)


def test_4096_lags(ctx):
  """64 lag blocks; the window convention leaves five origins, the oracle stays cheap"""
  frames, offsets, S_ld, n, tol = _oracle(4100, 1, 4096, "window", False)
  sums, counts = ctx.msd_frames_device(_dev(frames), 4096, origins="window")
  assert np.all(counts == 5)
  _within(sums.cpu().numpy(), S_ld, tol, "4096 lags")


@pytest.mark.parametrize("origins", ["window", "all"])
def test_closed_form(ctx, origins):
  """constant velocity and angular velocity about a fixed axis: Delta = [v l tau; sin(w l tau) n]; the sums against the exact
  ones under the same bound (X from the trajectory, A and B from the exact displacements)"""
  F, N, L = 80, 5, 66      # two lag blocks; tau = 2^-8 keeps every angle below 4 rad, so that their own rounding stays a few u
  frames, exact = mnp.screw_motion(F, N, seed=3, tau=2.0 ** -8)
  assert np.abs(np.sum(frames[..., 3:].astype(np.longdouble) ** 2, axis=-1) - 1).max() <= 8 * mnp.U
  sums, counts = ctx.msd_frames_device(_dev(frames), L, origins=origins)
  got = sums.cpu().numpy()
  want, A, B = np.zeros((L, 6, 6)), np.zeros((L, 6, 6)), np.zeros((L, 6))
  for lag in range(L):
    D, k = exact(lag), counts[lag] // N
    want[lag], A[lag], B[lag] = k * np.einsum("bi,bj->ij", D, D), k * np.einsum("bi,bj->ij", np.abs(D), np.abs(D)), k * np.abs(D).sum(axis=0)
  # the quaternions of the trajectory carry their own rounding (the exact motion's, rounded: 2 u per factor of R, absolute):
  # it enters like the rotational e above, well inside C1
  tol = mnp.bound(frames, None, counts, A, B)
  assert np.all(np.abs(got - want) <= tol)
  assert np.all(counts == N * (F - L + 1)) if origins == "window" else np.array_equal(counts, N * (F - np.arange(L)))


@pytest.mark.parametrize("name", ["plain", "interval", "tracked"])
def test_reference_msd_against_the_golden(ctx, name):
  g = load_golden(os.path.join(GOLDEN, "g18_msd_reference.npz"))
  offset = g[name + "_offset"] if bool(g[name + "_has_offset"]) else None
  got = msd.reference_msd(g[name + "_locations"], g[name + "_orientations"], float(g[name + "_dt"]), float(g[name + "_end"]),
                          burn_in=int(g[name + "_burn_in"]), trajectory_length=int(g[name + "_trajectory_length"]), offset=offset, ctx=ctx)
  want = g[name + "_msd"]
  assert got.shape == want.shape
  assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("origins", ["window", "all"])
def test_streamed_in_uneven_chunks(ctx, origins):
  F, N, L = 300, 3, 65
  frames, offsets, S_ld, n, tol = _oracle(F, N, L, origins, True)
  one_shot, counts = ctx.msd_frames_device(_dev(frames), L, offsets=offsets, origins=origins)
  acc = msd.MeanSquareDisplacement(N, L, dt=0.25, origins=origins, offsets=offsets, ctx=ctx)
  acc.add_frames(frames[:1]).add_frames(torch.from_numpy(frames[1:6]).cuda()).add_frames(frames[6:])
  assert acc._tail is not None and [t.shape[0] for t in acc._tail] == [L - 1]      # only the origins whose lags are not complete are kept
  acc.finish()
  assert np.array_equal(acc.counts(), n) and np.array_equal(acc.counts(), counts) and acc.n_frames == F
  _within(acc.sums(), S_ld, tol, "streamed")
  _within(one_shot.cpu().numpy(), S_ld, tol, "one shot")
  assert np.array_equal(acc.times(), 0.25 * np.arange(L))
  assert np.allclose(acc.msd(), acc.sums() / n[:, None, None], rtol=0, atol=0)
  with pytest.raises(ValueError, match="after finish"):
    acc.add_frames(frames[:1])
  acc.close()
  assert ctx._h.value      # a caller's context is not closed


def test_same_call_same_bits_and_out_is_added_to(ctx):
  frames, offsets, S_ld, n, tol = _oracle(300, 3, 65, "all", True)
  dev = _dev(frames)
  a, _ = ctx.msd_frames_device(dev, 65, offsets=offsets, origins="all")
  b, _ = ctx.msd_frames_device(dev, 65, offsets=offsets, origins="all")
  assert torch.equal(a, b)
  out = torch.full((65, 6, 6), 2.0, dtype=torch.float64, device="cuda")
  c, _ = ctx.msd_frames_device(dev, 65, offsets=offsets, origins="all", out=out)
  assert c is out and torch.equal(out, a + 2.0)      # one addition per entry: a + 2 rounded once, like the reference value
  for bad in (torch.zeros((65, 36), dtype=torch.float64, device="cuda"), torch.zeros((65, 6, 6), dtype=torch.float32, device="cuda"),
              torch.zeros((65, 6, 6), dtype=torch.float64), torch.zeros((6, 6, 65), dtype=torch.float64, device="cuda").permute(2, 0, 1)):
    with pytest.raises(ValueError, match="out must be"):
      ctx.msd_frames_device(dev, 65, out=bad)
  with pytest.raises(ValueError, match="frames must be"):
    ctx.msd_frames_device(dev[..., :3], 65)
  with pytest.raises(ValueError, match="frames must be"):
    ctx.msd_frames_device(frames, 65)


def test_host_entry_equals_the_device_entry(ctx):
  import ctypes
  from rigidmultiblobswall_amd import _lib
  frames, offsets, S_ld, n, tol = _oracle(300, 3, 65, "all", True)
  dev, _ = ctx.msd_frames_device(_dev(frames), 65, offsets=offsets, origins="all", origin_chunk=7)
  host = np.full((65, 6, 6), 3.0)      # the host entry zeroes first
  f, o = np.ascontiguousarray(frames), np.ascontiguousarray(offsets)
  _lib.check(_lib.load().rmb_msd_frames(ctx._h, ctypes.c_void_p(f.ctypes.data), 300, 3, ctypes.c_void_p(o.ctypes.data), 65, 0, 300, 7,
                                        ctypes.c_void_p(host.ctypes.data)))
  assert np.array_equal(host, dev.cpu().numpy())
  # an origin range of the caller's: [o_begin, o_end) only
  part = np.empty((65, 6, 6))
  _lib.check(_lib.load().rmb_msd_frames(ctx._h, ctypes.c_void_p(f.ctypes.data), 300, 3, None, 65, 10, 17, 0, ctypes.c_void_p(part.ctypes.data)))
  c, R = mnp.tracked(frames, None, np.longdouble)
  want = np.zeros((65, 6, 6), dtype=np.longdouble)
  for lag in range(65):
    D = mnp.displacements(c[10:], R[10:], lag, 7).reshape(-1, 6)
    want[lag] = np.einsum("ti,tj->ij", D, D)
  assert np.allclose(part, want.astype(np.float64), rtol=1e-12, atol=1e-15)


def test_resident_configuration_is_left_alone():
  """a wall M_tt f of the resident blobs before and after, on the atomic-free sweep (option "deterministic": the default
  product adds with floating-point atomics and is not the same bits twice anyway)"""
  from rigidmultiblobswall_amd import MobilityContext
  rng = np.random.RandomState(4)
  r = rng.uniform(0, 6, (500, 3)) + np.array([0, 0, 0.5])
  f = rng.randn(1500)
  frames, offsets, *_ = _oracle(300, 3, 65, "all", True)
  c = MobilityContext(0)
  try:
    c.set_option("deterministic", 1)
    c.set_positions(r, 0.2, wall=True)
    before, again = c.matvec("tt", f, 1.0), c.matvec("tt", f, 1.0)
    assert np.array_equal(before, again)      # the yardstick itself repeats
    c.msd_frames_device(_dev(frames), 65, offsets=offsets, origins="all")
    c.msd_frames_device(_dev(frames), 65, origins="window", origin_chunk=7)
    torch.cuda.synchronize()
    after = c.matvec("tt", f, 1.0)
    assert np.array_equal(before, after) and c.n == 500
  finally:
    c.close()


def test_multi_device_context_refuses(ctx):
  from rigidmultiblobswall_amd.multi import MultiContext
  m = MultiContext([0])
  try:
    assert not hasattr(m, "msd_frames_device")
    with pytest.raises(ValueError, match="single-GPU MobilityContext"):
      msd.MeanSquareDisplacement(2, 4, ctx=m)
  finally:
    m.close()


def test_command_line_matches_the_class(ctx, tmp_path):
  frames = mnp.random_walk(40, 2, seed=77)
  traj = tmp_path / "run.config"
  traj.write_text(mnp.config_text(frames))
  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
  out = subprocess.run([sys.executable, "-m", "rigidmultiblobswall_amd.msd", str(traj), "2", "0.5", "--lags", "9", "--every", "2", "--skip", "3",
                        "--origins", "all", "--offset", "0.1,-0.2,0.3"], check=True, capture_output=True, text=True, env=env, timeout=300).stdout
  t, n, tri = mnp.parse_msd(out)
  acc = msd.MeanSquareDisplacement(2, 9, dt=1.0, origins="all", offsets=(0.1, -0.2, 0.3), ctx=ctx)
  acc.add_frames(frames[3::2]).finish()
  assert np.array_equal(t, acc.times()) and np.array_equal(n, acc.counts())
  assert np.array_equal(tri, acc.msd()[:, msd.TRIU[0], msd.TRIU[1]])      # 17 digits: the same doubles
  # the module's main() in this process, and write()
  buf = io.StringIO()
  assert msd.main([str(traj), "2", "0.5", "--lags", "9", "--every", "2", "--skip", "3", "--origins", "all", "--offset", "0.1,-0.2,0.3"], out=buf) == 0
  assert buf.getvalue() == out
  acc.write(str(tmp_path / "msd.txt"))
  assert (tmp_path / "msd.txt").read_text() == out
  acc.close()
