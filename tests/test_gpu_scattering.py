"""The HIP scattering sweeps (rmb_density_modes_frames_device, rmb_scattering_lags_device, rmb_self_scattering_frames_device,
rigidmultiblobswall_amd.scattering) against the long-double restatement (tests/_scattering_numpy.py), under bounds derived
from the kernels' arithmetic.  u = 2^-53; T_j = sum_d |n_d x_jd / L_d| is the size of a point's phase in turns.

The phase of a point (scat_phase): c_d = n_d / L_d is one correctly rounded division (relative error u); the turn count
t = fma(z, c_z, fma(y, c_y, x c_x)) rounds three times, each time a partial sum of magnitude at most T: with the error of
the c_d, |dt| <= 4 u T.  r = t - rint(t) is exact (|r| <= 1/2 and r is a multiple of the last bit of t), and so is 2 r.
The reference reduces its own, exact t, so the two reduced phases differ by dt modulo whole turns, which no trigonometric
function sees.  sincospi(2 r) returns cos and sin of 2 pi r to within about one unit in the last place of a number <= 1,
i.e. e_s <= 2 u absolute; the phase error moves either by at most 2 pi |dt| <= 8 pi u T < 26 u T.

  Modes, per component:  |d rho| <= u [ (N + C0) N + C1 sum_j T_j ],  C0 = 4, C1 = 32.
    C1: 8 pi = 25.2 from the turn count as above, rounded up to 32 for the second-order terms and the long-double
    reference's own division and products (2^-64 T each).  C0: every term is off by e_s <= 2 u before it is added; the
    remaining 2 u cover the reference's own rounding and the products of first-order terms.  The summation is the N N: the
    N terms of magnitude <= 1 are added lane by lane, wave by wave and range by range, in any grouping a chain of at most N
    additions, each rounding a partial sum of at most N.
  Collective lags, the modes taken as exact inputs:  |d C[l]| <= u (n_o[l] + 3) sum_o (|a_r b_r| + |a_i b_i|).
    A term is fma(b_r, a_r, b_i a_i): one rounded product, one fused step, 2 u of the term's absolute value; the n_o terms
    are added in a chain of at most n_o - 1 additions, however they are grouped; one more for the reference.  The standard
    bound of a dot product, for any order of summation.
  Self lags:  |d Sf[l]| <= u [ (n[l] + C0) n[l] + C1 sum (T_j(o) + T_j(o + l)) ],  n[l] = N n_o[l] terms.
    A term Re(z1 conj z0) of unit phase factors: its error is at most |dz1| + |dz0| to first order, each the phase error
    8 pi u T (C1, as for the modes) plus the sincospi error; the product and the fused step add 2 u.  With e_s of one unit in
    the last place of numbers that are rarely both near 1 this stays inside C0 = 4 on average, not in the worst case
    (2 sqrt(2) e_s + 2 u = 7.7 u for e_s = 2 u): for n[l] = 1 the bound is the sharpest statement here, and where an
    arithmetic mistake would show.  Summation: n[l] n[l] as above.

test_scattering_host.py checks on the CPU that plain fp64 numpy meets each of these bounds, so they are reachable.
Measured on an MI355X (profiles/r23_scattering_bounds.txt), worst error / bound: modes 0.29 (N = 1), collective lags 0.43,
self lags 0.18."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _scattering_numpy as snp
from conftest import GOLDEN, ROOT, load_golden
from rigidmultiblobswall_amd import _lib, msd, scattering

pytestmark = pytest.mark.gpu

LD = np.longdouble
BOX = (6.0, 4.5, 3.0)      # anisotropic, every direction periodic


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _dev(a):
  return torch.tensor(a, dtype=torch.float64, device="cuda")      # a copy: the shared arrays are read-only


_ORACLE = {}


def _modes_oracle(F, N, K, shift, L=BOX):
  """frames, wavevectors (mixed signs, n_z != 0), long-double modes and the bound: once per shape, shared, never modified"""
  key = (F, N, K, shift, L)
  if key not in _ORACLE:
    frames = snp.random_frames(F, N, L, seed=100 * N + K + F, shift=shift)
    wv = snp.mixed_wavevectors(K, seed=K + 1)
    rho, T = snp.modes(frames, L, wv, LD, absolute=True)
    tol = snp.modes_bound(N, T)
    for a in (frames, wv, rho, tol):
      a.setflags(write=False)
    _ORACLE[key] = (frames, wv, rho, tol)
  return _ORACLE[key]


def _ratio(err, tol):
  pos = tol > 0
  return float(np.max(err[pos] / tol[pos])) if pos.any() else 0.0


def _modes_within(got, rho_ld, tol, what):
  err = np.abs(got.astype(LD) - rho_ld).astype(np.float64)
  print("modes %s: max err / bound = %.3f" % (what, _ratio(err, np.broadcast_to(tol[..., None], err.shape))))
  assert np.all(err <= tol[..., None]), what


def _sums_within(kind, got, want_ld, tol, what):
  err = np.abs(got.astype(LD) - want_ld).astype(np.float64)
  print("%s %s: max err / bound = %.3f" % (kind, what, _ratio(err, tol)))
  assert np.all(err <= tol), (kind, what)


MODE_SHAPES = [(1, 1), (2, 3), (63, 63), (64, 64), (65, 65), (257, 130), (1, 130), (257, 1)]      # (N, K)


@pytest.mark.parametrize("shift", [0.0, 1000.0])
@pytest.mark.parametrize("N, K", MODE_SHAPES)
def test_modes_against_the_long_double_oracle(ctx, N, K, shift):
  frames, wv, rho_ld, tol = _modes_oracle(3, N, K, shift)
  got = ctx.density_modes_frames_device(_dev(frames), BOX, wv)
  assert tuple(got.shape) == (3, K, 2)
  _modes_within(got.cpu().numpy(), rho_ld, tol, "N=%d K=%d shift=%g" % (N, K, shift))


def test_modes_of_one_large_frame_split_into_point_ranges(ctx):
  """one frame of 20 000 points: the point ranges, their partials and the finishing launch"""
  frames, wv, rho_ld, tol = _modes_oracle(1, 20000, 65, 0.0)
  got = ctx.density_modes_frames_device(_dev(frames), BOX, wv)
  _modes_within(got.cpu().numpy(), rho_ld, tol, "N=20000 K=65")


def test_zero_wavevector_counts_the_points_exactly(ctx):
  frames = snp.random_frames(2, 257, BOX, seed=5)
  wv = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.int32)
  got = ctx.density_modes_frames_device(_dev(frames), (6.0, -1.0, 0.0), wv).cpu().numpy()      # open y and z: allowed where n_d = 0
  assert np.all(got[:, 0, 0] == 257.0) and np.all(got[:, 0, 1] == 0.0)


def test_square_lattice(ctx):
  L = (8.0, 8.0, 0.0)
  i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
  frame = np.stack([i.ravel() + 0.5, j.ravel() + 0.25, np.full(64, 0.3)], axis=-1)[None]
  wv = scattering.wavevectors(L, n_max=9)
  _, T = snp.modes(frame, L, wv, absolute=True)
  tol = np.sqrt(2) * snp.modes_bound(64, T)[0]
  got = ctx.density_modes_frames_device(_dev(frame), L, wv).cpu().numpy()[0]
  mag = np.hypot(got[:, 0], got[:, 1])
  bragg = np.all(wv % 8 == 0, axis=1)
  assert bragg.sum() == 4
  print("lattice: largest off-lattice |rho| = %.2e, err / bound = %.3f" % (mag[~bragg].max(), _ratio(mag[~bragg], tol[~bragg])))
  assert np.all(np.abs(mag[bragg] - 64.0) <= tol[bragg]) and np.all(mag[~bragg] <= tol[~bragg])


def test_pair_identity_on_the_quasi2d_golden(ctx):
  g = load_golden(os.path.join(GOLDEN, "g17_gr_quasi2d.npz"))
  frames, L = g["frames"], g["periodic_length"]
  N = frames.shape[1]
  wv = scattering.wavevectors(L, n_max=3)
  _, T = snp.modes(frames, L, wv, absolute=True)
  tol = snp.modes_bound(N, T)
  got = ctx.density_modes_frames_device(_dev(frames), L, wv).cpu().numpy()
  for f in range(frames.shape[0]):
    want = snp.pair_sum(frames[f], L, wv).astype(np.float64)
    sq = got[f, :, 0] ** 2 + got[f, :, 1] ** 2
    # as test_scattering_host.py: the components within tol, the pair sum's own differences of coordinates
    slack = 2 * np.sqrt(2) * np.sqrt(sq) * tol[f] + 2 * tol[f] ** 2 + 8 * snp.U * N * T[f] * 2 * np.pi
    assert np.all(np.abs(sq - want) <= slack)


def test_wrapping_into_the_box_changes_nothing_beyond_the_bound(ctx):
  frames, wv, rho_ld, tol = _modes_oracle(3, 65, 65, 1000.0)
  box = np.array(BOX)
  wrapped = frames - np.floor(frames / box) * box
  assert np.all((wrapped >= 0) & (wrapped <= box)) and np.abs(frames - wrapped).min() > 100
  _, T = snp.modes(wrapped, BOX, wv, absolute=True)
  a = ctx.density_modes_frames_device(_dev(frames), BOX, wv).cpu().numpy()
  b = ctx.density_modes_frames_device(_dev(wrapped), BOX, wv).cpu().numpy()
  # the wrapped coordinates are themselves rounded: m L and x - m L each to u |x|, which moves a phase by up to 4 pi u T of
  # the unwrapped point
  T_far = snp.turn_magnitudes(frames, BOX, wv).sum(axis=1)
  assert np.all(np.abs(a - b) <= (tol + snp.modes_bound(65, T) + 4 * np.pi * snp.U * T_far)[..., None])


LAG_SHAPES = [(1, 130, 2), (63, 1, 65), (64, 3, 1), (65, 65, 3), (130, 64, 2), (65, 63, 64)]      # (n_lags, K, N)


def _lag_oracle(F, N, K, n_lags, origins, o_begin=0, o_end=None):
  key = ("lags", F, N, K, n_lags, origins, o_begin, o_end)
  if key not in _ORACLE:
    frames, wv, _, _ = _modes_oracle(F, N, K, 0.0)
    S, n, TT = snp.self_sums(frames, BOX, wv, n_lags, o_begin, o_end, origins, LD, absolute=True)
    _ORACLE[key] = (frames, wv, S, n, snp.self_bound(n, TT))
  return _ORACLE[key]


def _check_lags(ctx, F, N, K, n_lags, origins, o_begin=0, o_end=None):
  frames, wv, S_ld, n, tol_s = _lag_oracle(F, N, K, n_lags, origins, o_begin, o_end)
  what = "F=%d N=%d K=%d lags=%d %s [%s, %s)" % (F, N, K, n_lags, origins, o_begin, o_end)
  dev = _dev(frames)
  modes = ctx.density_modes_frames_device(dev, BOX, wv)
  C, counts = ctx.scattering_lags_device(modes, n_lags, origins=origins, o_begin=o_begin, o_end=o_end)
  C_ld, n_o, A = snp.collective(modes.cpu().numpy(), n_lags, o_begin, o_end, origins, LD, absolute=True)      # the GPU's modes as exact inputs
  if o_begin == 0 and o_end is None:
    assert np.array_equal(counts, n_o) and np.array_equal(counts, msd.counts_per_lag(F, 1, n_lags, origins)) and counts.dtype == np.int64
  _sums_within("collective", C.cpu().numpy(), C_ld, snp.collective_bound(n_o, A), what)
  Sf, counts_s = ctx.self_scattering_frames_device(dev, BOX, wv, n_lags, origins=origins, o_begin=o_begin, o_end=o_end)
  assert np.array_equal(n, N * n_o) and np.array_equal(counts_s, counts)
  got = Sf.cpu().numpy()
  _sums_within("self", got, S_ld, tol_s, what)
  assert np.all(got[n == 0] == 0.0) and np.all(C.cpu().numpy()[n_o == 0] == 0.0)      # lags without an origin: exactly zero
  return modes.cpu().numpy(), C.cpu().numpy(), got, n_o, n, tol_s


@pytest.mark.parametrize("n_lags, K, N", LAG_SHAPES)
def test_lag_sums_against_the_long_double_oracle(ctx, n_lags, K, N):
  for F in sorted({1, 2, n_lags - 1, n_lags, n_lags + 5} - {0}):
    for origins in ("window", "all"):
      modes, C, Sf, n_o, n, tol_s = _check_lags(ctx, F, N, K, n_lags, origins)
      if n_o[0] > 0:
        # lag 0: C[0, k] = sum_o |rho_k(o)|^2 and Sf[0, k] = n[0], within the bounds
        sq = (modes[:n_o[0]].astype(LD) ** 2).sum(axis=(0, 2))
        A0 = (modes[:n_o[0]] ** 2).sum(axis=(0, 2))
        assert np.all(np.abs(C[0].astype(LD) - sq).astype(np.float64) <= snp.U * (n_o[0] + 3.0) * A0)
        assert np.all(np.abs(Sf[0] - n[0]) <= tol_s[0])


def test_origin_ranges_and_several_origin_chunks(ctx):
  """600 frames: three staged windows per series; interior and empty origin ranges"""
  _check_lags(ctx, 600, 2, 3, 65, "all")
  _check_lags(ctx, 600, 2, 3, 65, "window")
  _check_lags(ctx, 600, 2, 3, 65, "all", 300, 580)
  _check_lags(ctx, 70, 3, 65, 65, "all", 3, 11)
  frames, wv, _, _ = _modes_oracle(70, 3, 65, 0.0)
  dev = _dev(frames)
  modes = ctx.density_modes_frames_device(dev, BOX, wv)
  out = torch.full((65, 65), 1.5, dtype=torch.float64, device="cuda")
  ctx.scattering_lags_device(modes, 65, origins="all", o_begin=7, o_end=7, out=out)
  ctx.self_scattering_frames_device(dev, BOX, wv, 65, origins="all", o_begin=70, o_end=70, out=out)
  assert torch.all(out == 1.5)


def test_rigid_drift(ctx):
  N, F, n_lags = 5, 70, 66
  wv = snp.mixed_wavevectors(7, seed=3, n_max=4)
  d = np.array([0.031, -0.017, 0.011])
  x0 = snp.random_frames(1, N, BOX, seed=4)[0]
  frames = x0[None] + np.arange(F)[:, None, None] * d
  kd = snp.coefficients(BOX, wv, LD) @ d.astype(LD)
  T = snp.turn_magnitudes(frames, BOX, wv)
  dev = _dev(frames)
  modes = ctx.density_modes_frames_device(dev, BOX, wv)
  C, n_o = ctx.scattering_lags_device(modes, n_lags, origins="all")
  Sf, _ = ctx.self_scattering_frames_device(dev, BOX, wv, n_lags, origins="all")
  C, Sf, rho = C.cpu().numpy(), Sf.cpu().numpy(), modes.cpu().numpy()
  S_ld, n, TT = snp.self_sums(frames, BOX, wv, n_lags, origins="all", dtype=LD, absolute=True)
  # the frames are the drift rounded to double: x0 + f d is off by u |x| per coordinate, a phase error 2 pi u T per factor
  slack = 2 * np.pi * snp.U * TT
  tol_m = snp.modes_bound(N, T.sum(axis=1))      # (F, K)
  for lag in range(n_lags):
    c = np.cos(2 * snp.pi(LD) * lag * kd).astype(np.float64)
    assert np.all(np.abs(Sf[lag] - n[lag] * c) <= snp.self_bound(n, TT)[lag] + slack[lag])
    a, b = rho[:n_o[lag]], rho[lag:lag + n_o[lag]]
    sq = (a ** 2).sum(axis=(0, 2))
    mag = np.sqrt((a ** 2).sum(axis=2))
    # each mode within tol_m of the exact one (and the rounded frames' 2 pi u sum T): first order in the two factors
    dm = np.sqrt(2) * (tol_m + 2 * np.pi * snp.U * T.sum(axis=1))
    first = (mag * dm[lag:lag + n_o[lag]] + np.sqrt((b ** 2).sum(axis=2)) * dm[:n_o[lag]] + 2 * mag * dm[:n_o[lag]]).sum(axis=0)
    assert np.all(np.abs(C[lag] - c * sq) <= first + snp.U * (n_o[lag] + 3.0) * 2 * sq)


def test_same_call_same_bits_out_is_added_to_and_modes_overwritten(ctx):
  frames, wv, _, _ = _modes_oracle(70, 3, 65, 0.0)
  dev = _dev(frames)
  m1 = ctx.density_modes_frames_device(dev, BOX, wv)
  m2 = ctx.density_modes_frames_device(dev, BOX, wv)
  assert torch.equal(m1, m2)
  big, wvb, _, _ = _modes_oracle(1, 20000, 65, 0.0)      # the split path too
  assert torch.equal(ctx.density_modes_frames_device(_dev(big), BOX, wvb), ctx.density_modes_frames_device(_dev(big), BOX, wvb))
  junk = torch.full((70, 65, 2), 7.0, dtype=torch.float64, device="cuda")
  assert ctx.density_modes_frames_device(dev, BOX, wv, out=junk) is junk and torch.equal(junk, m1)      # OVERWRITTEN
  for call in (lambda **kw: ctx.scattering_lags_device(m1, 65, origins="all", **kw),
               lambda **kw: ctx.self_scattering_frames_device(dev, BOX, wv, 65, origins="all", **kw)):
    a, _ = call()
    b, _ = call()
    assert torch.equal(a, b)
    out = torch.full((65, 65), 2.0, dtype=torch.float64, device="cuda")
    c, _ = call(out=out)
    assert c is out and torch.equal(out, a + 2.0)      # ADDED: one addition per entry
    for bad in (torch.zeros((65, 64), dtype=torch.float64, device="cuda"), torch.zeros((65, 65), dtype=torch.float32, device="cuda"),
                torch.zeros((65, 65), dtype=torch.float64), torch.zeros((65, 65), dtype=torch.float64, device="cuda").t()):
      with pytest.raises(ValueError, match="out must be"):
        call(out=bad)
  with pytest.raises(ValueError, match="frames must be"):
    ctx.density_modes_frames_device(dev[..., :2], BOX, wv)
  with pytest.raises(ValueError, match="frames must be"):
    ctx.self_scattering_frames_device(frames, BOX, wv, 3)
  with pytest.raises(ValueError, match="modes must be"):
    ctx.scattering_lags_device(dev, 3)
  with pytest.raises(ValueError, match="wavevectors must be"):
    ctx.density_modes_frames_device(dev, BOX, wv.astype(np.float64))


def test_resident_configuration_is_left_alone():
  """a wall M_tt f of the resident blobs before and after, on the atomic-free sweep (option "deterministic")"""
  from rigidmultiblobswall_amd import MobilityContext
  rng = np.random.RandomState(4)
  r = rng.uniform(0, 6, (500, 3)) + np.array([0, 0, 0.5])
  f = rng.randn(1500)
  frames, wv, _, _ = _modes_oracle(70, 3, 65, 0.0)
  c = MobilityContext(0)
  try:
    c.set_option("deterministic", 1)
    c.set_positions(r, 0.2, wall=True)
    before, again = c.matvec("tt", f, 1.0), c.matvec("tt", f, 1.0)
    assert np.array_equal(before, again)      # the yardstick itself repeats
    dev = _dev(frames)
    modes = c.density_modes_frames_device(dev, BOX, wv)
    c.scattering_lags_device(modes, 65, origins="all")
    c.self_scattering_frames_device(dev, BOX, wv, 65, origins="window")
    torch.cuda.synchronize()
    after = c.matvec("tt", f, 1.0)
    assert np.array_equal(before, after) and c.n == 500
  finally:
    c.close()


@pytest.mark.parametrize("origins", ["window", "all"])
def test_streamed_in_pieces(ctx, origins):
  F, N, K, L = 150, 3, 65, 65
  frames, wv, S_ld, n, tol_s = _lag_oracle(F, N, K, L, origins)
  dev = _dev(frames)
  modes = ctx.density_modes_frames_device(dev, BOX, wv)
  C_ld, n_o, A = snp.collective(modes.cpu().numpy(), L, origins=origins, dtype=LD, absolute=True)
  for pieces in ([1] * 5 + [145], [L - 1, F - L + 1], [1, 5, 70, 74]):
    acc = scattering.IntermediateScattering(N, BOX, wv, n_lags=L, dt=0.25, origins=origins, self_part=True, ctx=ctx)
    start = 0
    for i, size in enumerate(pieces):
      piece = frames[start:start + size]
      acc.add_frames(torch.from_numpy(piece.copy()).cuda() if i % 2 else piece)
      start += size
    assert start == F and [t.shape[0] for t in acc._tail] == [L - 1, L - 1]      # modes and frames: only the incomplete origins are kept
    acc.finish()
    assert np.array_equal(acc.counts(), n_o) and np.array_equal(acc.counts(), msd.counts_per_lag(F, 1, L, origins)) and acc.n_frames == F
    _sums_within("collective", acc.collective_sums(), C_ld, snp.collective_bound(n_o, A), "streamed %s %s" % (origins, pieces))
    _sums_within("self", acc.self_sums(), S_ld, tol_s, "streamed %s %s" % (origins, pieces))
    assert np.array_equal(acc.times(), 0.25 * np.arange(L))
    assert np.array_equal(acc.F(), acc.collective_sums() / (N * n_o.astype(np.float64))[:, None])
    assert np.array_equal(acc.Fs(), acc.self_sums() / (N * n_o.astype(np.float64))[:, None]) and np.array_equal(acc.S(), acc.F()[0])
    with pytest.raises(ValueError, match="after finish"):
      acc.add_frames(frames[:1])
    acc.close()
  assert ctx._h.value      # a caller's context is not closed


def test_structure_factor_and_shells(ctx):
  g = load_golden(os.path.join(GOLDEN, "g17_gr_quasi2d.npz"))
  frames, L = g["frames"], g["periodic_length"]
  wv = scattering.wavevectors(L, n_max=6)
  acc = scattering.IntermediateScattering(frames.shape[1], L, wv, ctx=ctx)
  acc.add_frames(frames).finish()
  S = acc.S()
  rho = snp.modes(frames, L, wv, LD)
  want = ((rho ** 2).sum(axis=(0, 2)) / (frames.shape[0] * frames.shape[1])).astype(np.float64)
  assert np.allclose(S, want, rtol=1e-12, atol=0) and np.array_equal(acc.counts(), [frames.shape[0]])
  with pytest.raises(ValueError, match="self part"):
    acc.Fs()
  k_mean, n_k, values = acc.shells(5)
  knorm = acc.k_norm
  assert np.allclose(knorm, np.linalg.norm(2 * np.pi * wv[:, :2] / L[:2], axis=1), rtol=1e-15)
  idx = np.minimum((knorm / knorm.max() * 5).astype(int), 4)
  for b in range(5):
    assert n_k[b] == np.sum(idx == b)
    assert np.isclose(values[b], S[idx == b].mean(), rtol=1e-14) and np.isclose(k_mean[b], knorm[idx == b].mean(), rtol=1e-14)
  assert n_k.sum() == len(wv)
  acc.close()


def test_multi_device_context_refuses(ctx):
  from rigidmultiblobswall_amd.multi import MultiContext
  m = MultiContext([0])
  try:
    assert not hasattr(m, "density_modes_frames_device")
    with pytest.raises(ValueError, match="single-GPU MobilityContext"):
      scattering.IntermediateScattering(2, BOX, np.array([[1, 0, 0]]), ctx=m)
  finally:
    m.close()


def test_command_line(ctx, tmp_path):
  L = (6.0, 4.5, 0.0)
  frames = snp.random_frames(40, 5, L, seed=77)
  traj = tmp_path / "run.config"
  traj.write_text(snp.config_text(frames))
  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
  argv = [str(traj), "5", "6.0", "4.5", "0", "--nmax", "2", "--lags", "9", "--dt", "0.5", "--every", "2", "--skip", "3", "--origins", "all", "--self"]
  out = subprocess.run([sys.executable, "-m", "rigidmultiblobswall_amd.scattering"] + argv, check=True, capture_output=True, text=True, env=env,
                       timeout=300).stdout
  blocks = snp.parse_output(out)
  used = frames[3::2]
  wv = scattering.wavevectors(L, n_max=2)
  rho = snp.modes(used, L, wv, LD)
  C, n_o = snp.collective(rho, 9, origins="all", dtype=LD)
  Sf, n = snp.self_sums(used, L, wv, 9, origins="all", dtype=LD)
  k = scattering.k_vectors(L, wv)
  assert len(blocks) == 9
  for lag, (t, count, rows) in enumerate(blocks):
    assert t == 1.0 * lag and count == n_o[lag] and rows.shape == (len(wv), 6)
    assert np.array_equal(rows[:, :3], k) and np.array_equal(rows[:, 3], np.sqrt((k ** 2).sum(axis=1)))
    F_want, Fs_want = (C[lag] / (5 * n_o[lag])).astype(np.float64), (Sf[lag] / n[lag]).astype(np.float64)
    scale = np.abs(rho).max() ** 2 / 5      # F(k, t) near a zero crossing: relative to the scale of the sum's terms
    assert np.all(np.abs(rows[:, 4] - F_want) <= 1e-12 * max(scale, 1.0)) and np.all(np.abs(rows[:, 5] - Fs_want) <= 1e-12)
  # write() gives the same text; the module's main() in this process: the plain structure factor with shells
  acc =scattering.IntermediateScattering(5, L, wv, n_lags=9, dt=1.0, origins="all", self_part=True, ctx=ctx)
  acc.add_frames(used).finish().write(str(tmp_path / "f.txt"))
  assert (tmp_path / "f.txt").read_text() == out
  acc.close()
  buf = io.StringIO()
  assert scattering.main([str(traj), "5", "6.0", "4.5", "0", "--kmax", "3.0", "--shells", "4"], out=buf) == 0
  (t, count, rows), = snp.parse_output(buf.getvalue())
  wk = scattering.wavevectors(L, k_max=3.0)
  rho = snp.modes(frames, L, wk, LD)
  S = ((rho ** 2).sum(axis=(0, 2)) / (40 * 5)).astype(np.float64)
  k_mean, n_k, want = scattering.shell_average(np.linalg.norm(scattering.k_vectors(L, wk), axis=1), S, 4)
  assert t is None and rows.shape == (4, 3) and np.array_equal(rows[:, 1], n_k)
  assert np.allclose(rows[:, 0], k_mean, rtol=1e-15, equal_nan=True) and np.allclose(rows[:, 2], want, rtol=1e-12, equal_nan=True)


def test_bad_arguments_raise(ctx):
  """every RMB_ERR_ARG case of the header, with a live context"""
  lib = _lib.load()
  buf, L, wv = torch.zeros(64, dtype=torch.float64, device="cuda"), np.array([4.0, 3.0, 0.0]), np.array([[1, 0, 0], [1, -2, 0]], dtype=np.int32)
  out = torch.zeros(64, dtype=torch.float64, device="cuda")
  big = np.zeros((16385, 3), dtype=np.int32)
  p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
  good = dict(frames=ctypes.c_void_p(buf.data_ptr()), n_frames=3, n=2, L=p(L), kint=p(wv), K=2, n_lags=2, o_begin=0, o_end=2,
              out=ctypes.c_void_p(out.data_ptr()))
  wv_n, wv_z, L_x = np.array([[1, 0, 0], [-32769, 0, 0]], dtype=np.int32), np.array([[1, 0, -1]], dtype=np.int32), np.array([0.0, 3.0, 2.0])
  sizes = [dict(n_frames=-1), dict(K=-1), dict(K=16385, kint=p(big))]
  waves = [dict(n=-1), dict(L=None), dict(kint=None), dict(kint=p(wv_n)), dict(kint=p(wv_z), K=1), dict(L=p(L_x)), dict(frames=None)]
  lags = [dict(n_lags=0), dict(o_end=4), dict(o_begin=-1), dict(o_begin=2, o_end=1)]
  calls = {
      "rmb_density_modes_frames_device": (lambda a: (a["frames"], a["n_frames"], a["n"], a["L"], a["kint"], a["K"], a["out"]),
                                          sizes + waves + [dict(out=None)]),
      "rmb_scattering_lags_device": (lambda a: (a["frames"], a["n_frames"], a["K"], a["n_lags"], a["o_begin"], a["o_end"], a["out"]),
                                     sizes + lags + [dict(frames=None), dict(out=None)]),
      "rmb_self_scattering_frames_device": (lambda a: (a["frames"], a["n_frames"], a["n"], a["L"], a["kint"], a["K"], a["n_lags"], a["o_begin"],
                                                       a["o_end"], a["out"]), sizes + waves + lags + [dict(out=None)]),
  }
  for name, (args, bad) in calls.items():
    fn = getattr(lib, name)
    for change in bad:
      with pytest.raises(_lib.RmbError, match="error -1"):
        _lib.check(fn(ctx._h, *args(dict(good, **change))))
    _lib.check(fn(ctx._h, *args(good)))      # and the call they were derived from is in order
  torch.cuda.synchronize()
  # through the context: the same refusals
  dev = torch.zeros((3, 2, 3), dtype=torch.float64, device="cuda")
  with pytest.raises(_lib.RmbError, match="32768"):
    ctx.density_modes_frames_device(dev, L, np.array([[40000, 0, 0]]))
  with pytest.raises(_lib.RmbError, match="positive length"):
    ctx.self_scattering_frames_device(dev, L, np.array([[0, 0, 1]]), 2)
  with pytest.raises(ValueError, match="n_lags"):
    ctx.scattering_lags_device(torch.zeros((3, 2, 2), dtype=torch.float64, device="cuda"), 0)
  with pytest.raises(_lib.RmbError, match="o_begin <= o_end"):
    ctx.scattering_lags_device(torch.zeros((3, 2, 2), dtype=torch.float64, device="cuda"), 2, origins="all", o_begin=2, o_end=5)


def test_empty_inputs(ctx):
  wv = snp.mixed_wavevectors(5, seed=1)
  none = np.zeros((0, 3), dtype=np.int32)
  z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")      # noqa: E731
  marked = lambda *shape: torch.full(shape, 1.5, dtype=torch.float64, device="cuda")      # noqa: E731
  # n = 0: zero modes, nothing added to the self sums
  out = marked(4, 5, 2)
  assert torch.all(ctx.density_modes_frames_device(z(4, 0, 3), BOX, wv, out=out) == 0.0)
  out = marked(3, 5)
  ctx.self_scattering_frames_device(z(4, 0, 3), BOX, wv, 3, origins="all", out=out)
  assert torch.all(out == 1.5)
  # n_frames = 0, K = 0, o_begin = o_end: the lag sums stay
  ctx.self_scattering_frames_device(z(0, 7, 3), BOX, wv, 3, origins="all", out=out)
  ctx.scattering_lags_device(z(0, 5, 2), 3, origins="all", out=out)
  ctx.scattering_lags_device(z(2, 5, 2) + 1.0, 3, origins="window", out=out)      # fewer frames than lags: no window origin
  ctx.scattering_lags_device(z(6, 5, 2) + 1.0, 3, origins="all", o_begin=4, o_end=4, out=out)
  assert torch.all(out == 1.5)
  assert tuple(ctx.density_modes_frames_device(z(4, 7, 3), BOX, none).shape) == (4, 0, 2)
  assert tuple(ctx.density_modes_frames_device(z(0, 7, 3), BOX, wv).shape) == (0, 5, 2)
  s, n = ctx.scattering_lags_device(z(4, 0, 2), 3, origins="all")
  assert tuple(s.shape) == (3, 0) and np.array_equal(n, [4, 3, 2])
  s, _ = ctx.self_scattering_frames_device(z(4, 7, 3), BOX, none, 3)
  assert tuple(s.shape) == (3, 0)
