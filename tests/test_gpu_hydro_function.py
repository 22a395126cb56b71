"""The HIP hydrodynamic-function sweep (rmb_hydro_function_frames_device, rmb_hydro_function_device, hydro_function_kernels.h)
against the long-double restatement and the bound of tests/_hydro_function_numpy.py (its docstring derives the bound; the host
test shows that plain fp64 numpy meets it), against the product the engine already has, and against closed forms.

One long-double evaluation per boundary of the largest trajectory (3 frames x 200 points x 19 wavevectors) serves every
smaller shape: the block of a pair does not depend on the other points.

The identity test compares S_self + S_dist with v_c . (M v_c) + v_s . (M v_s), v_c[i] = e cos(theta_i), v_s[i] = e sin(theta_i),
from ctx.matvec("tt", ...).  Its tolerance is the sum of the two routes' bounds.  The product's route, u = 2^-53: an element of
a block is off by at most 4 C u s_ij and meets |v_a| <= |e_a|, sum_ab |e_a| |e_b| <= 3; an entry of v_c, v_s carries the phase
error u (C0 + C1 T_i) of its point; the sums of the product and of the dot product pass through at most 2 N + 64 additions of
terms of size at most 2 s_ij.  Together 3 u sum_ij s_ij [4 C + 2 C0 + C1 (T_i + T_j) + 2 (2 N + 64)]."""
import io

import numpy as np
import pytest
import torch

import _hydro_function_numpy as hn
import _mobility_numpy as mn
import _scattering_numpy as sn
from _mobility_numpy import EXT
from rigidmultiblobswall_amd import hydrofunction as hf
from rigidmultiblobswall_amd._lib import RmbError

pytestmark = pytest.mark.gpu

A, ETA = hn.A, hn.ETA
KC = 8
N_LIST = (1, 2, 63, 64, 65, 129, 200)
K_LIST = (1, KC, KC + 1, 2 * KC + 3)
CHUNK_STEPS = (0, 4, 28, 1024)
OVERSUB = (1, 8)
DEFAULTS = {"sym_chunk_steps": 1024, "sym_oversub": 8}
MU0 = 1.0 / (6.0 * np.pi * ETA * A)
WORST = {}


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  assert {k: c.get_option(k) for k in DEFAULTS} == DEFAULTS
  yield c
  c.close()


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _run(ctx, ref, n, K, F, out=None):
  frames = _dev(ref["frames"][:F, :n])
  got = ctx.hydrodynamic_function_frames_device(frames, A, ETA, ref["L"], ref["kint"][:K], ref["pol"][:K], wall=ref["boundary"] == "wall",
                                                mobility_periodic_length=ref["mob_L"], out=out)
  return got.cpu().numpy()


def _check(label, got, S, B):
  assert got.shape == S.shape and np.all(np.isfinite(got)), label
  err = np.abs(got.astype(EXT) - S).astype(np.float64)
  ok = (err <= B)
  ratio = float(np.max(err / np.where(B > 0, B, 1.0)))
  WORST[label] = max(WORST.get(label, 0.0), ratio)
  assert np.all(ok), "%s: worst error / bound %.3g at %r" % (label, ratio, np.unravel_index(np.argmax(err / np.where(B > 0, B, 1.0)), err.shape))
  return ratio


# ---- against the long-double restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(hn.CASES))
def test_against_the_long_double_restatement(ctx, case):
  ref = hn.reference(case)
  assert hn.K_MAX == K_LIST[-1] and ref["frames"].shape[:2] == (3, N_LIST[-1])
  worst = 0.0
  for n in N_LIST:
    for K in K_LIST:
      for F in (1, 3):
        S, B = hn.expected(ref, n, K, F)
        worst = max(worst, _check(case, _run(ctx, ref, n, K, F), S, B))
  print("hydrodynamic function %-14s worst error / bound %.4f over %d shapes" % (case, worst, len(N_LIST) * len(K_LIST) * 2))


def test_a_thousand_periods_away(ctx):
  ref = hn.reference("wall_periodic", 1000.0)
  assert ref["frames"][..., 0].min() > 999.0 * ref["L"][0]
  worst = 0.0
  for n, K in ((65, KC + 1), (200, 2 * KC + 3)):
    S, B = hn.expected(ref, n, K, 3)
    worst = max(worst, _check("wall_periodic + 1000 L", _run(ctx, ref, n, K, 3), S, B))
  print("hydrodynamic function 1000 periods away: worst error / bound %.4f" % worst)


class _plan:
  def __init__(self, ctx, chunk_steps, oversub):
    self.ctx, self.values = ctx, {"sym_chunk_steps": chunk_steps, "sym_oversub": oversub}

  def __enter__(self):
    for k, v in self.values.items():
      self.ctx.set_option(k, v)

  def __exit__(self, *exc):
    for k, v in DEFAULTS.items():
      self.ctx.set_option(k, v)


@pytest.mark.parametrize("case", ("wall_open", "none_periodic"))
def test_launch_plans(ctx, case):
  """a pair is met exactly once whatever the chunks are: at a chunk edge inside a unit, at the peeled step, at a frame's edge"""
  ref = hn.reference(case)
  K = 2 * KC + 3
  worst = 0.0
  for n in (65, 129, 200):
    S, B = hn.expected(ref, n, K, 3)
    for chunk in CHUNK_STEPS:
      for over in OVERSUB:
        with _plan(ctx, chunk, over):
          got = _run(ctx, ref, n, K, 3)
        worst = max(worst, _check("plans " + case, got, S, B))
  assert {k: ctx.get_option(k) for k in DEFAULTS} == DEFAULTS
  print("hydrodynamic function launch plans %-14s worst error / bound %.4f" % (case, worst))


@pytest.mark.parametrize("case", list(hn.CASES))
def test_resident_entry(ctx, case):
  """the resident configuration, packed by set_positions, through the same kernel as one frame"""
  ref = hn.reference(case)
  for n, K in ((65, KC + 1), (200, 2 * KC + 3)):
    ctx.set_positions(ref["frames"][0, :n], A, ref["mob_L"], ref["boundary"] == "wall")
    got = ctx.hydrodynamic_function(ETA, ref["L"], ref["kint"][:K], ref["pol"][:K])
    S, B = hn.expected(ref, n, K, 1)
    _check("resident " + case, got[None], S, B)


# ---- identity with the product the engine already has -------------------------------------------------------------------
def _row_sums(r, a, eta, mob_L, wall):
  """sum_j s_ij of _mobility_numpy.scale("tt", ...) in float64, rows in blocks (4096^2 long doubles would not be quick)"""
  r = np.asarray(r, dtype=np.float64)
  z = np.where(r[:, 2] <= a, a, r[:, 2]) if wall else r[:, 2]
  b = np.abs(np.where(r[:, 2] < a, r[:, 2] / a, 1.0)) if wall else np.ones(len(r))
  L = np.zeros(3) if mob_L is None else np.asarray(mob_L, dtype=np.float64)
  boxes = [(bx, by) for bx in ((-1, 0, 1) if L[0] > 0 else (0,)) for by in ((-1, 0, 1) if L[1] > 0 else (0,))]
  out = np.zeros(len(r))
  for i0 in range(0, len(r), 512):
    d = r[i0:i0 + 512, None, :2] - r[None, :, :2]
    for k in range(2):
      if L[k] > 0:
        d[..., k] -= np.trunc(d[..., k] / L[k] + 0.5 * np.sign(d[..., k])) * L[k]
    dz2, Rz2 = (z[i0:i0 + 512, None] - z[None, :]) ** 2, (z[i0:i0 + 512, None] + z[None, :]) ** 2
    s = np.zeros(d.shape[:2])
    for bx, by in boxes:
      rho2 = (d[..., 0] + bx * L[0]) ** 2 + (d[..., 1] + by * L[1]) ** 2
      s += 1.0 / np.maximum(np.sqrt(rho2 + dz2), a)
      if wall:
        s += 1.0 / np.sqrt(rho2 + Rz2)
    out[i0:i0 + 512] = (s * b[None, :]).sum(axis=1) * b[i0:i0 + 512]
  return out / (8.0 * np.pi * eta)


@pytest.mark.parametrize("periodic", (False, True))
def test_identity_with_the_product(ctx, periodic):
  """catches a wrong convention: clamp, damping, images, transpose"""
  n, K = 4096, 32
  box = np.array([96.0, 80.0, 0.0])
  rng = np.random.RandomState(41)
  r = rng.uniform(0, 1, (n, 3)) * np.array([box[0], box[1], 3.0 * A])      # a monolayer; a sixth of the blobs below z = a (damped)
  r[:, 2] -= 0.1 * A                                                        # and a few below the wall
  mob_L = box if periodic else None
  L = np.array([box[0], box[1], 9.0])
  kint = sn.mixed_wavevectors(K, 17, n_max=7, plane="xyz")
  e = rng.standard_normal((K, 3))
  e /= np.sqrt((e * e).sum(axis=1))[:, None]
  got = ctx.hydrodynamic_function_frames_device(_dev(r[None]), A, ETA, L, kint, e, wall=True, mobility_periodic_length=mob_L).cpu().numpy()[0]
  ctx.set_positions(r, A, mob_L, True)
  theta = 2.0 * np.pi * sn.reduced_turns(r[None], L, kint)[0]               # (n, K), float64
  other = np.zeros(K)
  for m in range(K):
    for trig in (np.cos, np.sin):
      v = (trig(theta[:, m])[:, None] * e[m][None, :]).reshape(-1)
      other[m] += float(np.dot(v, ctx.matvec("tt", v, ETA)))
  rows = _row_sums(r, A, ETA, mob_L, True)
  T = sn.turn_magnitudes(r[None], L, kint)[0]
  C = mn.C_ORACLE["tt", "wall", periodic]
  total, phase = rows.sum(), 2.0 * sn.C1 * (T * rows[:, None]).sum(axis=0)      # sum_ij s_ij (T_i + T_j): s is symmetric
  bound_sweep = hn.U * ((4.0 * C + 2.0 * sn.C0 + hn.c_sum(n)) * total + phase)
  bound_product = 3.0 * hn.U * ((4.0 * C + 2.0 * sn.C0 + 2.0 * (2.0 * n + 64.0)) * total + phase)
  err = np.abs(got.sum(axis=1) - other)
  print("identity with the product, periodic %s: worst difference / (sum of the bounds) %.4f; H between %.3f and %.3f" %
        (periodic, float(np.max(err / (bound_sweep + bound_product))), float(got.sum(axis=1).min() / (n * MU0)), float(got.sum(axis=1).max() / (n * MU0))))
  assert np.all(err <= bound_sweep + bound_product)
  assert np.all(np.abs(got.sum(axis=1)) > 1e6 * (bound_sweep + bound_product))      # the comparison has digits to lose


# ---- closed forms ----------------------------------------------------------------------------------------------------
def test_two_distant_blobs_without_wall(ctx):
  d = np.array([30.0 * A, -40.0 * A, 120.0 * A])      # r = 130 a
  r = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]) + np.array([np.zeros(3), d])
  L = np.array([50.0, 60.0, 70.0])
  kint = np.array([[1, 0, 0], [2, -1, 3], [0, 0, 5]], dtype=np.int32)
  e = np.array([[1.0, 0.0, 0.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])
  S = ctx.hydrodynamic_function_frames_device(_dev(r[None]), A, ETA, L, kint, e, wall=False).cpu().numpy()[0]
  H = S.sum(axis=1) / (2.0 * MU0)
  dist = np.linalg.norm(d)
  k = 2.0 * np.pi * kint / L
  q = (A / dist) ** 2
  want = 1.0 + (3.0 * A / (4.0 * dist)) * ((1.0 + 2.0 * q / 3.0) + (1.0 - 2.0 * q) * (e @ (d / dist)) ** 2) * np.cos(-(k @ d))
  assert np.allclose(H, want, rtol=0, atol=1e-14), (H, want)
  assert np.allclose(S[:, 0] / (2.0 * MU0), 1.0, rtol=0, atol=4e-16)


def test_one_blob_above_the_wall(ctx):
  h = 1.7 * A
  r = np.array([[0.3, -0.2, h]])
  ctx.set_positions(r, A, None, True)
  dense = ctx.body_mobility_dense_device(torch.zeros(1, dtype=torch.int64, device="cuda"), 1, ETA)[0].cpu().numpy().reshape(3, 3)
  kint = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.int32)
  e = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
  S = ctx.hydrodynamic_function_frames_device(_dev(r[None]), A, ETA, (10.0, 10.0, 0.0), kint, e, wall=True).cpu().numpy()[0]
  assert np.all(S[:, 1] == 0.0)
  assert np.allclose(S[:, 0], [dense[0, 0], dense[2, 2]], rtol=4e-16, atol=0), (S, dense)
  x = A / h      # the textbook expansions of the wall's self mobility, parallel and vertical
  assert np.allclose(S[:, 0] / MU0, [1 - 9 * x / 16 + x ** 3 / 8 - x ** 5 / 16, 1 - 9 * x / 8 + x ** 3 / 2 - x ** 5 / 8], rtol=1e-14)


def test_zero_wavevector_is_the_product(ctx):
  ref = hn.reference("wall_open")
  n = 200
  r = ref["frames"][0]
  e = np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])
  kint = np.zeros((2, 3), dtype=np.int32)
  S = ctx.hydrodynamic_function_frames_device(_dev(r[None]), A, ETA, ref["L"], kint, e, wall=True).cpu().numpy()[0]
  ctx.set_positions(r, A, None, True)
  s, w = ref["per"][0][2], ref["per"][0][3]
  C = mn.C_ORACLE["tt", "wall", False]
  for m in range(2):
    v = np.tile(e[m], n)
    want = float(np.dot(v, ctx.matvec("tt", v, ETA)))
    bound = hn.U * (4.0 * C + 2.0 * sn.C0 + hn.c_sum(n)) * s.sum() + 3.0 * hn.U * (4.0 * C + 2.0 * (2.0 * n + 64.0)) * s.sum()
    assert abs(S[m].sum() - want) <= bound, (m, S[m].sum(), want, bound)
    assert abs(want) > 1e6 * bound


# ---- bits, streams, state ----------------------------------------------------------------------------------------------
def test_same_call_same_bits_and_nothing_else_touched(ctx):
  from rigidmultiblobswall_amd import MobilityContext
  ref = hn.reference("wall_periodic")
  r0 = ref["frames"][1, :129]
  own = MobilityContext(0)
  try:      # the yardstick: a wall M_tt f of the resident blobs on the atomic-free sweep (option "deterministic"), before and after
    own.set_option("deterministic", 1)
    own.set_positions(r0, A, None, True)
    v = np.random.RandomState(2).standard_normal(3 * 129)
    before, again = own.matvec("tt", v, ETA), own.matvec("tt", v, ETA)
    assert np.array_equal(before, again)
    first = _run(own, ref, 200, 2 * KC + 3, 3)
    torch.cuda.synchronize()
    assert np.array_equal(own.matvec("tt", v, ETA), before) and own.n == 129      # neither read nor written
  finally:
    own.close()
  out = torch.full((3, 2 * KC + 3, 2), float("nan"), dtype=torch.float64, device="cuda")
  a = _run(ctx, ref, 200, 2 * KC + 3, 3, out=out)
  assert np.all(np.isfinite(a)) and np.array_equal(a, out.cpu().numpy())      # overwritten, every entry
  out.fill_(7.0)
  b = _run(ctx, ref, 200, 2 * KC + 3, 3, out=out)
  assert np.array_equal(a, b)
  assert np.array_equal(_run(ctx, ref, 200, 2 * KC + 3, 3), a)
  assert np.array_equal(first, a)                                             # another context, the same plan, the same bits
  # a frame's sums do not depend on the frames around it
  assert np.array_equal(_run(ctx, ref, 200, 2 * KC + 3, 1)[0], a[0])


def test_streamed_class_does_not_depend_on_the_cut(ctx):
  ref = hn.reference("wall_periodic")
  rng = np.random.RandomState(5)
  frames = np.concatenate([ref["frames"][:, :65], ref["frames"][:, :65] + 0.02 * A * rng.standard_normal((3, 65, 3)), ref["frames"][:1, :65] + 0.05 * A])
  assert frames.shape == (7, 65, 3)
  wv = np.array([[1, 0, 0], [0, 1, 0], [2, 1, 0], [3, -2, 0]], dtype=np.int32)
  L = (ref["L"][0], ref["L"][1], 0.0)

  def run(cuts):
    acc = hf.HydrodynamicFunction(65, L, wv, A, ETA, ctx=ctx)
    k = 0
    for c in cuts:
      acc.add_frames(frames[k:k + c] if c % 2 else _dev(frames[k:k + c]))      # numpy and device pieces
      k += c
    acc.finish()
    with pytest.raises(ValueError, match="after finish"):
      acc.add_frames(frames[:1])
    res = [acc.H(), acc.H_self(), acc.H_distinct(), acc.stderr()]
    assert acc.n_frames == 7
    acc.close()
    return res
  whole = run((7,))
  for cuts in ((1, 6), (3, 4)):
    for x, y in zip(run(cuts), whole):
      assert np.array_equal(x, y), cuts
  assert ctx._h.value      # a borrowed context is not closed
  # the means are the kernel's sums, normalised
  S = ctx.hydrodynamic_function_frames_device(_dev(frames), A, ETA, L, wv, hf.polarisations(L, wv), wall=True,
                                              mobility_periodic_length=(L[0], L[1], 0.0)).cpu().numpy()
  assert np.allclose(whole[0], S.sum(axis=2).mean(axis=0) / (65 * MU0), rtol=1e-14)
  assert np.all(whole[1] > 0) and np.all(whole[1] < 1) and np.all(whole[3] > 0)


# ---- refusals and empty inputs -----------------------------------------------------------------------------------------
def test_refusals_and_empty_inputs(ctx):
  ref = hn.reference("wall_open")
  frames, L, kint, pol = _dev(ref["frames"][:2, :65]), ref["L"], ref["kint"][:3], ref["pol"][:3]
  f = ctx.hydrodynamic_function_frames_device
  with pytest.raises(RmbError, match="mobility's period must equal the wavevector length"):
    f(frames, A, ETA, L, kint, pol, mobility_periodic_length=(L[0], 2.0 * L[1], 0.0))
  with pytest.raises(RmbError, match="needs a positive length"):
    f(frames, A, ETA, (L[0], L[1], 0.0), kint, pol)
  with pytest.raises(RmbError, match="radius must be positive"):
    f(frames, 0.0, ETA, L, kint, pol)
  with pytest.raises(RmbError, match="eta must be positive"):
    f(frames, A, -1.0, L, kint, pol)
  with pytest.raises(ValueError, match="no in_plane variant"):
    f(frames, A, ETA, L, kint, pol, in_plane=True)
  with pytest.raises(ValueError, match="pair shards"):
    f(frames, A, ETA, L, kint, pol, shard=1, nshards=2)
  with pytest.raises(ValueError, match="per-blob radii"):
    f(frames, np.full(65, A), ETA, L, kint, pol)
  with pytest.raises(ValueError, match="not 'free_surface'"):
    f(frames, A, ETA, L, kint, pol, wall="free_surface")
  with pytest.raises(ValueError, match=r"shape \(n_frames, K, 2\)"):
    f(frames, A, ETA, L, kint, pol, out=torch.zeros((2, 3), dtype=torch.float64, device="cuda"))
  with pytest.raises(ValueError, match="longitudinal polarisation of n = 0"):
    hf.HydrodynamicFunction(65, L, np.zeros((1, 3), dtype=np.int32), A, ETA, ctx=ctx)
  from rigidmultiblobswall_amd.multi import MultiContext
  multi = MultiContext([0])
  try:
    with pytest.raises(ValueError, match="single-GPU MobilityContext, got 'MultiContext'"):
      hf.HydrodynamicFunction(65, L, kint, A, ETA, polarisation=pol, ctx=multi)
  finally:
    multi.close()
  # precision = 32, a free-surface configuration, a target sub-range: their own context
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  try:
    with pytest.raises(RmbError, match="rmb_set_positions has not been called"):
      c.hydrodynamic_function(ETA, L, kint, pol)
    c.set_option("precision", 32)
    with pytest.raises(RmbError, match="fp64 only"):
      c.hydrodynamic_function_frames_device(frames, A, ETA, L, kint, pol)
    c.set_positions(ref["frames"][0, :65], A, None, True)
    with pytest.raises(RmbError, match="fp64 only"):
      c.hydrodynamic_function(ETA, L, kint, pol)
    c.set_option("precision", 64)
    c.set_target_range(0, 32)
    with pytest.raises(RmbError, match="reset the target range"):
      c.hydrodynamic_function(ETA, L, kint, pol)
    c.set_target_range(0, 65)
    assert c.hydrodynamic_function(ETA, L, kint, pol).shape == (3, 2)
    with pytest.raises(RmbError, match="mobility's period must equal the wavevector length"):
      c.set_positions(ref["frames"][0, :65], A, (2.0 * L[0], 0.0, 0.0), True)
      c.hydrodynamic_function(ETA, L, kint, pol)
    c.set_positions(ref["frames"][0, :65] + np.array([0.0, 0.0, 2.0 * A]), A, None, "free_surface")
    with pytest.raises(RmbError, match="no free-surface configurations"):
      c.hydrodynamic_function(ETA, L, kint, pol)
  finally:
    c.close()
  # empty inputs
  assert tuple(f(frames[:0], A, ETA, L, kint, pol).shape) == (0, 3, 2)
  assert tuple(f(frames, A, ETA, L, kint[:0], pol[:0]).shape) == (2, 0, 2)
  assert ctx.hydrodynamic_function(ETA, L, kint[:0], pol[:0]).shape == (0, 2)


# ---- command line ----------------------------------------------------------------------------------------------------
def test_command_line(ctx, tmp_path):
  ref = hn.reference("wall_periodic")
  frames = ref["frames"][:, :65]
  traj = tmp_path / "run.config"
  traj.write_text(sn.config_text(frames))
  base = [str(traj), "65", "%.17g" % ref["L"][0], "%.17g" % ref["L"][1], "0", "--radius", "%.17g" % A, "--eta", "%.17g" % ETA, "--nmax", "2"]
  buf = io.StringIO()
  assert hf.main(base, out=buf) == 0
  rows = np.array([[float(x) for x in line.split()] for line in buf.getvalue().splitlines()])
  wv = hf._wavevectors((ref["L"][0], ref["L"][1], 0.0), n_max=2, plane="xy")
  assert rows.shape == (len(wv), 8) and len(wv) == 12
  assert np.allclose(rows[:, 6], rows[:, 4] + rows[:, 5], rtol=4e-16) and np.all(rows[:, 7] > 0)
  assert np.allclose(rows[:, 3], np.linalg.norm(rows[:, :3], axis=1), rtol=1e-15)
  acc = hf.HydrodynamicFunction(65, (ref["L"][0], ref["L"][1], 0.0), wv, A, ETA, ctx=ctx).add_frames(frames).finish()
  assert acc.format() == buf.getvalue()
  buf2 = io.StringIO()
  assert hf.main(base + ["--with-S"], out=buf2) == 0
  rows2 = np.array([[float(x) for x in line.split()] for line in buf2.getvalue().splitlines()])
  assert rows2.shape == (len(wv), 10) and np.array_equal(rows2[:, :8], rows)
  rho = sn.modes(frames, (ref["L"][0], ref["L"][1], 0.0), wv)
  assert np.allclose(rows2[:, 8], (rho ** 2).sum(axis=2).mean(axis=0) / 65.0, rtol=1e-12)
  assert np.allclose(rows2[:, 9], rows2[:, 6] / rows2[:, 8], rtol=4e-16)
  buf3 = io.StringIO()
  assert hf.main(base + ["--shells", "3", "--no-wall", "--open", "--polarisation", "transverse"], out=buf3) == 0
  assert np.array([line.split() for line in buf3.getvalue().splitlines()]).shape == (3, 6)
  acc.close()
  for label in sorted(WORST):      # the figures of profiles/r32_hydro_function_bounds.txt (run the file with -s)
    print("worst error / bound  %-28s %.4f" % (label, WORST[label]))
