"""Body-body Yukawa energy on the device: the energy sweep over body centres (rmb_body_body_potential) against the long-double
restatement (_body_forces_numpy.energy), bound |U_hip - U_ref| <= 1e-13 S with S = sum|terms| = U_ref (every term is positive)
-- the bound test_gpu_potential.py states for energies; the centre term of the single-body difference
(rmb_mcmc_body_delta_bb_device), bound 1e-13 sum(|new| + |old|); and the sampler with body_potential= against its numpy twin,
both move kinds."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _body_forces_numpy as bfn
import _potential_numpy as potnp
from conftest import ROOT
from _mcmc_moves_common import (deck_of, delta_rule, energy_fn, layout, potential_kw, quaternion_of_rotation_vector, quaternion_product,
                                write_deck)
from rigidmultiblobswall_amd.read_input import ReadInput

pytestmark = pytest.mark.gpu

EXT = potnp.EXT
BOUND = 1e-13
EPS, B = 1.7, 0.9
WORST = {"energy": 0.0, "delta": 0.0}     # largest error / scale seen by this module (printed at teardown; DESIGN 3.9 quotes them)
_ORACLE = {}


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()
  print("worst |U_hip - U_ref| / U_ref of this module = %.3e, worst |d_hip - d_ref| / sum(|new| + |old|) = %.3e (bound %.1e)" %
        (WORST["energy"], WORST["delta"], BOUND))


def _oracle(key, x, L):
  """The long-double energy, computed once per (cloud, box)."""
  key = (key, tuple(float(v) for v in L))
  if key not in _ORACLE:
    _ORACLE[key] = bfn.energy(x, L, EPS, B)
  return _ORACLE[key]


def _hip(ctx, x, L):
  ctx.set_positions(x, 1.0, L, wall=False)
  return ctx.body_body_potential(EPS, B)


def _check_energy(got, ref, what):
  ratio = float(abs(EXT(got) - ref) / ref) if ref > 0 else abs(got)
  WORST["energy"] = max(WORST["energy"], ratio)
  print("%s U_hip %.15e  U_ref %.15e  ratio %.3e" % (what, got, float(ref), ratio))
  assert abs(EXT(got) - ref) <= BOUND * ref, (what, got, float(ref))


# n = 2: the seed is the first for which the two lattice points lie more than half a box apart in z, so that the z image acts
CLOUD_SEED = {1: 1, 2: 2, 65: 65, 257: 257, 2049: 2049}


def _cloud(n):
  return bfn.lattice_cloud(n, CLOUD_SEED[n])


# ---- 1. energy parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [False, True], ids=["open", "xyz"])
@pytest.mark.parametrize("n", [1, 2, 65, 257, 2049])
def test_energy_parity(ctx, n, periodic):
  """1: no pair, exactly 0; 2: one pair; 65: straddles a wave; 257: second workgroup; 2049: the Morton sort starts at 2048."""
  x, box = _cloud(n)
  L = np.array([box, box, box]) if periodic else np.zeros(3)
  ref = _oracle(n, x, L)
  if periodic and n > 1:      # an x,y-only image fails this test
    flat = _oracle(n, x, np.array([box, box, 0.0]))
    print("n %d: U(Lz = box) - U(Lz = 0) = %.3e = %.3e of the bound" % (n, float(ref - flat), float(abs(ref - flat) / (BOUND * ref))))
    assert abs(ref - flat) > 1000 * BOUND * ref
  got = _hip(ctx, x, L)
  if n == 1:
    assert got == 0.0 and ref == 0
  else:
    _check_energy(got, ref, "n %d %s" % (n, "xyz" if periodic else "open"))
  dev = ctx.body_body_potential_device(EPS, B)
  out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda:0")
  assert ctx.body_body_potential_device(EPS, B, out=out) is out
  assert float(dev.item()) == got == float(out.item())


# ---- 2. no wall gate ---------------------------------------------------------------------------------------------------------
def test_centres_behind_the_wall_count_in_full(ctx):
  x, box = _cloud(257)
  x = x.copy()
  x[:, 2] -= np.median(x[:, 2])
  assert (x[:, 2] <= 0).sum() > 60 and (x[:, 2] > 0).sum() > 60
  L = np.zeros(3)
  ref = bfn.energy(x, L, EPS, B)
  got = _hip(ctx, x, L)
  _check_energy(got, ref, "257 centres astride z = 0")
  u_one, u_pair = ctx.blob_potential(EPS, B, 1.0, potential="yukawa")
  print("blob yukawa form on the same points: U_pair %.6e (the centres' %.6e), U_one %.6e" % (u_pair, got, u_one))
  assert abs(u_pair - got) > 1000 * BOUND * ref and u_one > 1e5      # gated pairs, and the 1e5 (1 - z) penalty that is not ours


# ---- 3. culling ----------------------------------------------------------------------------------------------------------------
def test_culling_gives_exact_zeros(ctx):
  a, box = bfn.lattice_cloud(300, 300)
  b, _ = bfn.lattice_cloud(300, 301)
  b[:, 0] += box + 800.0 * B      # the clusters' boxes are 800 b apart
  x = np.concatenate([a, b])
  L = np.zeros(3)
  ref = bfn.energy(x, L, EPS, B)
  try:
    for cull in (1, 0):
      ctx.set_option("force_cull", cull)
      _check_energy(_hip(ctx, x, L), ref, "two clusters, force_cull %d" % cull)
  finally:
    ctx.set_option("force_cull", 1)


# ---- 4. order and repeatability ----------------------------------------------------------------------------------------------
def test_order_and_repeatability(ctx):
  x, box = _cloud(2049)
  L = np.array([box, box, box])
  ref = _oracle(2049, x, L)
  perm = np.random.RandomState(4).permutation(len(x))
  u0, u1 = _hip(ctx, x, L), _hip(ctx, x[perm], L)
  _check_energy(u0, ref, "2049 as listed")
  _check_energy(u1, ref, "2049 in random order")
  assert abs(u0 - u1) <= BOUND * float(ref)
  ctx.set_positions(x, 1.0, L, wall=False)
  assert ctx.body_body_potential(EPS, B) == ctx.body_body_potential(EPS, B)
  assert _hip(ctx, x, L) == u0


# ---- 5. the force is minus the gradient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("z_period", [False, True], ids=["xy", "xyz"])
def test_force_is_minus_the_gradient_of_the_energy(ctx, z_period):
  """Central difference of body_body_potential on gradient_cloud() against -F . delta of body_body_force, bound 1e-7 |F| (the
  bound tests/test_body_forces_host.py establishes for this cloud and step).  With a z period of 3 some pairs meet through
  the z image: the blob-form energy, which ignores periodic_length[2], cannot serve as the reference of this case."""
  x, L, eps, b, h = bfn.gradient_cloud()
  if z_period:
    L = L.copy()
    L[2] = 3.0
    dz = np.abs(x[:, None, 2] - x[None, :, 2])
    assert (dz > 0.5 * L[2]).any()
    assert abs(bfn.energy(x, L, eps, b) - bfn.energy(x, np.array([L[0], L[1], 0.0]), eps, b)) > 1e-6
  ctx.set_positions(x, 1.0, L, wall=False)
  F = ctx.body_body_force(eps, b)
  nF = float(np.linalg.norm(F))
  rng = np.random.RandomState(bfn.GRADIENT["seed"])

  def U(y):
    ctx.set_positions(y, 1.0, L, wall=False)
    return ctx.body_body_potential(eps, b)

  for _ in range(bfn.GRADIENT["directions"]):
    delta = rng.randn(*x.shape)
    delta /= np.linalg.norm(delta)
    want = -float(np.sum(F * delta))
    fd = (U(x + h * delta) - U(x - h * delta)) / (2 * h)
    print("dU/dh %.12e  -F.delta %.12e  |F| %.6e  miss %.2e |F|" % (fd, want, nF, abs(fd - want) / nF))
    assert abs(fd - want) <= 1e-7 * nF


# ---- 6. / 7. coincident centres, state and argument checks --------------------------------------------------------------------
def test_coincident_centres_give_inf(ctx):
  x, _ = _cloud(65)
  x = x.copy()
  x[40] = x[3]
  assert _hip(ctx, x, np.zeros(3)) == np.inf


def test_state_and_argument_checks(ctx):
  from rigidmultiblobswall_amd import _lib
  lib, ARG, STATE = _lib.load(), -1, -2
  x, _ = bfn.lattice_cloud(10, 1650)
  out = np.zeros(1)
  dev = torch.zeros(1, dtype=torch.float64, device="cuda:0")
  host = lambda eps, b, o=out: lib.rmb_body_body_potential(ctx._h, eps, b, None if o is None else ctypes.c_void_p(o.ctypes.data))      # noqa: E731
  device = lambda eps, b, o=dev: lib.rmb_body_body_potential_device(ctx._h, eps, b, None if o is None else ctypes.c_void_p(o.data_ptr()))      # noqa: E731
  ctx.set_positions(x, 1.0, np.zeros(3), wall=False)
  assert host(1.0, 1.0) == 0 and device(1.0, 1.0) == 0
  for bad in (0.0, -1.0, float("nan")):
    assert host(1.0, bad) == ARG and device(1.0, bad) == ARG
  assert host(1.0, 1.0, None) == ARG and device(1.0, 1.0, None) == ARG
  ctx.set_positions(x, 1.0, np.zeros(3), wall=True)
  assert host(1.0, 1.0) == STATE and device(1.0, 1.0) == STATE
  ctx.set_positions(x, 1.0, np.zeros(3), wall=False)
  ctx.set_target_range(2, 7)
  assert host(1.0, 1.0) == STATE and device(1.0, 1.0) == STATE
  ctx.set_target_range(0, 10)
  assert host(1.0, 1.0) == 0 and np.isfinite(out[0]) and out[0] > 0
  with pytest.raises(ValueError):
    ctx.body_body_potential_device(1.0, 1.0, out=torch.empty(2, dtype=torch.float64, device="cuda:0"))


def test_bodies_potential_of_the_module(ctx):
  """potential.bodies_potential_hip: 0.0 without the keyword (the reference), the sweep's value with it."""
  from rigidmultiblobswall_amd import potential
  x, box = _cloud(65)
  L = np.array([box, box, box])

  class Body(object):
    def __init__(self, location):
      self.location = location

  bodies = [Body(row) for row in x]
  try:
    assert potential.bodies_potential_hip(bodies, periodic_length=L) == 0.0
    got = potential.bodies_potential_hip(bodies, periodic_length=L, body_potential=(EPS, B))
    assert got == _hip(ctx, x, L) and potential.bodies_potential_hip(x, periodic_length=L, body_potential=(EPS, B)) == got
  finally:
    potential.reset()


# ---- 8. the stateless difference ----------------------------------------------------------------------------------------------
def _one_blob_deck(nb, periodic, seed):
  """nb one-blob bodies on a jittered grid of pitch 1.3 at height 1.2."""
  spacing = 1.3
  side = max(2.5, spacing * np.ceil(np.sqrt(nb)) * 0.9) if periodic else None
  d = layout([np.zeros((1, 3))] * nb, spacing, 1.2, seed, side)
  d.L = np.array([side, side, 0.0]) if periodic else np.zeros(3)
  return d


def _deck(name, periodic):
  if isinstance(name, str):      # "b65": 65 one-blob bodies
    return _one_blob_deck(int(name[1:]), periodic, seed=int(name[1:]))
  return deck_of(name, seed=name, periodic=periodic)


def _proposal(deck, k, seed, shift=0.08, angle=0.3):
  """A proposal for body k: (new location, new blob coordinates)."""
  rng = np.random.RandomState(7000 + seed)
  loc = deck.loc[k] + rng.uniform(-shift, shift, 3)
  quat = quaternion_product(quaternion_of_rotation_vector(angle * rng.normal(size=3)), deck.quat[k])
  return loc, deck.body_blobs(k, loc, quat)


def _centre_terms(loc, k, x_k, L):
  """u(|loc_j - x_k|) over the other bodies j, in long double, with the image rule of the force law."""
  others = np.delete(np.asarray(loc, dtype=EXT), k, axis=0)
  d = others - np.asarray(x_k, dtype=EXT)[None, :]
  for c in range(3):
    if L[c] > 0:
      Lc = EXT(L[c])
      d[:, c] -= np.trunc(d[:, c] / Lc + EXT(0.5) * np.sign(d[:, c])) * Lc
  r = np.sqrt(np.sum(d * d, axis=1))
  return EXT(EPS) * np.exp(-r / EXT(B)) / r


def _centre_delta_ref(loc, k, new, L):
  t_new, t_old = _centre_terms(loc, k, new, L), _centre_terms(loc, k, loc[k], L)
  return (t_new - t_old).sum(dtype=EXT), (np.abs(t_new) + np.abs(t_old)).sum(dtype=EXT)


def _delta_bb(ctx, deck, k, loc_new, new, kw):
  """-> ({dU_one, dU_pair, dU_body} of the _bb entry, {dU_one, dU_pair} of the entry without the centre term) on the same inputs,
  and the inputs read back."""
  t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()      # noqa: E731
  r, new_dev, loc_dev, loc_new_dev = t(deck.blobs()), t(new), t(deck.loc), t(loc_new)
  kw = dict(kw)
  L, eps, b, a = kw.pop("periodic_length"), kw.pop("repulsion_strength"), kw.pop("debye_length"), kw.pop("blob_radius")
  first, count = int(deck.first[k]), new.shape[0]
  got = ctx.mcmc_body_delta_device(r, first, count, new_dev, L, eps, b, a, body_potential=(EPS, B), locations=loc_dev, body=k,
                                   location_new=loc_new_dev, **kw)
  plain = ctx.mcmc_body_delta_device(r, first, count, new_dev, L, eps, b, a, **kw)
  assert got.numel() == 3 and plain.numel() == 2
  return got.cpu().numpy(), plain.cpu().numpy(), r.cpu().numpy(), new_dev.cpu().numpy()


# every deck open and periodic in x and y, and one case with a centre pair across a z period
DELTA_CASES = [(name, periodic) for name in ("b1", "b2", "b65", "b257", 66, 600) for periodic in (False, True)] + [("b65", "z")]
DELTA_IDS = ["%s-%s" % (name, {False: "open", True: "xy", "z": "xyz"}[periodic]) for name, periodic in DELTA_CASES]


@pytest.mark.parametrize("form", ["soft", "yukawa"])
@pytest.mark.parametrize("name, periodic", DELTA_CASES, ids=DELTA_IDS)
def test_difference_parity(ctx, name, periodic, form):
  """b1: no centre pair, the third component is exactly 0; b2: one pair; b65: the centre lanes straddle a wave; b257: a second
  workgroup; 66 / 600: bodies of many blobs, far fewer centre lanes than blob lanes.  "xyz": a z period so short that the two
  centres furthest apart in z meet through the image (the blob terms go on ignoring it)."""
  deck = _deck(name, bool(periodic))
  L = deck.L.copy()
  nb = len(deck.refs)
  if periodic == "z":
    dz = np.abs(deck.loc[:, None, 2] - deck.loc[None, :, 2])
    L[2] = 1.25 * dz.max()
    assert (dz > 0.5 * L[2]).any()
  kw = potential_kw(form, L)
  bit_identical = True
  for k in sorted({0, nb // 2, nb - 1}):      # the first, a middle and the last body
    loc_new, new = _proposal(deck, k, seed=nb + k)
    got, plain, r_back, new_back = _delta_bb(ctx, deck, k, loc_new, new, kw)
    d1, d2, S1, S2 = delta_rule(r_back, int(deck.first[k]), new_back, **kw)
    d3, S3 = _centre_delta_ref(deck.loc, k, loc_new, L)
    errs = [abs(EXT(g) - d) for g, d in zip(got, (d1, d2, d3))]
    ratio = max(float(e / S) if S > 0 else float(e) for e, S in zip(errs, (S1, S2, S3)))
    WORST["delta"] = max(WORST["delta"], ratio)
    same = bool(got[0] == plain[0] and got[1] == plain[1])
    bit_identical = bit_identical and same
    print("%s body %d %s %s: dU_body %.6e (off by %.3e of S %.6e)  ratio of the three %.3e  first two bit-identical to the plain entry: %s" %
          (name, k, form, periodic, got[2], float(errs[2]), float(S3), ratio, same))
    assert errs[2] <= BOUND * S3, (float(errs[2]), float(S3))
    assert errs[0] <= BOUND * S1 and errs[1] <= BOUND * S2, (float(errs[0]), float(S1), float(errs[1]), float(S2))
    assert abs(EXT(plain[0]) - d1) <= BOUND * S1 and abs(EXT(plain[1]) - d2) <= BOUND * S2
    if nb == 1:
      assert got[2] == 0.0 and S3 == 0
    else:
      assert S3 > 0
  print("%s %s %s: first two components bit-identical to rmb_mcmc_body_delta_device: %s" % (name, form, periodic, bit_identical))


def test_refused_arguments_of_the_bb_entries(ctx):
  from rigidmultiblobswall_amd import _lib
  lib, ARG = _lib.load(), -1
  f64 = lambda *shape: torch.ones(*shape, dtype=torch.float64).cuda()      # noqa: E731
  r, new, out, loc, loc_new = f64(12, 3), f64(4, 3), f64(3), f64(3, 3), f64(3)
  loc[:, 0] = torch.arange(3, dtype=torch.float64)
  L = np.zeros(3)
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
  hp = lambda x: ctypes.c_void_p(x.ctypes.data)     # noqa: E731
  pot = (0.3, 0.1, 0.0, 1.0, 0.0, 0.2, 0)

  def delta(n_bodies=3, loc_t=loc, body=1, new_t=loc_new, b=1.0, out_t=out):
    return lib.rmb_mcmc_body_delta_bb_device(ctx._h, 12, p(r), 4, 4, p(new), n_bodies, p(loc_t), body, p(new_t), hp(L), *pot, 1.0, b, p(out_t))
  assert delta() == 0
  assert delta(loc_t=None) == ARG and delta(new_t=None) == ARG and delta(out_t=None) == ARG
  assert delta(body=3) == ARG and delta(body=-1) == ARG and delta(n_bodies=0) == ARG
  assert delta(b=0.0) == ARG and delta(b=float("nan")) == ARG
  first = np.array([0, 4, 8, 12], dtype=np.int64)
  blob_ref, ref, quat = torch.zeros(12, dtype=torch.int32).cuda(), torch.zeros(4, 3, dtype=torch.float64).cuda(), f64(3, 4)
  draws, energy, flags = torch.zeros(3, 7, dtype=torch.float64).cuda(), torch.zeros(3, dtype=torch.float64).cuda(), torch.zeros(3, dtype=torch.int32).cuda()

  def sweep(n_free=3, b=1.0, kT=0.1, energy_t=energy):
    return lib.rmb_mcmc_sweep_bb_device(ctx._h, 3, n_free, 12, hp(first), p(blob_ref), p(ref), p(loc), p(quat), p(r), p(draws), 0.1, hp(L), *pot,
                                        1.0, b, kT, p(energy_t), p(flags))
  assert sweep(b=0.0) == ARG and sweep(b=-1.0) == ARG and sweep(kT=0.0) == ARG and sweep(energy_t=None) == ARG
  before = (r.clone(), loc.clone(), energy.clone())
  assert sweep(n_free=0) == 0
  torch.cuda.synchronize()
  assert torch.equal(before[0], r) and torch.equal(before[1], loc) and torch.equal(before[2], energy)
  with pytest.raises(ValueError, match="3 entries"):
    ctx.mcmc_body_delta_device(r, 4, 4, new, L, 0.3, 0.1, 0.2, out=f64(2), body_potential=(1.0, 1.0), locations=loc, body=1, location_new=loc_new)
  with pytest.raises(ValueError, match="debye_length"):
    ctx.mcmc_body_delta_device(r, 4, 4, new, L, 0.3, 0.1, 0.2, body_potential=(1.0, 0.0), locations=loc, body=1, location_new=loc_new)


# ---- 9. - 11. the sampler ------------------------------------------------------------------------------------------------------
LINES = ("n_steps %d\nn_save 1\ninitial_step 0\ng 0.6\nblob_radius 0.2\nkT %r\nperiodic_length %r %r %r\nrepulsion_strength_wall 0.8\n"
         "debye_length_wall 0.12\nrepulsion_strength 0.35\ndebye_length 0.09\nseed %d\noutput_name run\n")
FREE66 = [("structure", "boom", [0, 1]), ("structure", "shell", [2, 3, 4])]
OBSTACLES66 = [("structure", "boom", [0, 1]), ("obstacle", "shell", [2, 3, 4])]      # prescribed bodies after the free ones


def _deck66(tmp_path, steps, periodic=False, z_period=False, kT=0.05, seed=21, structures=FREE66, extra=""):
  deck = deck_of(66, seed=3, periodic=periodic)
  Lz = 0.0
  if z_period:
    dz = np.abs(deck.loc[:, None, 2] - deck.loc[None, :, 2])
    Lz = float(1.25 * dz.max())
  return deck, write_deck(str(tmp_path), deck, structures, LINES % (steps, kT, float(deck.L[0]), float(deck.L[1]), Lz, seed) + extra)


def _run_device(path, **kw):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  s = MCMCSampler(ReadInput(path), device=0, write_files=False, **kw)
  try:
    s.run()
  finally:
    s.close()
  return s


def _scale(cpu, kw, L):
  """The largest sum|terms| over the saved configurations: the blob terms' S plus U_body."""
  S = 0.0
  for loc, quat in cpu.saved.values():
    S = max(S, float(potnp.energy(cpu.state._blobs(loc, quat), **kw)[2]) + float(bfn.energy(loc, L, EPS, B)))
  return S


# seeds chosen on the CPU, with the twin alone: its smallest |u - exp(-dE/kT)| exceeds 1e-9 and both outcomes occur
SWEEP_CASES = [("free_open", FREE66, False, False, 21), ("free_xyz", FREE66, True, True, 22), ("obstacles_xy", OBSTACLES66, True, False, 23)]


@pytest.mark.parametrize("name, structures, periodic, z_period, seed", SWEEP_CASES, ids=[c[0] for c in SWEEP_CASES])
def test_sweeps_make_the_twins_decisions(name, structures, periodic, z_period, seed, tmp_path, monkeypatch):
  """66 blobs, 5 bodies, 6 sweeps over the free ones, every move compared with the numpy twin (f = the blob energy in long
  double, plus mcmc.body_body_energy).  The running energy of three sums against the full recompute at every save (n_save 1:
  a drift covers the moves of one sweep): n_moves 1e-13 S, S the largest sum|terms| over the saved configurations.  With the
  shells as obstacles only the boomerangs move, but all five centres enter the pairs: the twin's energy says so."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler, body_body_energy
  deck, path = _deck66(tmp_path, 6, periodic, z_period, seed=seed, structures=structures)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  f, kw = energy_fn(read, "soft")
  L = np.asarray(read.periodic_length, dtype=np.float64)
  cpu = MCMCSampler(read, energy=f, write_files=False, moves="single", body_potential=(EPS, B)).run()
  n_free = cpu.n_free
  print("twin: decision margin %.3e, accepted %d of %d" % (cpu.state.decision_margin, cpu.accepted_moves, len(cpu.accepted)))
  assert cpu.state.decision_margin > 1e-9 and len(cpu.accepted) == 6 * n_free and 0 < cpu.accepted_moves < 6 * n_free
  assert n_free == (5 if structures is FREE66 else 2) and cpu.n_bodies == 5
  if structures is OBSTACLES66:      # the prescribed centres carry most of the body energy
    assert body_body_energy(deck.loc, L, EPS, B) > 2.0 * body_body_energy(deck.loc[:2], L, EPS, B)
  gpu = _run_device(path, moves="single", body_potential=(EPS, B))
  assert gpu.accepted == cpu.accepted and gpu.accepted_moves == cpu.accepted_moves
  assert sorted(gpu.saved) == sorted(cpu.saved) == list(range(7))
  for step in cpu.saved:
    assert np.max(np.abs(gpu.saved[step][0] - cpu.saved[step][0])) <= 1e-12 and np.max(np.abs(gpu.saved[step][1] - cpu.saved[step][1])) <= 1e-12
  S = _scale(cpu, kw, L)
  for step, (running, full) in sorted(gpu.energy_drift.items()):
    print("step %d: running %.15e  full %.15e  drift %.3e (allowed %.3e)" % (step, running, full, abs(running - full), n_free * 1e-13 * S))
    assert abs(running - full) <= n_free * 1e-13 * S
  assert np.allclose(gpu.energy_log, cpu.energy_log, rtol=0, atol=n_free * 1e-13 * S) and len(gpu.energy_log) == 7
  # and the body term is in those energies
  off = MCMCSampler(read, energy=f, write_files=False, moves="single")
  assert abs(cpu.energy_log[0] - off.state.current_energy()) > 1e-3 * S


def test_a_rejected_move_writes_nothing(tmp_path, monkeypatch):
  """kT so small that every uphill move is rejected: the rejected bodies' rows of r, their locations and quaternions are
  bit-identical afterwards, the accepted ones moved and the running energy fell.  Then a sweep whose uniforms are NaN
  (numpy's comparison: u < x is false) rejects every move: r, loc, quat and all three running energies keep their bits."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck, path = _deck66(tmp_path, 2, kT=1e-12)
  monkeypatch.chdir(tmp_path)
  s = MCMCSampler(ReadInput(path), device=0, write_files=False, moves="single", body_potential=(EPS, B))
  snap = lambda: (s.state.r_new.cpu().numpy().copy(), s.state.loc.cpu().numpy().copy(), s.state.quat.cpu().numpy().copy(),      # noqa: E731
                  s.state.energy.cpu().numpy().copy())
  try:
    s.state.current_energy()
    draws = s._sweep_draws(np.random.RandomState(5))
    before = snap()
    flags, running = s.state.sweep(draws, s.max_angle_shift)
    after = snap()
    draws[:, 6] = np.nan
    flags2, running2 = s.state.sweep(draws, s.max_angle_shift)
    after2 = snap()
  finally:
    s.close()
  assert before[3].shape == (3,) and before[3][2] > 0
  assert len(flags) == 5 and not all(flags) and any(flags)
  for k, ok in enumerate(flags):
    rows = slice(int(s.body_first[k]), int(s.body_first[k + 1]))
    same = np.array_equal(before[0][rows], after[0][rows]) and np.array_equal(before[1][k], after[1][k]) and np.array_equal(before[2][k], after[2][k])
    assert same != ok, (k, ok)
  assert after[3].sum() < before[3].sum() and running == float(after[3].sum()) and not np.array_equal(before[3], after[3])
  assert flags2 == [False] * 5 and running2 == running
  assert all(np.array_equal(a, b) for a, b in zip(after, after2))


@pytest.mark.parametrize("periodic, z_period, seed", [(False, False, 31), (True, True, 32)], ids=["open", "xyz"])
def test_all_body_moves_make_the_twins_decisions(periodic, z_period, seed, tmp_path, monkeypatch):
  """moves="all": every proposal's energy gains U_body of the proposed locations (the sweep on the second context).  The same
  accepts as the twin, energies to 1e-12 relative (what test_gpu_mcmc.py asks of the HIP energy through assert_chain_matches)."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck, path = _deck66(tmp_path, 12, periodic, z_period, seed=seed)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  f, kw = energy_fn(read, "soft")
  cpu = MCMCSampler(read, energy=f, write_files=False, moves="all", body_potential=(EPS, B)).run()
  gpu = _run_device(path, moves="all", body_potential=(EPS, B))
  assert gpu.accepted == cpu.accepted and len(cpu.accepted) == 12 and 0 < cpu.accepted_moves < 12
  log, ref = np.array(gpu.energy_log), np.array(cpu.energy_log)
  worst = np.max(np.abs(log - ref) / np.abs(ref))
  print("energy log: worst relative difference %.3e over %d values" % (worst, ref.size))
  assert worst <= 1e-12 and log.shape == (13,)
  for step in cpu.saved:
    assert np.max(np.abs(gpu.saved[step][0] - cpu.saved[step][0])) <= 1e-12 and np.max(np.abs(gpu.saved[step][1] - cpu.saved[step][1])) <= 1e-12
  off = _run_device(path, moves="all")
  assert abs(off.energy_log[0] - gpu.energy_log[0]) > 1e-3 * abs(gpu.energy_log[0])


@pytest.mark.parametrize("moves", ["all", "single"])
def test_zero_strength_reproduces_the_default_chain(moves, tmp_path, monkeypatch):
  deck, path = _deck66(tmp_path, 6, periodic=True)
  monkeypatch.chdir(tmp_path)
  a, b = _run_device(path, moves=moves, body_potential=(0.0, B)), _run_device(path, moves=moves)
  assert a.body_potential == (0.0, B) and b.body_potential is None
  assert a.accepted == b.accepted and any(a.accepted) and not all(a.accepted)
  assert np.allclose(a.energy_log, b.energy_log, rtol=1e-12, atol=0)
  for step in b.saved:
    assert np.max(np.abs(a.saved[step][0] - b.saved[step][0])) <= 1e-12 and np.max(np.abs(a.saved[step][1] - b.saved[step][1])) <= 1e-12


# ---- 12. the command line --------------------------------------------------------------------------------------------------------
def test_command_line_with_the_decks_law(tmp_path):
  """One run: the deck names the option, --body-potential deck takes its two numbers, .MCMC_info names the law."""
  deck, path = _deck66(tmp_path, 3, extra="body_body_force_torque_implementation hip\n")
  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
  out = subprocess.run([sys.executable, "-m", "rigidmultiblobswall_amd.mcmc", "data.main", "--body-potential", "deck", "--moves", "single"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
  assert out.returncode == 0, out.stdout + out.stderr
  text = open(os.path.join(str(tmp_path), "run.MCMC_info")).read().splitlines()
  assert len(text) == 5 and text[4] == "body_potential = yukawa repulsion_strength 0.35 debye_length 0.09"
  assert {"run.inputfile", "run.random_state", "run.time"} <= set(os.listdir(str(tmp_path)))
