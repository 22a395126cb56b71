"""Single-body Metropolis moves on the device: the energy difference of one moved body (rmb_mcmc_body_delta_device) against
the long-double statement of the rule (_mcmc_moves_common.delta_rule, built from _potential_numpy's terms) on the same
coordinates, bound |d_hip - d_ref| <= 1e-13 S with S = sum(|new term| + |old term|) over the touched terms -- the bound
test_gpu_potential.py states for the energy itself -- separately for the one-blob and the pair part; and the sweep
(rmb_mcmc_sweep_device through MCMCSampler(moves="single")) against its numpy twin."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _potential_numpy as potnp
from _mcmc_moves_common import (GATE_CASES, deck_of, delta_rule, energy_fn, gate_case, moved_body, potential_kw, write_deck)
from rigidmultiblobswall_amd.read_input import ReadInput

pytestmark = pytest.mark.gpu

BOUND = 1e-13
WORST = {"ratio": 0.0}     # largest |d_hip - d_ref| / S seen by this module (printed when the context fixture is torn down)


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()
  print("worst |d_hip - d_ref| / sum(|new| + |old|) of this module = %.3e (bound %.1e)" % (WORST["ratio"], BOUND))     # DESIGN 3.9 quotes it


def _delta_gpu(ctx, r, first, new, kw):
  """-> (d_one, d_pair) of the device, and the coordinates it computed on, read back."""
  r_dev, new_dev = torch.as_tensor(r).cuda(), torch.as_tensor(new).cuda()
  kw = dict(kw)
  L, eps, b, a = kw.pop("periodic_length"), kw.pop("repulsion_strength"), kw.pop("debye_length"), kw.pop("blob_radius")
  out = ctx.mcmc_body_delta_device(r_dev, first, new.shape[0], new_dev, L, eps, b, a, **kw)
  return out.cpu().numpy(), r_dev.cpu().numpy(), new_dev.cpu().numpy()


def _check(got, ref, what):
  d1, d2, S1, S2 = ref
  e1, e2 = abs(potnp.EXT(got[0]) - d1), abs(potnp.EXT(got[1]) - d2)
  ratio = max(float(e / S) if S > 0 else float(e) for e, S in ((e1, S1), (e2, S2)))
  WORST["ratio"] = max(WORST["ratio"], ratio)
  print("%s dU_one %.6e (off by %.3e of S %.6e)  dU_pair %.6e (off by %.3e of S %.6e)  ratio %.3e" %
        (what, got[0], e1, S1, got[1], e2, S2, ratio))
  assert e1 <= BOUND * S1 and e2 <= BOUND * S2, (what, float(e1), float(S1), float(e2), float(S2))


def _bodies_to_move(deck):
  nb = len(deck.refs)
  return sorted({0, nb // 2, nb - 1})      # the first, a middle and the last body


@pytest.mark.parametrize("form", ["soft", "yukawa"])
@pytest.mark.parametrize("periodic", [False, True], ids=["open", "periodic"])
@pytest.mark.parametrize("n", [1, 2, 66, 267, 600])
def test_difference_parity(ctx, n, periodic, form):
  """1 blob: no pair at all; 66: body ranges straddle lane 63 / 64; 267: two workgroups, odd tail; 600: two 300-blob bodies,
  the LDS chunk loop (256 + 44 blobs)."""
  two = n in (2, 600)      # two bodies = one body pair: a periodic deck is run with that pair on either side of the half box
  for far in ((False, True) if periodic and two else (None,)):
    deck = deck_of(n, seed=n, periodic=periodic, far=far)
    assert deck.n == n
    kw = potential_kw(form, deck.L)
    r = deck.blobs()
    if periodic and len(deck.refs) > 1:      # body pairs on both sides of the half box
      d = np.abs(deck.loc[:, None, 0] - deck.loc[None, :, 0])
      beyond, within = (d > 0.5 * deck.L[0]).any(), (d[d > 0] < 0.5 * deck.L[0]).any()
      assert (beyond and within) if far is None else (beyond == far and within != far)
    for k in _bodies_to_move(deck):
      first = int(deck.first[k])
      new = moved_body(deck, k, seed=n + k)
      got, r_back, new_back = _delta_gpu(ctx, r, first, new, kw)
      ref = delta_rule(r_back, first, new_back, **kw)
      assert n == 1 or ref[3] > 0
      _check(got, ref, "n %d body %d %s %s%s" % (n, k, form, "periodic" if periodic else "open", "" if far is None else (" far" if far else " near")))
      if n == 1:
        assert got[1] == 0.0


@pytest.mark.parametrize("form", ["soft", "yukawa"])
@pytest.mark.parametrize("periodic", [False, True], ids=["open", "periodic"])
@pytest.mark.parametrize("case", GATE_CASES)
def test_difference_behind_the_wall(ctx, case, periodic, form):
  deck, r, first, new = gate_case(case, periodic)
  kw = potential_kw(form, deck.L)
  got, r_back, new_back = _delta_gpu(ctx, r, first, new, kw)
  _check(got, delta_rule(r_back, first, new_back, **kw), "%s %s %s" % (case, form, "periodic" if periodic else "open"))


def test_difference_without_wall_terms_and_the_module_wrapper(ctx):
  """repulsion_strength_wall = 0 drops the wall term; potential.body_energy_difference_hip takes numpy arrays."""
  from rigidmultiblobswall_amd import potential
  deck = deck_of(66, seed=5)
  kw = potential_kw("soft", deck.L, wall_terms=False)
  r, first, new = deck.blobs(), int(deck.first[3]), moved_body(deck, 3, seed=9)
  got, r_back, new_back = _delta_gpu(ctx, r, first, new, kw)
  ref = delta_rule(r_back, first, new_back, **kw)
  assert got[0] == 0.0 and ref[2] == 0
  _check(got, ref, "no wall terms")
  assert potential.body_energy_difference_hip(r, first, new, **kw) == (got[0], got[1])
  potential.reset()


def test_refused_arguments_of_the_c_entries(ctx):
  from rigidmultiblobswall_amd import _lib
  lib, ARG = _lib.load(), -1      # RMB_ERR_ARG
  r, new, out = torch.ones(12, 3, dtype=torch.float64).cuda(), torch.ones(4, 3, dtype=torch.float64).cuda(), torch.zeros(2, dtype=torch.float64).cuda()
  L = np.zeros(3)
  p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
  hp = lambda x: ctypes.c_void_p(x.ctypes.data)     # noqa: E731
  pot = (0.3, 0.1, 0.0, 1.0, 0.0, 0.2, 0)
  delta = lambda *a: lib.rmb_mcmc_body_delta_device(ctx._h, *a)      # noqa: E731
  assert delta(12, p(r), 4, 4, p(new), hp(L), *pot, p(out)) == 0
  assert delta(12, None, 4, 4, p(new), hp(L), *pot, p(out)) == ARG and delta(12, p(r), 4, 4, p(new), hp(L), *pot, None) == ARG
  assert delta(12, p(r), 10, 4, p(new), hp(L), *pot, p(out)) == ARG and delta(12, p(r), 4, 0, p(new), hp(L), *pot, p(out)) == ARG
  assert delta(12, p(r), 4, 4, p(new), hp(L), 0.3, 0.0, 0.0, 1.0, 0.0, 0.2, 0, p(out)) == ARG          # debye_length
  # the sweep
  first = np.array([0, 4, 8, 12], dtype=np.int64)
  blob_ref, ref = torch.zeros(12, dtype=torch.int32).cuda(), torch.zeros(4, 3, dtype=torch.float64).cuda()
  loc, quat = torch.ones(3, 3, dtype=torch.float64).cuda(), torch.ones(3, 4, dtype=torch.float64).cuda()
  draws, energy, flags = torch.zeros(3, 7, dtype=torch.float64).cuda(), torch.zeros(2, dtype=torch.float64).cuda(), torch.zeros(3, dtype=torch.int32).cuda()
  def sweep(n_free=3, table=first, kT=0.1, debye=0.1, loc_p=p(loc), flags_p=p(flags)):
    return lib.rmb_mcmc_sweep_device(ctx._h, 3, n_free, 12, hp(table) if table is not None else None, p(blob_ref), p(ref), loc_p, p(quat), p(r),
                                     p(draws), 0.1, hp(L), 0.3, debye, 0.0, 1.0, 0.0, 0.2, 0, kT, p(energy), flags_p)
  assert sweep(kT=0.0) == ARG and sweep(kT=-1.0) == ARG and sweep(kT=float("nan")) == ARG
  assert b"kT" in lib.rmb_last_error()
  assert sweep(debye=0.0) == ARG and sweep(loc_p=None) == ARG and sweep(flags_p=None) == ARG and sweep(table=None) == ARG
  assert sweep(table=np.array([0, 8, 4, 12], dtype=np.int64)) == ARG          # decreasing
  assert sweep(table=np.array([0, 4, 8, 11], dtype=np.int64)) == ARG and sweep(table=np.array([1, 4, 8, 12], dtype=np.int64)) == ARG      # not all of [0, n)
  # n_free = 0 is a no-op: nothing is written
  before = (r.clone(), loc.clone(), energy.clone())
  assert sweep(n_free=0) == 0
  torch.cuda.synchronize()
  assert torch.equal(before[0], r) and torch.equal(before[1], loc) and torch.equal(before[2], energy)


# ---- the sweep through the sampler ---------------------------------------------------------------------------------------
LINES = ("n_steps %d\nn_save 1\ninitial_step 0\ng %r\nblob_radius 0.2\nkT %r\nperiodic_length %r %r 0\nrepulsion_strength_wall %r\n"
         "debye_length_wall 0.12\nrepulsion_strength %r\ndebye_length 0.09\nseed %d\noutput_name run\n")
STRUCTURES66 = [("structure", "boom", [0, 1]), ("structure", "shell", [2, 3, 4])]


def _deck66(tmp_path, steps, periodic=False, g=0.6, kT=0.05, eps_wall=0.8, eps=0.35, seed=21, structures=STRUCTURES66, layout_seed=3):
  """layout_seed 3: two blobs below z = a, none behind the wall; 5: every blob above z = 0.75 (the yukawa wall term adds
  1e12 e_w below z = a, where an energy difference is only good to 1e-4 in double precision -- on either side)."""
  deck = deck_of(66, seed=layout_seed, periodic=periodic)
  return deck, write_deck(str(tmp_path), deck, structures, LINES % (steps, g, kT, float(deck.L[0]), float(deck.L[1]), eps_wall, eps, seed))


def _run_device(path, **kw):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  s = MCMCSampler(ReadInput(path), device=0, write_files=False, moves="single", **kw)
  try:
    s.run()
  finally:
    s.close()
  return s


# seeds chosen on the CPU, with the twin alone: its smallest |u - exp(-dE/kT)| exceeds 1e-9 and both outcomes occur
@pytest.mark.parametrize("rng_mode, form, periodic, seed", [("reference", "soft", False, 21), ("batched", "soft", True, 22),
                                                            ("reference", "yukawa", True, 23), ("batched", "yukawa", False, 24)])
def test_sweeps_make_the_twins_decisions(rng_mode, form, periodic, seed, tmp_path, monkeypatch):
  """66 blobs, 5 free bodies, 6 sweeps = 30 moves, every one compared.  The running energy against the full evaluation at
  every save: each move adds a difference that is off by at most 1e-13 of its touched terms' scale, which the scale of the
  whole configuration bounds -- n_moves 1e-13 S_total, S_total the largest over the saved configurations, n_moves the moves since the last save."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck, path = _deck66(tmp_path, 6, periodic, seed=seed, layout_seed=5 if form == "yukawa" else 3)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  energy, kw = energy_fn(read, form)
  cpu = MCMCSampler(read, potential=form, energy=energy, write_files=False, moves="single", rng=rng_mode).run()
  print("twin: decision margin %.3e, accepted %d of %d" % (cpu.state.decision_margin, cpu.accepted_moves, len(cpu.accepted)))
  assert cpu.state.decision_margin > 1e-9 and len(cpu.accepted) == 30 and 0 < cpu.accepted_moves < 30
  gpu = _run_device(path, potential=form, rng=rng_mode)
  assert gpu.accepted == cpu.accepted and gpu.accepted_moves == cpu.accepted_moves
  assert sorted(gpu.saved) == sorted(cpu.saved) == list(range(7))
  for step in cpu.saved:
    assert np.max(np.abs(gpu.saved[step][0] - cpu.saved[step][0])) <= 1e-12 and np.max(np.abs(gpu.saved[step][1] - cpu.saved[step][1])) <= 1e-12
  S_total = 0.0
  for step, (loc, quat) in cpu.saved.items():
    u1, u2, S = potnp.energy(cpu.state._blobs(loc, quat), **kw)
    S_total = max(S_total, float(S))
  # n_save 1: the running energy restarts from a full evaluation at every save, so a drift covers the 5 moves of one sweep
  for step, (running, full) in sorted(gpu.energy_drift.items()):
    print("step %d: running %.15e  full %.15e  drift %.3e (allowed %.3e)" % (step, running, full, abs(running - full), 5 * 1e-13 * S_total))
    assert abs(running - full) <= 5 * 1e-13 * S_total
  assert np.allclose(gpu.energy_log, cpu.energy_log, rtol=0, atol=5 * 1e-13 * S_total) and len(gpu.energy_log) == 7


def test_sweeps_of_bodies_larger_than_one_chunk(tmp_path, monkeypatch):
  """600 blobs, two 300-blob bodies (lifted above the wall), 2 sweeps: the sweep's instance composes and stages a body in two
  chunks (256 + 44), leaves 900 proposed coordinates in the scratch and commits them.  Saved after steps 0 and 1: the last
  drift covers the 2 moves of the second sweep, within 2 1e-13 S_total of the full evaluation."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck = deck_of(600, seed=600)
  deck.loc[:, 2] += 1.0
  assert deck.blobs()[:, 2].min() > 0.2
  path = write_deck(str(tmp_path), deck, [("structure", "big0", [0]), ("structure", "big1", [1])],
                    LINES % (2, 0.6, 0.05, 0.0, 0.0, 0.8, 0.35, 31))
  text = open(path).read().replace("n_save 1\n", "n_save 2\n")
  with open(path, "w") as f:
    f.write(text)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  energy, kw = energy_fn(read, "soft")
  cpu = MCMCSampler(read, energy=energy, write_files=False, moves="single").run()
  print("twin: decision margin %.3e, accepted %s" % (cpu.state.decision_margin, cpu.accepted))
  assert cpu.state.decision_margin > 1e-9 and len(cpu.accepted) == 4 and 0 < cpu.accepted_moves < 4
  gpu = _run_device(path)
  assert gpu.accepted == cpu.accepted and sorted(gpu.saved) == sorted(cpu.saved) == [0, 2]
  for step in cpu.saved:
    assert np.max(np.abs(gpu.saved[step][0] - cpu.saved[step][0])) <= 1e-12 and np.max(np.abs(gpu.saved[step][1] - cpu.saved[step][1])) <= 1e-12
  S_total = max(float(potnp.energy(cpu.state._blobs(*cpu.saved[k]), **kw)[2]) for k in cpu.saved)
  running, full = gpu.energy_drift[2]
  print("running %.15e  full %.15e  drift %.3e (allowed %.3e)" % (running, full, abs(running - full), 2 * 1e-13 * S_total))
  assert abs(running - full) <= 2 * 1e-13 * S_total


def _device_state(path, **kw):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  s = MCMCSampler(ReadInput(path), device=0, write_files=False, moves="single", **kw)
  s.state.current_energy()
  return s


def _snapshot(s):
  return s.state.r_new.cpu().numpy().copy(), s.state.loc.cpu().numpy().copy(), s.state.quat.cpu().numpy().copy()


def test_a_rejected_move_writes_nothing(tmp_path, monkeypatch):
  """kT so small that every uphill move is rejected (exp(-dE/kT) = 0): the rejected bodies' rows of r, their locations and
  quaternions are bit-identical afterwards, the accepted (downhill) ones moved, and the running energy fell."""
  deck, path = _deck66(tmp_path, 2, kT=1e-12)
  monkeypatch.chdir(tmp_path)
  s = _device_state(path)
  try:
    rng = np.random.RandomState(5)
    before, e0 = _snapshot(s), s.state.energy.cpu().numpy().copy()
    flags, running = s.state.sweep(s._sweep_draws(rng), s.max_angle_shift)
    after, e1 = _snapshot(s), s.state.energy.cpu().numpy().copy()
  finally:
    s.close()
  assert len(flags) == 5 and not all(flags) and any(flags)
  for k, ok in enumerate(flags):
    rows = slice(int(s.body_first[k]), int(s.body_first[k + 1]))
    same = np.array_equal(before[0][rows], after[0][rows]) and np.array_equal(before[1][k], after[1][k]) and np.array_equal(before[2][k], after[2][k])
    assert same != ok, (k, ok)
    if ok:
      assert not np.array_equal(before[0][rows], after[0][rows]) and not np.array_equal(before[2][k], after[2][k])
  assert e1.sum() < e0.sum() and running == float(e1.sum())


def test_without_forces_every_move_is_accepted(tmp_path, monkeypatch):
  deck, path = _deck66(tmp_path, 3, g=0.0, eps_wall=0.0, eps=0.0, layout_seed=5)
  monkeypatch.chdir(tmp_path)
  s = _run_device(path)
  assert len(s.accepted) == 15 and all(s.accepted) and s.accepted_moves == 15 and s.energy_log == [0.0] * 4


def test_prescribed_bodies_are_never_moved(tmp_path, monkeypatch):
  """The three shells are obstacles: only the two boomerangs are swept."""
  deck, path = _deck66(tmp_path, 4, structures=[("structure", "boom", [0, 1]), ("obstacle", "shell", [2, 3, 4])])
  monkeypatch.chdir(tmp_path)
  s = _device_state(path)
  try:
    before = _snapshot(s)
    s.run()
    after = _snapshot(s)
  finally:
    s.close()
  assert s.n_free == 2 and s.n_bodies == 5 and len(s.accepted) == 8 and any(s.accepted)
  assert np.array_equal(before[0][30:], after[0][30:]) and np.array_equal(before[1][2:], after[1][2:]) and np.array_equal(before[2][2:], after[2][2:])
  assert not np.array_equal(before[1][:2], after[1][:2])


@pytest.mark.parametrize("rng_mode", ["reference", "batched"])
def test_a_seeded_run_is_bit_repeatable(rng_mode, tmp_path, monkeypatch):
  deck, path = _deck66(tmp_path, 6, periodic=True)
  monkeypatch.chdir(tmp_path)
  a, b = _run_device(path, rng=rng_mode), _run_device(path, rng=rng_mode)
  assert a.energy_log == b.energy_log and a.accepted == b.accepted and a.energy_drift == b.energy_drift and 0 < a.accepted_moves < 30
  for step in a.saved:
    assert np.array_equal(a.saved[step][0], b.saved[step][0]) and np.array_equal(a.saved[step][1], b.saved[step][1])


# ---- 32 non-interacting blobs above the wall: the sampled height distribution -------------------------------------------------
def test_height_distribution_of_non_interacting_blobs(tmp_path, monkeypatch):
  """The parameters of test_gpu_mcmc.test_single_blob_height_distribution, 32 single-blob bodies with repulsion_strength = 0
  (every pair term is eps * finite = 0 exactly), 625 seeded sweeps = 20 000 height samples: the mean height lies within five
  batch-means standard errors (20 batches of consecutive sweeps) of the quadrature of exp(-U(h)/kT).  The twin runs the same
  chain with the one-blob terms as its energy; the device makes its decisions."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  from test_gpu_mcmc import A, BW, EW, KT, W, _batch_means, _mean_height_by_quadrature
  sweeps, nb = 625, 32
  d = str(tmp_path)
  with open(os.path.join(d, "blob.vertex"), "w") as f:
    f.write("1\n0 0 0\n")
  with open(os.path.join(d, "blob.clones"), "w") as f:
    f.write("%d\n" % nb + "".join("%d %d 0.5 1 0 0 0\n" % (k % 8, k // 8) for k in range(nb)))
  with open(os.path.join(d, "data.main"), "w") as f:
    f.write("n_steps %d\nn_save 1\ninitial_step 0\ng %r\nblob_radius %r\nkT %r\nrepulsion_strength_wall %r\ndebye_length_wall %r\n"
            "repulsion_strength 0\ndebye_length 0.1\nseed 1\noutput_name run\nstructure blob.vertex blob.clones\n" % (sweeps, W, A, KT, EW, BW))
  monkeypatch.chdir(tmp_path)
  ext = potnp.EXT
  energy = lambda r: float(potnp.one_blob_terms(r[:, 2], ext(EW), ext(BW), ext(W), ext(A), "soft").sum(dtype=ext))      # noqa: E731
  cpu = MCMCSampler(ReadInput("data.main"), energy=energy, write_files=False, moves="single").run()
  gpu = _run_device("data.main")
  exact = _mean_height_by_quadrature()
  assert cpu.state.decision_margin > 1e-9
  for name, s in (("twin", cpu), ("device", gpu)):
    heights = np.array([s.saved[k][0][:, 2].mean() for k in range(sweeps)])      # per sweep: the mean over the 32 blobs
    mean, se = _batch_means(heights)
    print("%s: mean height %.6f, quadrature %.6f, batch-means standard error %.6f, acceptance %.3f" %
          (name, mean, exact, se, s.accepted_moves / float(sweeps * nb)))
    assert abs(mean - exact) <= 5 * se
  assert gpu.accepted == cpu.accepted and len(gpu.accepted) == sweeps * nb
