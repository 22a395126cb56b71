"""Single-body Metropolis moves, host side: the numpy twin of the sweep (MCMCSampler(moves="single", energy=f)) against a
brute-force loop, the untouched all-body mode, the refused arguments, and the energy-difference rule stated in numpy against
total(new) - total(old) of the long-double restatement on the cases that put a blob behind the wall."""
import numpy as np
import pytest

import _potential_numpy as potnp
from _mcmc_common import FIXTURES, assert_chain_matches, load_case
from _mcmc_moves_common import GATE_CASES, brute_force_chain, deck_of, delta_rule, energy_fn, gate_case, potential_kw, write_deck
from rigidmultiblobswall_amd.read_input import ReadInput

LINES = ("n_steps %d\nn_save 1\ninitial_step %d\ng 0.6\nblob_radius 0.2\nkT 0.05\nrepulsion_strength_wall 0.8\ndebye_length_wall 0.12\n"
         "repulsion_strength 0.35\ndebye_length 0.09\nseed 21\noutput_name run\n")


def _deck27(tmp_path, steps, initial=0):
  deck = deck_of(27, seed=1)
  return deck, write_deck(str(tmp_path), deck, [("structure", "boom", [0]), ("structure", "shell", [1])], LINES % (steps, initial))


@pytest.mark.parametrize("rng_mode", ["reference", "batched"])
def test_twin_equals_a_brute_force_loop(rng_mode, tmp_path, monkeypatch):
  """27 blobs (a boomerang and a shell), 8 sweeps: the same decisions, the same configurations after every sweep, the same
  energies -- and both outcomes occur."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck, path = _deck27(tmp_path, 8)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  energy, _ = energy_fn(read, "soft")
  s = MCMCSampler(read, energy=energy, write_files=False, moves="single", rng=rng_mode)
  assert s.n_blobs == 27 and s.n_free == 2 and list(s.body_first) == [0, 15, 27]
  step0, angle0 = s.max_translation, s.max_angle_shift
  s.run(rng=np.random.RandomState(21))
  flags, states, energies = brute_force_chain(deck, 2, np.random.RandomState(21), 8, step0, angle0, read.kT, energy, rng_mode)
  assert s.accepted == flags and len(flags) == 16 and 0 < sum(flags) < 16
  assert s.accepted_moves == sum(flags)
  assert np.allclose(s.energy_log, energies, rtol=1e-12, atol=0) and len(s.energy_log) == 9
  for step in range(8):      # the save of step k holds the state after sweep k
    assert np.max(np.abs(s.saved[step][0] - states[step][0])) <= 1e-12 and np.max(np.abs(s.saved[step][1] - states[step][1])) <= 1e-12
  assert np.isfinite(s.state.decision_margin) and s.state.decision_margin > 0
  # the twin's running energy IS a full evaluation
  assert all(run == full for run, full in s.energy_drift.values()) and sorted(s.energy_drift) == sorted(s.saved)


def test_adaptation_and_info_count_moves(tmp_path, monkeypatch):
  """Negative steps: the 0.95 recursion runs once per move, the +-2 % rule once per step; .MCMC_info reports per move."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck, path = _deck27(tmp_path, 2, initial=-6)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  s = MCMCSampler(read, energy=energy_fn(read, "soft")[0], moves="single")
  step0 = s.max_translation
  s.run()
  ratio, step = 0.5, step0
  for k in range(8):                       # steps -6 ... 1, two moves each
    for ok in s.accepted[2 * k:2 * k + 2]:
      ratio = ratio * 0.95 + (0.05 if ok else 0.0)
    if k - 6 < 0 and k - 6 < -6 // 2:
      step *= 1.02 if ratio > 0.5 else 0.98
  assert len(s.accepted) == 16 and s.max_translation == step and step != step0 and s.acceptance_ratio == ratio
  text = open("run.MCMC_info").read().splitlines()
  assert text[0] == "acceptance ratio = " + str(sum(s.accepted) / 16.0) and text[1] == "accepted_moves = " + str(sum(s.accepted))


def test_all_body_mode_is_unchanged(tmp_path, monkeypatch):
  """moves="all" (and the default) replay a recorded chain of the reference exactly as before."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  for kw in ({}, {"moves": "all"}):
    g, deck = load_case(FIXTURES[0], str(tmp_path))
    monkeypatch.chdir(tmp_path)
    read = ReadInput(deck)
    s = MCMCSampler(read, potential=str(g["potential"]), energy=energy_fn(read, str(g["potential"]))[0], keep_saved=True, **kw)
    s.run()
    assert_chain_matches(s, g, 1e-13)
    assert s.energy_drift == {} and open("run.MCMC_info").read().splitlines()[1] == str(g["mcmc_info"][1])


def test_refused_arguments(tmp_path, monkeypatch):
  from rigidmultiblobswall_amd import mcmc
  deck, path = _deck27(tmp_path, 2)
  monkeypatch.chdir(tmp_path)
  with pytest.raises(ValueError, match="moves"):
    mcmc.MCMCSampler(ReadInput(path), energy=lambda r: 0.0, moves="some")
  with pytest.raises(ValueError, match="device index"):
    mcmc.MCMCSampler(ReadInput(path), device=[0, 1], moves="single")
  with pytest.raises(SystemExit):
    mcmc.main(["data.main", "--moves", "pairs"])


def test_prescribed_bodies_are_never_moved(tmp_path, monkeypatch):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck = deck_of(27, seed=1)
  path = write_deck(str(tmp_path), deck, [("structure", "boom", [0]), ("obstacle", "shell", [1])], LINES % (6, 0))
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  s = MCMCSampler(read, energy=energy_fn(read, "soft")[0], write_files=False, moves="single").run()
  loc, quat = s.state.configuration()
  assert s.n_free == 1 and len(s.accepted) == 6 and any(s.accepted)
  assert np.array_equal(loc[1], s.loc0[1]) and np.array_equal(quat[1], s.quat0[1]) and not np.array_equal(loc[0], s.loc0[0])      # (as read from the files)


@pytest.mark.parametrize("form", ["soft", "yukawa"])
@pytest.mark.parametrize("periodic", [False, True], ids=["open", "periodic"])
@pytest.mark.parametrize("case", GATE_CASES)
def test_difference_rule_equals_the_difference_of_totals(case, periodic, form):
  """The rule of the kernel, stated in numpy, against energy(new) - energy(old) of the restatement, both in long double:
  they differ by the rounding of two sums of 66 + 2145 terms, bounded by 1e3 eps sum|terms| (1e-16 of the scale in long
  double)."""
  deck, r, first, new = gate_case(case, periodic)
  kw = potential_kw(form, deck.L)
  d_one, d_pair, S_one, S_pair = delta_rule(r, first, new, **kw)
  r_new = r.copy()
  r_new[first:first + len(new)] = new
  n1, n2, Sn1, Sn2 = potnp.energy(r_new, split=True, **kw)
  o1, o2, So1, So2 = potnp.energy(r, split=True, **kw)
  tol = 1e3 * np.finfo(potnp.EXT).eps
  assert abs(d_one - (n1 - o1)) <= tol * (Sn1 + So1) and abs(d_pair - (n2 - o2)) <= tol * (Sn2 + So2)
  assert S_one > 0 and S_pair > 0 and d_pair != 0
  # the case does put a blob behind the wall where it says
  below_old, below_new = np.flatnonzero(r[:, 2] <= 0), np.flatnonzero(r_new[:, 2] <= 0)
  expect = {"before_only": ([first + 4], []), "after_only": ([], [first + 4]), "lower_body_not_moved": ([7, 20], [7, 20]),
            "moved_body_lower_index": ([first], [first]), "moved_body_higher_index": ([first + len(new) - 1], [first + len(new) - 1])}[case]
  assert list(below_old) == expect[0] and list(below_new) == expect[1]
