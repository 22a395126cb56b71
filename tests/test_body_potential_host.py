"""Body-body Yukawa energy in the equilibrium sampler, host side: the C exports, MCMCSampler(energy=f, body_potential=...)
on the numpy twin -- both move kinds log f(r) + U_body(loc) against the long-double restatement
(_body_forces_numpy.energy), a zero strength changes no decision -- and the refused arguments.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import _body_forces_numpy as bfn
from conftest import ROOT
from _mcmc_moves_common import deck_of, energy_fn, write_deck
from rigidmultiblobswall_amd.read_input import ReadInput

EPS, B = 1.7, 0.9
LINES = ("n_steps %d\nn_save 1\ninitial_step 0\ng 0.6\nblob_radius 0.2\nkT 0.05\nperiodic_length %r %r %r\nrepulsion_strength_wall 0.8\n"
         "debye_length_wall 0.12\nrepulsion_strength 0.35\ndebye_length 0.09\nseed 21\noutput_name run\n")
STRUCTURES66 = [("structure", "boom", [0, 1]), ("structure", "shell", [2, 3, 4])]


def _deck66(tmp_path, steps, periodic, Lz=0.0, extra=""):
  deck = deck_of(66, seed=3, periodic=periodic)
  if Lz == "z":      # a period in z short enough that the two centres furthest apart in z meet through the image
    dz = np.abs(deck.loc[:, None, 2] - deck.loc[None, :, 2]).max()
    Lz = 1.25 * dz
  L = (float(deck.L[0]), float(deck.L[1]), float(Lz))
  return deck, write_deck(str(tmp_path), deck, STRUCTURES66, LINES % ((steps,) + L) + extra)


def test_the_exports_exist_and_refuse_a_null_context():
  from rigidmultiblobswall_amd import _lib
  lib = _lib.load()
  header = open(os.path.join(ROOT, "include", "rmb_mobility.h")).read()
  for name in ("rmb_body_body_potential", "rmb_body_body_potential_device", "rmb_mcmc_body_delta_bb_device", "rmb_mcmc_sweep_bb_device"):
    assert name in _lib.SYMBOLS and ("int %s(" % name) in header
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
  assert lib.rmb_body_body_potential(None, 1.0, 1.0, None) < 0 and lib.rmb_body_body_potential_device(None, 1.0, 1.0, None) < 0
  pot = (0.3, 0.1, 0.0, 1.0, 0.0, 0.2, 0)
  assert lib.rmb_mcmc_body_delta_bb_device(None, 1, None, 0, 1, None, 1, None, 0, None, None, *pot, 1.0, 1.0, None) < 0
  assert lib.rmb_mcmc_sweep_bb_device(None, 1, 1, 1, None, None, None, None, None, None, None, 0.1, None, *pot, 1.0, 1.0, 0.1, None, None) < 0


def test_the_numpy_twin_of_the_energy_is_the_restatement():
  """mcmc.body_body_energy (double) against the long-double restatement: open, x-y periodic and periodic in z as well."""
  from rigidmultiblobswall_amd.mcmc import body_body_energy
  x, box = bfn.lattice_cloud(65, seed=65)
  for L in (np.zeros(3), np.array([box, box, 0.0]), np.array([box, box, box])):
    ref = bfn.energy(x, L, EPS, B)
    got = body_body_energy(x, L, EPS, B)
    assert abs(got - ref) <= 1e-13 * ref and ref > 0
  assert body_body_energy(x[:1], np.zeros(3), EPS, B) == 0.0


@pytest.mark.parametrize("moves", ["all", "single"])
@pytest.mark.parametrize("periodic, Lz", [(False, 0.0), (True, 0.0), (True, "z")], ids=["open", "xy", "xyz"])
def test_logged_energies_are_the_callers_plus_the_body_term(moves, periodic, Lz, tmp_path, monkeypatch):
  """66 blobs, 5 bodies, 6 steps.  moves="all": energy_log[k + 1] is the energy of proposal k, whose configuration is the
  saved one when it was accepted; moves="single": energy_log[k + 1] is the running energy = the energy of the configuration
  saved after sweep k.  Every logged energy whose configuration is known is f(r) + U_body(loc) of the long-double
  restatement, to 1e-13 of |f| + U_body (the double evaluation of ten positive terms and one addition)."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck, path = _deck66(tmp_path, 6, periodic, Lz)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  f, _ = energy_fn(read, "soft")
  s = MCMCSampler(read, energy=f, write_files=False, moves=moves, body_potential=(EPS, B)).run()
  off = MCMCSampler(read, energy=f, write_files=False, moves=moves)
  L = np.asarray(read.periodic_length, dtype=np.float64)
  assert (L[2] > 0) == (Lz == "z") and s.body_potential == (EPS, B)
  if L[2] > 0:      # a centre pair meets through the z image
    dz = np.abs(deck.loc[:, None, 2] - deck.loc[None, :, 2])
    assert (dz > 0.5 * L[2]).any()

  def total(loc, quat):
    u_f, u_b = f(s.state._blobs(loc, quat)), float(bfn.energy(loc, L, EPS, B))
    return u_f + u_b, abs(u_f) + u_b

  want, scale = total(s.loc0, s.quat0)
  assert abs(s.energy_log[0] - want) <= 1e-13 * scale and abs(s.energy_log[0] - off.state.current_energy()) > 1e-3 * scale
  checked = 0
  for step in range(6):
    if moves == "single" or s.accepted[step]:
      want, scale = total(*s.saved[step])
      assert abs(s.energy_log[step + 1] - want) <= 1e-13 * scale, (step, s.energy_log[step + 1], want)
      checked += 1
  assert checked >= 2 and len(s.energy_log) == 7
  if moves == "single":      # the twin's running energy IS a full evaluation, body term included
    assert all(run == full for run, full in s.energy_drift.values())
    assert 0 < s.accepted_moves < len(s.accepted) == 30


@pytest.mark.parametrize("moves", ["all", "single"])
def test_zero_strength_changes_nothing(moves, tmp_path, monkeypatch):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck, path = _deck66(tmp_path, 6, True)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  f, _ = energy_fn(read, "soft")
  a = MCMCSampler(read, energy=f, write_files=False, moves=moves, body_potential=(0.0, B)).run()
  b = MCMCSampler(read, energy=f, write_files=False, moves=moves).run()
  assert a.accepted == b.accepted and a.energy_log == b.energy_log and any(a.accepted)
  for step in b.saved:
    assert np.array_equal(a.saved[step][0], b.saved[step][0]) and np.array_equal(a.saved[step][1], b.saved[step][1])


def test_the_body_term_changes_the_chain(tmp_path, monkeypatch):
  """A body law strong against kT (a move of 0.02 changes U_body by several kT): some decision of the 30 moves differs from
  the chain without it."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck, path = _deck66(tmp_path, 6, False)
  monkeypatch.chdir(tmp_path)
  read = ReadInput(path)
  f, _ = energy_fn(read, "soft")
  a = MCMCSampler(read, energy=f, write_files=False, moves="single", body_potential=(100.0 * EPS, B)).run()
  b = MCMCSampler(read, energy=f, write_files=False, moves="single").run()
  assert a.accepted != b.accepted and len(a.accepted) == 30


def test_refused_arguments_and_the_deck_keyword(tmp_path, monkeypatch):
  from rigidmultiblobswall_amd import mcmc
  deck, path = _deck66(tmp_path, 2, False)
  monkeypatch.chdir(tmp_path)
  f = lambda r: 0.0      # noqa: E731
  with pytest.raises(ValueError, match="body_body_force_torque_implementation"):
    mcmc.MCMCSampler(ReadInput(path), energy=f, body_potential="deck")
  for bad in ((1.0,), (1.0, 2.0, 3.0), 1.0, ("a", "b"), "yukawa"):
    with pytest.raises(ValueError, match="body_potential"):
      mcmc.MCMCSampler(ReadInput(path), energy=f, body_potential=bad)
  for b in (0.0, -1.0, float("nan")):
    with pytest.raises(ValueError, match="debye_length"):
      mcmc.MCMCSampler(ReadInput(path), energy=f, body_potential=(1.0, b))
  with pytest.raises(SystemExit):
    mcmc.main(["data.main", "--body-potential", "1.0;2.0"])
  # a deck that names the option: "deck" is the steppers' pair of numbers, and .MCMC_info names the law
  for impl in ("python", "hip"):
    deck, path = _deck66(tmp_path, 2, False, extra="body_body_force_torque_implementation %s\n" % impl)
    read = ReadInput(path)
    s = mcmc.MCMCSampler(read, energy=f, body_potential="deck")
    assert s.body_potential == (read.repulsion_strength, read.debye_length) == (0.35, 0.09)
    s.run()
    info = open("run.MCMC_info").read().splitlines()
    assert len(info) == 5 and info[4] == "body_potential = yukawa repulsion_strength 0.35 debye_length 0.09"
    # without the keyword the option stays ignored, as in the reference sampler
    s = mcmc.MCMCSampler(read, energy=f).run()
    assert s.body_potential is None and len(open("run.MCMC_info").read().splitlines()) == 4


def test_bodies_potential_keeps_its_default():
  from rigidmultiblobswall_amd import potential
  assert potential.bodies_potential_hip([]) == 0.0 and potential.bodies_potential_hip([], periodic_length=np.zeros(3)) == 0.0
  with pytest.raises(ValueError, match="debye_length"):
    potential.bodies_potential_hip(np.zeros((2, 3)), body_potential=(1.0, 0.0))
