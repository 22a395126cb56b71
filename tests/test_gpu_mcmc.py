"""The Metropolis sampler on the device: replays of the reference driver's recorded chains (g14_mcmc_*), the command line's
file set, repeatability of seeded chains, and the equilibrium height distribution of one blob above the wall."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _potential_numpy as potnp
from _mcmc_common import FIXTURES, IDS, assert_chain_matches, info_numbers, load_case
from conftest import ROOT
from rigidmultiblobswall_amd.read_input import ReadInput

pytestmark = pytest.mark.gpu


def _device_sampler(path, tmp_path, monkeypatch, **kw):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  g, deck = load_case(path, str(tmp_path))
  monkeypatch.chdir(tmp_path)
  return g, MCMCSampler(ReadInput(deck), device=0, potential=str(g["potential"]), keep_saved=True, **kw)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_device_replay_of_the_reference_chain(path, tmp_path, monkeypatch):
  g, s = _device_sampler(path, tmp_path, monkeypatch)
  try:
    s.run()
  finally:
    s.close()
  assert_chain_matches(s, g, 1e-12)
  text = open("run.MCMC_info").read().splitlines()
  assert np.allclose(info_numbers(text), info_numbers(g["mcmc_info"]), rtol=1e-14, atol=0) and text[1] == str(g["mcmc_info"][1])


@pytest.mark.parametrize("name", ["boomerang_periodic_soft", "shells_yukawa"])
def test_command_line_writes_the_reference_file_set(name, tmp_path):
  path = [p for p in FIXTURES if name in p][0]
  g, deck = load_case(path, str(tmp_path))
  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
  out = subprocess.run([sys.executable, "-m", "rigidmultiblobswall_amd.mcmc", "--potential", str(g["potential"])], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)      # the deck is data.main: the default argument
  assert out.returncode == 0, out.stdout + out.stderr
  files = set(os.listdir(str(tmp_path)))
  assert {"run.inputfile", "run.random_state", "run.time", "run.MCMC_info"} <= files
  if "one_file_per_step" in str(g["deck"]):
    assert {"run.s0.%08d.clones" % int(s) for s in g["saved_steps"]} <= files and not any(f.endswith(".config") for f in files)
  else:
    assert "run.s0.config" in files and not any(f.startswith("run.s0.0") for f in files)
    rows = open(os.path.join(str(tmp_path), "run.s0.config")).read().splitlines()
    assert len(rows) == (g["start_loc_0"].shape[0] + 1) * len(g["saved_steps"])
  text = open(os.path.join(str(tmp_path), "run.MCMC_info")).read().splitlines()
  assert text[1] == str(g["mcmc_info"][1])
  assert np.allclose(info_numbers(text), info_numbers(g["mcmc_info"]), rtol=1e-14, atol=0)


@pytest.mark.parametrize("rng", ["reference", "batched"])
def test_a_seeded_chain_is_bit_repeatable(rng, tmp_path, monkeypatch):
  runs = []
  for _ in range(2):
    g, s = _device_sampler(FIXTURES[0], tmp_path, monkeypatch, rng=rng, write_files=False)
    try:
      s.run()
    finally:
      s.close()
    runs.append(s)
  a, b = runs
  assert a.energy_log == b.energy_log and a.accepted == b.accepted
  for step in a.saved:
    assert np.array_equal(a.saved[step][0], b.saved[step][0]) and np.array_equal(a.saved[step][1], b.saved[step][1])


def _shell_deck(directory, n_bodies, steps):
  from rigidmultiblobswall_amd.structures import icosahedron_shell, roller_monolayer
  loc, q, side = roller_monolayer(n_bodies, radius=1.0, phi2d=0.25, seed=2)
  with open(os.path.join(directory, "shell.vertex"), "w") as f:
    f.write("12\n" + "".join("%.17g %.17g %.17g\n" % tuple(x) for x in icosahedron_shell(0.7921)))
  with open(os.path.join(directory, "shell.clones"), "w") as f:
    f.write("%d\n" % n_bodies + "".join("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" % (tuple(x) + tuple(p)) for x, p in zip(loc, q)))
  deck = os.path.join(directory, "data.main")
  with open(deck, "w") as f:
    f.write("n_steps %d\nn_save %d\ninitial_step 0\ng 0.0124\nblob_radius 0.416\nkT 0.0041419464\nperiodic_length %.17g %.17g 0\n"
            "repulsion_strength_wall 0.03\ndebye_length_wall 0.04\nrepulsion_strength 0.03\ndebye_length 0.04\nseed 4\n"
            "output_name run\nstructure shell.vertex shell.clones\n" % (steps, steps // 2, float(side), float(side)))
  return deck


@pytest.mark.parametrize("rng", ["reference", "batched"])
def test_a_chain_on_the_sorted_path_is_bit_repeatable(rng, tmp_path, monkeypatch):
  """208 twelve-blob shells = 2496 blobs = 39 tiles: the sweep runs on the Morton-sorted copy and, over 40 steps, through
  the reuse schedule of "potential_resort" (rebuilt on evaluations 0, 16, 32, regathered in between).  Two runs are
  identical to the bit; a run that rebuilds the permutation on every evaluation sums in another order and agrees to
  rounding, with the same decisions."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck = _shell_deck(str(tmp_path), 208, 40)
  monkeypatch.chdir(tmp_path)
  runs = []
  for resort in (None, None, 1):
    s = MCMCSampler(ReadInput(deck), device=0, rng=rng, write_files=False)
    try:
      assert s.n_blobs == 2496 and s.state.ctx.get_option("potential_resort") == 16
      if resort is not None:
        s.state.ctx.set_option("potential_resort", resort)
      s.run()
    finally:
      s.close()
    runs.append(s)
  a, b, c = runs
  assert a.energy_log == b.energy_log and a.accepted == b.accepted and 0 < a.accepted_moves < 40
  for step in a.saved:
    assert np.array_equal(a.saved[step][0], b.saved[step][0]) and np.array_equal(a.saved[step][1], b.saved[step][1])
  worst = np.max(np.abs(np.array(a.energy_log) - np.array(c.energy_log)) / np.abs(np.array(c.energy_log)))
  print("reused against rebuilt permutation: worst relative energy difference %.3e" % worst)
  assert worst <= 1e-12 and a.accepted == c.accepted


# ---- one blob above the wall: the sampled height distribution ---------------------------------------------------------
A, W, EW, BW, KT, STEPS, SEED = 0.25, 0.5, 0.2, 0.1, 0.05, 20000, 1


def _single_blob_deck(directory):
  with open(os.path.join(directory, "blob.vertex"), "w") as f:
    f.write("1\n0 0 0\n")
  with open(os.path.join(directory, "blob.clones"), "w") as f:
    f.write("1\n0 0 0.5 1 0 0 0\n")
  deck = os.path.join(directory, "data.main")
  with open(deck, "w") as f:
    f.write("n_steps %d\nn_save 1\ninitial_step 0\ng %r\nblob_radius %r\nkT %r\nrepulsion_strength_wall %r\ndebye_length_wall %r\n"
            "repulsion_strength 0.1\ndebye_length 0.1\nseed %d\noutput_name run\nstructure blob.vertex blob.clones\n" % (STEPS, W, A, KT, EW, BW, SEED))
  return deck


def _mean_height_by_quadrature():
  h = np.linspace(1e-6, 3.0, 600001)
  u = np.array(potnp.one_blob_terms(h, potnp.EXT(EW), potnp.EXT(BW), potnp.EXT(W), potnp.EXT(A), "soft"), dtype=np.float64)
  p = np.exp(-(u - u.min()) / KT)
  trapezoid = lambda f: np.sum((f[1:] + f[:-1]) * np.diff(h)) / 2      # noqa: E731
  return trapezoid(h * p) / trapezoid(p)           # beyond h = 3 the weight is e^-25 of the peak's


def _batch_means(heights, batches=20):
  m = np.array([b.mean() for b in np.array_split(heights, batches)])
  return heights.mean(), m.std(ddof=1) / np.sqrt(batches)


def test_single_blob_height_distribution(tmp_path, monkeypatch):
  """20 000 seeded steps of one blob (soft form): the mean height lies within five batch-means standard errors of the
  quadrature of exp(-U(h)/kT).  The same chain is run with the numpy restatement first; the device chain must make the
  same decisions."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  deck = _single_blob_deck(str(tmp_path))
  monkeypatch.chdir(tmp_path)
  exact = _mean_height_by_quadrature()
  read = ReadInput(deck)
  kw = dict(periodic_length=read.periodic_length, debye_length_wall=BW, repulsion_strength_wall=EW, debye_length=0.1, repulsion_strength=0.1,
            weight=W, blob_radius=A)
  cpu = MCMCSampler(read, energy=lambda r: potnp.total(r, **kw), write_files=False).run()
  gpu = MCMCSampler(ReadInput(deck), device=0, write_files=False)
  try:
    gpu.run()
  finally:
    gpu.close()
  for name, s in (("restatement", cpu), ("device", gpu)):
    heights = np.array([s.saved[k][0][0, 2] for k in range(STEPS)])
    mean, se = _batch_means(heights)
    print("%s: mean height %.6f, quadrature %.6f, batch-means standard error %.6f, acceptance %.3f" % (name, mean, exact, se, s.accepted_moves / STEPS))
    assert abs(mean - exact) <= 5 * se
  assert gpu.accepted == cpu.accepted
