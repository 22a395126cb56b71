"""Shared by the host and GPU sampler tests: write a g14_mcmc_* fixture's deck and structure files into a directory and
compare a finished MCMCSampler with what the reference's driver recorded."""
import os

import numpy as np

from conftest import golden_files, load_golden

FIXTURES = golden_files("g14_mcmc_*.npz")
IDS = [os.path.basename(p)[len("g14_mcmc_"):-4] for p in FIXTURES]


def write_case(g, directory):
  """-> path of the deck; the structure files lie next to it under the names the deck uses (s<k>.vertex / s<k>.clones)."""
  for k in range(int(g["n_structures"])):
    vert, loc, quat = g["vertex_%d" % k], g["start_loc_%d" % k], g["start_quat_%d" % k]
    with open(os.path.join(directory, "s%d.vertex" % k), "w") as f:
      f.write("%d\n" % len(vert) + "".join("%.17g %.17g %.17g\n" % tuple(x) for x in vert))
    with open(os.path.join(directory, "s%d.clones" % k), "w") as f:
      f.write("%d\n" % len(loc) + "".join("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" % (tuple(x) + tuple(q)) for x, q in zip(loc, quat)))
  deck = os.path.join(directory, "data.main")
  with open(deck, "w") as f:
    f.write(str(g["deck"]))
  return deck


def load_case(path, directory):
  g = load_golden(path)
  return g, write_case(g, directory)


def assert_chain_matches(sampler, g, energy_rtol):
  """Accept / reject sequence identical, energy log to energy_rtol, saved configurations to 1e-12, the .MCMC_info numbers."""
  assert sampler.accepted == [bool(x) for x in g["accepted"]]
  assert sampler.accepted_moves == int(g["accepted_moves"])
  log, ref = np.array(sampler.energy_log), g["energy_log"]
  assert log.shape == ref.shape
  worst = np.max(np.abs(log - ref) / np.abs(ref))
  print("energy log: worst relative difference %.3e over %d values" % (worst, ref.size))
  assert worst <= energy_rtol
  assert sorted(sampler.saved) == [int(s) for s in g["saved_steps"]]
  offset = 0
  for k in range(int(g["n_structures"])):
    nb = g["start_loc_%d" % k].shape[0]
    for i, step in enumerate(g["saved_steps"]):
      loc, quat = sampler.saved[int(step)]
      assert np.max(np.abs(loc[offset:offset + nb] - g["saved_loc_%d" % k][i])) <= 1e-12
      assert np.max(np.abs(quat[offset:offset + nb] - g["saved_quat_%d" % k][i])) <= 1e-12
    offset += nb
  assert sampler.max_translation == float(g["max_translation"]) or abs(sampler.max_translation / float(g["max_translation"]) - 1) <= 1e-14
  assert abs(sampler.max_angle_shift / float(g["max_angle_shift"]) - 1) <= 1e-14


def info_numbers(lines):
  return [float(str(l).split("=")[1]) for l in lines]
