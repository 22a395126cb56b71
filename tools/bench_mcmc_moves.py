#!/usr/bin/env python
"""All-body steps against sweeps of single-body moves of the equilibrium sampler (mcmc.py, moves="all" | "single") on one GPU:
1000 and 21 845 twelve-blob shells on the monolayer of roller_monolayer, rng="batched".

Per deck and mode the chain first adapts its step size (the +-2 % rule over the first half of the negative steps, the second
half at the adapted size), then runs the timed phase.  Recorded per mode: the device time per all-body step (the library's
events around the energy sweep) or per sweep of single-body moves (the library's events around the whole sweep, 2 n_free
launches), median and minimum; the wall time per step of the timed phase (host included); the acceptance of the timed phase;
the adapted max_translation; and the mean squared displacement of the body centres over the timed phase per second of its
wall time -- with the ratio single / all of those rates, whichever way it falls.  The single-body run of the large deck
starts its adaptation from the step size the small deck adapted to (a single-body step does not depend on the number of
bodies at equal density), so that a few dozen sweeps suffice.

  python tools/bench_mcmc_moves.py [--out FILE.json] [--bodies 1000 21845] [--steps-all 200] [--sweeps 20]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _write_deck(nb):
  from rigidmultiblobswall_amd.structures import icosahedron_shell, roller_monolayer
  shell = icosahedron_shell(0.7921)
  loc, q, side = roller_monolayer(nb, radius=1.0, phi2d=0.25, seed=2)
  with open("shell.vertex", "w") as f:
    f.write("12\n" + "".join("%.17g %.17g %.17g\n" % tuple(x) for x in shell))
  with open("shell.clones", "w") as f:
    f.write("%d\n" % nb + "".join("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" % (tuple(x) + tuple(p)) for x, p in zip(loc, q)))
  with open("data.main", "w") as f:       # the deck of tools/bench_potential.py's mcmc_steps
    f.write("n_steps 1\nn_save 1000000\ninitial_step 0\ng 0.0124\nblob_radius 0.416\nkT 0.0041419464\nperiodic_length %r %r 0\n"
            "repulsion_strength_wall 0.03\ndebye_length_wall 0.04\nrepulsion_strength 0.03\ndebye_length 0.04\nseed 1\n"
            "output_name run\nstructure shell.vertex shell.clones\n" % (float(side), float(side)))


def _phase(s, rng, first_step, last_step):
  """Steps first_step ... last_step - 1 of the chain, continued from the sampler's state.  -> (wall seconds, flags of the phase)"""
  s.read.initial_step, s.read.n_steps = first_step, last_step
  before = len(s.accepted)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  s.run(rng)
  torch.cuda.synchronize()
  return time.perf_counter() - t0, s.accepted[before:]


def measure(nb, mode, adapt_steps, timed_steps, start_translation=None):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  from rigidmultiblobswall_amd.read_input import ReadInput
  s = MCMCSampler(ReadInput("data.main"), device=0, rng="batched", write_files=False, keep_saved=False, moves=mode)
  try:
    if start_translation is not None:
      s.max_translation = start_translation
      s.max_angle_shift = s.max_translation / s.max_body_length
    rng = np.random.RandomState(1)
    # adaptation: the rule acts on steps below initial_step // 2, the rest of the negative steps run at the adapted size
    s.read.initial_step = -2 * adapt_steps
    _phase(s, rng, -2 * adapt_steps, 0)
    _phase(s, rng, 0, 3)                       # priming of the timed phase (clocks, allocations)
    ctx = s.state.ctx
    ctx.set_option("timing", 1)
    ctx.timing_reset()
    loc0 = s.state.configuration()[0].copy()
    wall, flags = _phase(s, rng, 0, timed_steps)
    loc1 = s.state.configuration()[0]
    # the phase's events: the energy of its start configuration, step 0, (single: the energy of the save of step 0,) step 1 ...
    ring = ctx.timing_collect()[-(timed_steps - 1):]
    ctx.set_option("timing", 0)
    msd = float(np.mean(np.sum((loc1[:s.n_free] - loc0[:s.n_free]) ** 2, axis=1)))
    return dict(bodies=nb, blobs=s.n_blobs, moves=mode, timed_steps=timed_steps, adaptation_steps=adapt_steps,
                device_ms_median=float(np.median(ring)), device_ms_min=float(np.min(ring)), events=int(len(ring)),
                step_wall_ms=1e3 * wall / timed_steps, acceptance=float(np.mean(flags)), max_translation=s.max_translation,
                max_translation_over_blob_radius=s.max_translation / s.blob_radius, msd_of_phase=msd, msd_per_second=msd / wall)
  finally:
    s.close()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--bodies", type=int, nargs="+", default=[1000, 21845])
  ap.add_argument("--steps-all", type=int, default=200)
  ap.add_argument("--sweeps", type=int, default=20)
  ap.add_argument("--adapt-all", type=int, default=400)
  ap.add_argument("--adapt-single", type=int, nargs="+", default=[100, 30], help="per deck, in the order of --bodies")
  args = ap.parse_args()
  rows, cwd, single_step = [], os.getcwd(), None
  for k, nb in enumerate(args.bodies):
    with tempfile.TemporaryDirectory() as tmp:
      os.chdir(tmp)
      try:
        _write_deck(nb)
        a = measure(nb, "all", args.adapt_all, max(21, args.steps_all))
        print(json.dumps(a), flush=True)
        b = measure(nb, "single", args.adapt_single[min(k, len(args.adapt_single) - 1)], max(21, args.sweeps), single_step)
        print(json.dumps(b), flush=True)
        single_step = b["max_translation"]
      finally:
        os.chdir(cwd)
    ratio = dict(bodies=nb, msd_per_second_single_over_all=b["msd_per_second"] / a["msd_per_second"] if a["msd_per_second"] > 0 else None,
                 sweep_over_step_device_time=b["device_ms_median"] / a["device_ms_median"],
                 device_us_per_move=1e3 * b["device_ms_median"] / nb)
    print(json.dumps(ratio), flush=True)
    rows += [a, b, ratio]
  res = dict(device=torch.cuda.get_device_name(0), rows=rows)
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(res, fh, indent=1)


if __name__ == "__main__":
  main()
