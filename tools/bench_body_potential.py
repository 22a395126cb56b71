#!/usr/bin/env python
"""The body-body Yukawa energy of the equilibrium sampler on one GPU, against what it is an instance of.

Energy sweep: rmb_body_body_potential against rmb_blob_potential form "yukawa" on the SAME resident points in the same
process -- 4096 and 262 144 centres of a jittered square lattice of pitch 1.3 above z = 0 (no blob behind the wall, so the
blob form gates nothing), periodic in x and y, eps = 1.7, b = 0.9 (the cull distance of 750 b exceeds both boxes: every
pair is evaluated by both).  Device time from the library's events around the sweep, primed, median of --events calls.

Sweep of single-body moves: MCMCSampler(moves="single") with body_potential=(eps, b) against without, on 1000 and 21 845
twelve-blob shells (the deck of tools/bench_mcmc_moves.py), rng="batched", the same seeded draws; device time from the
library's events around the whole sweep (2 n_free launches), primed, median of --events sweeps.

  python tools/bench_body_potential.py [--out FILE.json] [--centres 4096 262144] [--bodies 1000 21845] [--events 21]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

EPS, B = 1.7, 0.9
SHELL_LAW = (0.03, 0.4)      # the shells' deck: its repulsion_strength, a range of the order of the body radius


def _monolayer(n, seed=16, spacing=1.3):
  rng = np.random.RandomState(seed)
  m = int(np.ceil(np.sqrt(n)))
  k = rng.permutation(m * m)[:n]
  x = np.stack([(k % m) * spacing, (k // m) * spacing, np.zeros(n)], axis=1)
  x += 0.1 * (2.0 * rng.rand(n, 3) - 1.0) + 0.5 * spacing
  x[:, 2] += 1.0 + 2.0 * rng.rand(n)
  return x, spacing * m


def _timed(ctx, call, events):
  for _ in range(3):
    call()
  ctx.set_option("timing", 1)
  ctx.timing_reset()
  values = [call() for _ in range(events)]
  torch.cuda.synchronize()
  ring = np.asarray(ctx.timing_collect()[-events:])
  ctx.set_option("timing", 0)
  assert len(ring) == events and len(set(values)) == 1
  return dict(device_ms_median=float(np.median(ring)), device_ms_min=float(np.min(ring)), events=int(len(ring))), values[0]


def energy_sweep(n, events):
  from rigidmultiblobswall_amd import MobilityContext
  x, box = _monolayer(n)
  ctx = MobilityContext(0)
  try:
    ctx.set_positions(x, 1.0, np.array([box, box, 0.0]), wall=False)
    body, u_body = _timed(ctx, lambda: ctx.body_body_potential(EPS, B), events)
    blob, u_blob = _timed(ctx, lambda: ctx.blob_potential(EPS, B, 1.0, potential="yukawa")[1], events)
  finally:
    ctx.close()
  return dict(kind="energy_sweep", centres=n, box=box, body_body_potential=body, blob_potential_yukawa=blob,
              ratio=body["device_ms_median"] / blob["device_ms_median"], expected_at_most=1.10,
              u_body=u_body, u_blob_pair=u_blob, relative_difference_of_the_two_sums=abs(u_body - u_blob) / u_blob)


def _sweeps(nb, law, events):
  from bench_mcmc_moves import _phase
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  from rigidmultiblobswall_amd.read_input import ReadInput
  s = MCMCSampler(ReadInput("data.main"), device=0, rng="batched", write_files=False, keep_saved=False, moves="single", body_potential=law)
  try:
    rng = np.random.RandomState(1)
    _phase(s, rng, 0, 3)                       # priming (clocks, allocations)
    ctx = s.state.ctx
    ctx.set_option("timing", 1)
    ctx.timing_reset()
    wall, flags = _phase(s, rng, 0, events + 1)
    ring = np.asarray(ctx.timing_collect())
    ctx.set_option("timing", 0)
    # the phase's events on the blob context: the energy sweep of its start configuration, sweep 0, the energy sweep of the save
    # of step 0, then one event per sweep of moves: the last `events` are sweeps 1 ... events
    assert len(ring) == events + 3
    ring = ring[-events:]
    return dict(bodies=nb, blobs=s.n_blobs, body_potential=law, device_ms_median=float(np.median(ring)), device_ms_min=float(np.min(ring)),
                events=int(len(ring)), sweep_wall_ms=1e3 * wall / (events + 1), acceptance=float(np.mean(flags)))
  finally:
    s.close()


def move_sweep(nb, events):
  from bench_mcmc_moves import _write_deck
  cwd = os.getcwd()
  with tempfile.TemporaryDirectory() as tmp:
    os.chdir(tmp)
    try:
      _write_deck(nb)
      without = _sweeps(nb, None, events)
      with_term = _sweeps(nb, SHELL_LAW, events)
    finally:
      os.chdir(cwd)
  return dict(kind="single_body_sweep", bodies=nb, without_the_term=without, with_the_term=with_term,
              ratio=with_term["device_ms_median"] / without["device_ms_median"], expected_at_most=1.15)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--centres", type=int, nargs="*", default=[4096, 262144])
  ap.add_argument("--bodies", type=int, nargs="*", default=[1000, 21845])
  ap.add_argument("--events", type=int, default=21)
  args = ap.parse_args()
  events = max(20, args.events)
  rows = []
  for n in args.centres:
    rows.append(energy_sweep(n, events))
    print(json.dumps(rows[-1]), flush=True)
  for nb in args.bodies:
    rows.append(move_sweep(nb, events))
    print(json.dumps(rows[-1]), flush=True)
  res = dict(device=torch.cuda.get_device_name(0), rows=rows)
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(res, fh, indent=1)


if __name__ == "__main__":
  main()
