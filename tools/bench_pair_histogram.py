#!/usr/bin/env python
"""The pair-distance histogram behind g(r) on one GPU, against the energy sweep whose schedule it runs on.

Resident sweep: rmb_pair_histogram_device against rmb_body_body_potential on the SAME resident points in the same process --
4096 and 262 144 centres of the jittered square lattice of tools/bench_body_potential.py (pitch 1.3, periodic in x and y,
eps = 1.7, b = 0.9: the energy's cull distance of 750 b exceeds both boxes, so it meets every pair).  Rows per size:
  unculled   "force_cull" 0, r_max = 10 mean spacings: both sweeps meet every pair; `ratio` = histogram / energy
  half_box   "force_cull" 0, r_max = box / 2 (the reference program's reach): every pair met, ~78 % of them counted
  culled     "force_cull" 1, r_max = 10 mean spacings: what a g(r) of a large frame costs
Device time from the library's events around the sweep kernel, primed, median of --events calls; 2000 bins.

Batch entry: rmb_pair_histogram_frames_device on --frames frames of 1875 points (the reference example's N) in a 40 x 16 box,
r_max = lx / 2, 2000 bins, one launch; torch events around the call, primed, median of --events calls.

  python tools/bench_pair_histogram.py [--out FILE.json] [--centres 4096 262144] [--frames 1000] [--events 21]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_body_potential import B, EPS, _monolayer  # noqa: E402

N_BINS = 2000
SPACING = 1.3


def _library_timed(ctx, call, events):
  for _ in range(3):
    call()
  ctx.set_option("timing", 1)
  ctx.timing_reset()
  for _ in range(events):
    call()
  torch.cuda.synchronize()
  ring = np.asarray(ctx.timing_collect()[-events:])
  ctx.set_option("timing", 0)
  assert len(ring) == events
  return dict(device_ms_median=float(np.median(ring)), device_ms_min=float(np.min(ring)), events=int(len(ring)))


def resident(n, events):
  from rigidmultiblobswall_amd import MobilityContext
  x, box = _monolayer(n)
  ctx = MobilityContext(0)
  rows = []
  try:
    ctx.set_positions(x, 1.0, np.array([box, box, 0.0]), wall=False)
    energy = _library_timed(ctx, lambda: ctx.body_body_potential(EPS, B), events)
    for name, cull, r_max in (("unculled", 0, 10 * SPACING), ("half_box", 0, 0.5 * box), ("culled", 1, 10 * SPACING)):
      ctx.set_option("force_cull", cull)
      out = torch.zeros(N_BINS, dtype=torch.int64, device="cuda")
      t = _library_timed(ctx, lambda: ctx.pair_histogram_device(r_max, N_BINS, out=out), events)
      counted = int(ctx.pair_histogram(r_max, N_BINS).sum())
      rows.append(dict(kind="resident_" + name, centres=n, box=box, r_max=r_max, n_bins=N_BINS, force_cull=cull, pair_histogram=t,
                       body_body_potential=energy, ratio=t["device_ms_median"] / energy["device_ms_median"], pairs=n * (n - 1) // 2,
                       pairs_counted=counted))
    ctx.set_option("force_cull", 1)
  finally:
    ctx.close()
  return rows


def batch(n_frames, events, n=1875):
  from rigidmultiblobswall_amd import MobilityContext
  rng = np.random.RandomState(17)
  L = np.array([40.0, 16.0, 0.0])
  frames = torch.from_numpy(rng.uniform(0, 1, (n_frames, n, 3)) * np.array([40.0, 16.0, 1.2])).cuda()
  ctx = MobilityContext(0)
  try:
    out = torch.zeros(N_BINS, dtype=torch.int64, device="cuda")
    call = lambda: ctx.pair_histogram_frames_device(frames, L, 0.5 * L[0], N_BINS, out=out)   # noqa: E731
    for _ in range(3):
      call()
    ms = []
    for _ in range(events):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      call()
      e1.record()
      e1.synchronize()
      ms.append(e0.elapsed_time(e1))
    pairs = n_frames * n * (n - 1) // 2
    med = float(np.median(ms))
    return dict(kind="batch", frames=n_frames, points=n, r_max=0.5 * L[0], n_bins=N_BINS, device_ms_median=med, device_ms_min=float(np.min(ms)),
                events=events, pairs=pairs, pairs_counted=int(out.sum().item()) // (events + 3), gpairs_per_s=pairs / med * 1e-6)
  finally:
    ctx.close()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--centres", type=int, nargs="*", default=[4096, 262144])
  ap.add_argument("--frames", type=int, default=1000)
  ap.add_argument("--events", type=int, default=21)
  args = ap.parse_args()
  events = max(20, args.events)
  rows = []
  for n in args.centres:
    for row in resident(n, events):
      rows.append(row)
      print(json.dumps(row), flush=True)
  if args.frames > 0:
    rows.append(batch(args.frames, events))
    print(json.dumps(rows[-1]), flush=True)
  res = dict(device=torch.cuda.get_device_name(0), rows=rows)
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(res, fh, indent=1)


if __name__ == "__main__":
  main()
