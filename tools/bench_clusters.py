#!/usr/bin/env python
"""The cluster sweep (rmb_cluster_labels_frames_device, rmb_cluster_labels_device) on one GPU, next to the pair histogram with
r_max = r_cut on the same points in the same run -- the cost of the bond test alone, so the ratio is the price of the unions --
and next to a torch baseline on the same device.

Cases (seeded uniform points in a square box of density ~1.17, z = 0, plane "xy", r_cut = 1.5, as tools/bench_bond_order.py):
  trajectory       1000 frames x 1875 points, box 40 x 40, the batch entry         (the reference example's frame size)
  large_batch      1 frame x 262 144 points, box 473 x 473, the batch entry        (every tile pair met)
  large_resident   the same frame through the resident entry: Morton sort, tile pairs beyond r_cut skipped
  density          one frame of 65 536 points through the batch entry at two bond lengths: dilute (0.3 bonds per point) and
                   one percolating cluster (12 bonds per point) -- how the price depends on the number of bonds
  torch            min-label propagation over a dense adjacency at 1875 points (one frame): labels = min over neighbours, until
                   nothing changes; the labels are compared with the kernel's

Per case: device time of the WHOLE call (three launches; the resident case includes sort and bounds) from torch events around it,
primed (2 calls), median and minimum of --events calls; pairs = frames n (n - 1) / 2.  `hist_ms_*` is the pair histogram
(pair_histogram_frames_device, or pair_histogram_device for the resident case) with r_max = r_cut and 16 bins on the same points,
`over_hist` the ratio of the medians.  Every row carries the number of clusters, the largest size and the bonds per point.

  python tools/bench_clusters.py [--out FILE.json] [--events 5] [--cases ...]
--out merges: rows of other cases already in the file are kept.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"trajectory": (1000, 1875, 40.0), "large": (1, 262144, 473.0), "density": (1, 65536, 236.5)}
CASES = ("trajectory", "large_batch", "large_resident", "density", "torch")
R_CUT, HIST_BINS = 1.5, 16


def points(n_frames, n, side, seed):
  g = torch.Generator(device="cuda")
  g.manual_seed(seed)
  x = torch.rand((n_frames, n, 3), dtype=torch.float64, device="cuda", generator=g) * side
  x[:, :, 2] = 0.0
  return x


def timed(call, prime, events):
  for _ in range(prime):
    call()
  ms = []
  for _ in range(events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
  return float(np.median(ms)), float(np.min(ms))


def describe(labels, sizes, hist):
  n = labels.numel()
  return dict(clusters=int(torch.count_nonzero(sizes)), largest=int(sizes.max()), bonds_per_point=2.0 * float(hist.sum()) / n)


def run_batch(name, shape, r_cut, args, ctx):
  F, n, side = SHAPES[shape]
  L = (side, side, 0.0)
  frames = points(F, n, side, seed=31)
  labels = torch.empty((F, n), dtype=torch.int32, device="cuda")
  sizes = torch.empty((F, n), dtype=torch.int32, device="cuda")
  hist = torch.zeros(HIST_BINS, dtype=torch.int64, device="cuda")
  med, low = timed(lambda: ctx.cluster_labels_frames_device(frames, L, r_cut, plane="xy", labels=labels, sizes=sizes), 2, args.events)
  h_med, h_low = timed(lambda: ctx.pair_histogram_frames_device(frames, L, r_cut, HIST_BINS, out=hist), 2, args.events)
  hist.zero_()
  ctx.pair_histogram_frames_device(frames, L, r_cut, HIST_BINS, out=hist)
  pairs = F * n * (n - 1) // 2
  row = dict(kind=name, entry="batch", frames=F, points=n, box=side, r_cut=r_cut, pairs=pairs, events=args.events, device_ms_median=med,
             device_ms_min=low, g_pairs_per_s=pairs / med * 1e-6, hist_ms_median=h_med, hist_ms_min=h_low, over_hist=med / h_med)
  row.update(describe(labels, sizes, hist))
  return row, frames, labels


def run_resident(args, ctx, batch_labels):
  F, n, side = SHAPES["large"]
  L = (side, side, 0.0)
  frames = points(F, n, side, seed=31)
  ctx.set_positions(frames[0].contiguous(), 0.5, periodic_length=L, wall=False)
  labels = torch.empty(n, dtype=torch.int32, device="cuda")
  sizes = torch.empty(n, dtype=torch.int32, device="cuda")
  hist = torch.zeros(HIST_BINS, dtype=torch.int64, device="cuda")
  med, low = timed(lambda: ctx.cluster_labels_device(R_CUT, plane="xy", labels=labels, sizes=sizes), 2, args.events)
  h_med, h_low = timed(lambda: ctx.pair_histogram_device(R_CUT, HIST_BINS, out=hist), 2, args.events)
  hist.zero_()
  ctx.pair_histogram_device(R_CUT, HIST_BINS, out=hist)
  pairs = n * (n - 1) // 2
  row = dict(kind="large_resident", entry="resident", frames=1, points=n, box=side, r_cut=R_CUT, pairs=pairs, events=args.events,
             device_ms_median=med, device_ms_min=low, hist_ms_median=h_med, hist_ms_min=h_low, over_hist=med / h_med)
  row.update(describe(labels, sizes, hist))
  if batch_labels is not None:
    row["labels_equal_batch_entry"] = bool(torch.equal(labels, batch_labels[0]))
  return row


def torch_labels(frame, side, r_cut):
  """min-label propagation over the dense adjacency (n, n) until a fixed point; -> (labels, rounds)"""
  d = frame[:, None, :2] - frame[None, :, :2]
  d = d - torch.trunc(d / side + 0.5 * torch.sign(d)) * side
  adj = (d * d).sum(dim=2) < r_cut * r_cut      # the diagonal is set: a point keeps its own label
  n = frame.shape[0]
  labels = torch.arange(n, device=frame.device)
  big = torch.full((n, n), n, dtype=torch.int64, device=frame.device)
  rounds = 0
  while True:
    new = torch.where(adj, labels[None, :].expand(n, n), big).min(dim=1).values
    rounds += 1
    if torch.equal(new, labels):
      return labels, rounds
    labels = new


def run_torch(args, ctx):
  F, n, side = SHAPES["trajectory"]
  frame = points(1, n, side, seed=31)[0].contiguous()
  L = (side, side, 0.0)
  labels, sizes = ctx.cluster_labels_frames_device(frame, L, R_CUT, plane="xy")
  med, low = timed(lambda: ctx.cluster_labels_frames_device(frame, L, R_CUT, plane="xy", labels=labels, sizes=sizes), 2, args.events)
  t_med, t_low = timed(lambda: torch_labels(frame, side, R_CUT), 1, args.events)
  ref, rounds = torch_labels(frame, side, R_CUT)
  return dict(kind="torch", frames=1, points=n, box=side, r_cut=R_CUT, events=args.events, device_ms_median=med, device_ms_min=low,
              torch_ms_median=t_med, torch_ms_min=t_low, torch_rounds=rounds, torch_over_hip=t_med / med,
              labels_differing_from_torch=int((labels.long() != ref).sum()), clusters=int(torch.count_nonzero(sizes)), largest=int(sizes.max()))


def main():
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("--out", default=None)
  ap.add_argument("--events", type=int, default=5)
  ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
  args = ap.parse_args()
  from rigidmultiblobswall_amd import MobilityContext
  ctx = MobilityContext(0)
  rows, large = [], None
  try:
    for case in args.cases:
      if case == "trajectory":
        rows.append(run_batch("trajectory", "trajectory", R_CUT, args, ctx)[0])
      elif case == "large_batch":
        row, _, large = run_batch("large_batch", "large", R_CUT, args, ctx)
        rows.append(row)
      elif case == "large_resident":
        rows.append(run_resident(args, ctx, large))
      elif case == "density":
        n, side = SHAPES["density"][1:]
        for name, per_point in (("density_dilute", 0.3), ("density_percolating", 12.0)):      # pi r^2 n / side^2 bonds per point
          rows.append(run_batch(name, "density", float(np.sqrt(per_point * side * side / (np.pi * n))), args, ctx)[0])
      else:
        rows.append(run_torch(args, ctx))
      print(json.dumps(rows[-1]), flush=True)
  finally:
    ctx.close()
  if args.out:
    kept = []
    if os.path.exists(args.out):
      with open(args.out) as f:
        kept = [r for r in json.load(f)["rows"] if not any(r["kind"].startswith(c) for c in args.cases)]
    with open(args.out, "w") as f:
      json.dump(dict(tool="tools/bench_clusters.py", device=torch.cuda.get_device_name(0), rows=kept + rows), f, indent=1)
      f.write("\n")


if __name__ == "__main__":
  main()
