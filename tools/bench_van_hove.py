#!/usr/bin/env python
"""The van Hove sweeps (rmb_van_hove_distinct_frames_device, rmb_van_hove_self_frames_device) on one GPU, next to the batch pair
histogram on the same frames and to the same counts evaluated with torch on the same device.

Cases (seeded random walks made on the device, steps of 0.05 per frame and coordinate, a layer of thickness 1):
  distinct_trajectory   1000 frames x 1875 points x 50 lags, box 40 x 40, 1000 bins to 20     (the reference example's frame size)
  distinct_large        100 frames x 16 384 points x 10 lags, box 120 x 120, 1000 bins to 20
  self_trajectory       4096 points x 10 000 frames x 100 lags, 1000 bins to 2
  self_large            262 144 points x 100 frames x 20 lags, 1000 bins to 2
All with origins="window", plane="xyz".

Per case: device time of the WHOLE call from torch events around it, primed (2 calls), median and minimum of --events calls;
terms = (origin, lag, ordered pair) or (origin, lag, point), and terms per second.  Yardsticks, never the code under test itself:
  pair_hist  rmb_pair_histogram_frames_device on the same frames (lag 0, unordered pairs: frames n (n - 1) / 2 terms), same bins,
             primed, median of --events; both sweeps do the same work per term
  torch      the same counts on the same device: per (origin, lag) the separations by broadcasting, the minimal image, norm,
             bincount -- on --torch-origins origins for the distinct part (its rate is per term), on everything for the self part
             (per lag one difference of two slices).  Primed once, median of --torch-events.
Each row also carries the number of counts by which the kernel's histogram differs from torch's on the compared part (terms
within a rounding error of a bin edge may differ; the tests demand equality under a margin, this does not).

  python tools/bench_van_hove.py [--out FILE.json] [--events 5] [--torch-events 3] [--cases ...]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"distinct_trajectory": (1000, 1875, 50, 40.0, 20.0), "distinct_large": (100, 16384, 10, 120.0, 20.0),
         "self_trajectory": (10000, 4096, 100, 40.0, 2.0), "self_large": (100, 262144, 20, 480.0, 2.0)}
N_BINS = 1000
TORCH_PAIRS = 1 << 24      # separations per broadcast


def walk(n_frames, n_points, side, seed, step=0.05):
  g = torch.Generator(device="cuda")
  g.manual_seed(seed)
  x0 = torch.rand((1, n_points, 3), dtype=torch.float64, device="cuda", generator=g) * torch.tensor([side, side, 1.0], dtype=torch.float64, device="cuda")
  frames = torch.empty((n_frames, n_points, 3), dtype=torch.float64, device="cuda")
  per = max(1, (1 << 25) // n_points)
  for f0 in range(0, n_frames, per):      # in pieces: the normal deviates of the whole trajectory need not exist at once
    f1 = min(f0 + per, n_frames)
    frames[f0:f1] = x0 + torch.cumsum(step * torch.randn((f1 - f0, n_points, 3), dtype=torch.float64, device="cuda", generator=g), dim=0)
    x0 = frames[f1 - 1:f1].clone()
  return frames


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


def _bincount(r, r_max, n_bins):
  r = r[r < r_max]
  return torch.bincount(torch.clamp((r * (n_bins / r_max)).long(), max=n_bins - 1), minlength=n_bins)


def torch_distinct(frames, L, n_lags, n_origins, r_max, n_bins):
  n = frames.shape[1]
  out = torch.zeros((n_lags, n_bins), dtype=torch.int64, device="cuda")
  rows = max(1, TORCH_PAIRS // n)
  Lt = torch.tensor(L, dtype=torch.float64, device="cuda")
  per = Lt > 0
  for lag in range(n_lags):
    for o in range(n_origins):
      for i0 in range(0, n, rows):
        d = frames[o + lag, i0:i0 + rows, None, :] - frames[o, None, :, :]
        w = d - torch.trunc(d / torch.where(per, Lt, torch.ones_like(Lt)) + 0.5 * torch.sign(d)) * Lt
        r = torch.where(per, w, d).square().sum(dim=2).sqrt()
        idx = torch.arange(i0, min(i0 + rows, n), device="cuda")
        r[idx - i0, idx] = float("inf")      # i = j
        out[lag] += _bincount(r.reshape(-1), r_max, n_bins)
  return out


def torch_self(frames, n_lags, r_max, n_bins):
  n_o = frames.shape[0] - n_lags + 1
  out = torch.zeros((n_lags, n_bins), dtype=torch.int64, device="cuda")
  per = max(1, TORCH_PAIRS // frames.shape[1])
  for lag in range(n_lags):
    for o0 in range(0, n_o, per):
      o1 = min(o0 + per, n_o)
      r = (frames[o0 + lag:o1 + lag] - frames[o0:o1]).square().sum(dim=2).sqrt()
      out[lag] += _bincount(r.reshape(-1), r_max, n_bins)
  return out


def run(name, args, ctx):
  F, N, n_lags, side, r_max = CASES[name]
  L = (side, side, 0.0)
  frames = walk(F, N, side, seed=29)
  n_o = F - n_lags + 1
  row = dict(kind=name, frames=F, points=N, lags=n_lags, origins=n_o, n_bins=N_BINS, r_max=r_max, events=args.events, torch_events=args.torch_events)
  out = torch.zeros((n_lags, N_BINS), dtype=torch.int64, device="cuda")
  if name.startswith("distinct"):
    terms = n_o * n_lags * N * (N - 1)
    med, low = timed(lambda: ctx.van_hove_distinct_frames_device(frames, L, n_lags, r_max, N_BINS, origins="window", out=out), 2, args.events)
    k = min(n_o, args.torch_origins)
    t_med, _ = timed(lambda: torch_distinct(frames, L, n_lags, k, r_max, N_BINS), 1, args.torch_events)
    t_terms = k * n_lags * N * (N - 1)
    once = ctx.van_hove_distinct_frames_device(frames, L, n_lags, r_max, N_BINS, o_begin=0, o_end=k)
    diff = int((once - torch_distinct(frames, L, n_lags, k, r_max, N_BINS)).abs().sum())
    counted = int(once.sum())
    row.update(work="(origin, lag, ordered pair) terms", torch_origins=k)
  else:
    terms = n_o * n_lags * N
    mom = torch.zeros((n_lags, 2), dtype=torch.float64, device="cuda")
    med, low = timed(lambda: ctx.van_hove_self_frames_device(frames, n_lags, r_max, N_BINS, origins="window", out=out, moments=mom), 2, args.events)
    t_med, _ = timed(lambda: torch_self(frames, n_lags, r_max, N_BINS), 1, args.torch_events)
    t_terms = terms
    once, _ = ctx.van_hove_self_frames_device(frames, n_lags, r_max, N_BINS, origins="window")
    diff = int((once - torch_self(frames, n_lags, r_max, N_BINS)).abs().sum())
    counted = int(once.sum())
    row.update(work="(origin, lag, point) terms")
  # the batch pair histogram on the same frames, as many of them as make about 1e11 pairs
  hist = torch.zeros(N_BINS, dtype=torch.int64, device="cuda")
  hf = frames[:max(1, min(F, int(2.0e11 / (float(N) * N))))]
  p_med, _ = timed(lambda: ctx.pair_histogram_frames_device(hf, L, 20.0, N_BINS, out=hist), 2, args.events)
  p_terms = hf.shape[0] * N * (N - 1) // 2
  row.update(terms=terms, device_ms_median=med, device_ms_min=low, g_terms_per_s=terms / med * 1e-6, counted_terms_compared=counted,
             counts_differing_from_torch=diff, torch_terms=t_terms, torch_ms_median=t_med, torch_g_terms_per_s=t_terms / t_med * 1e-6,
             torch_over_hip=(t_med / t_terms) / (med / terms), pair_hist_frames=int(hf.shape[0]), pair_hist_terms=p_terms,
             pair_hist_ms_median=p_med, pair_hist_g_terms_per_s=p_terms / p_med * 1e-6)
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--events", type=int, default=5)
  ap.add_argument("--torch-events", type=int, default=3)
  ap.add_argument("--torch-origins", type=int, default=2)
  ap.add_argument("--cases", nargs="*", default=list(CASES))
  args = ap.parse_args()
  from rigidmultiblobswall_amd import MobilityContext
  ctx = MobilityContext(0)
  rows = []
  try:
    for name in args.cases:
      rows.append(run(name, args, ctx))
      print(json.dumps(rows[-1]), flush=True)
      torch.cuda.empty_cache()
  finally:
    ctx.close()
  res = dict(device=torch.cuda.get_device_name(0), rows=rows)
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(res, fh, indent=1)


if __name__ == "__main__":
  main()
