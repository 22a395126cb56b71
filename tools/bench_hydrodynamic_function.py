#!/usr/bin/env python
"""The hydrodynamic-function sweep (rmb_hydro_function_frames_device) on one GPU, next to the only route the library had
before it: the same sums from the two-vector product, S_self + S_dist = v_c . (M v_c) + v_s . (M v_s) with v_c[i] = e cos(k . x_i),
v_s[i] = e sin(k . x_i) -- one matvec2_device pass over the pairs per wavevector and frame, plus two dot products.

Cases (seeded uniform points in a square box of density ~1.17, heights a ... 3 a above the wall, a = 0.3, eta = 1; 544 in-plane
wavevectors |n_d| <= 16, longitudinal polarisation, wall on):
  trajectory           1000 frames x 1875 points, box 40 x 40, open mobility         (the reference example's frame size)
  trajectory_periodic  the same frames, the mobility summed over the 3 x 3 images
  large                1 frame x 262 144 points, box 473 x 473, open mobility

Both routes run in one process, primed, their calls interleaved (sweep, baseline, sweep, ...); device time of a whole call from
torch events around it, median and minimum over --events calls.  The baseline's time per (frame, wavevector) does not depend
on which frame or wavevector it is, so it is MEASURED ON A SUBSET -- `baseline_frames` frames x `baseline_wavevectors`
wavevectors, stated in every row -- and `baseline_ms_scaled` is that time times (frames K) / (subset size).  The baseline
includes set_positions per frame and the construction of its vectors (one batched torch expression per frame).
`ratio` = baseline_ms_scaled / sweep_ms_median; `ns_per_pair_wavevector` = sweep time / (frames n (n - 1) / 2 x K);
`max_rel_difference` compares the two routes' sums on the subset.

  python tools/bench_hydrodynamic_function.py [--out FILE.json] [--events 3] [--cases ...]
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

# name -> (frames, points, box side, periodic mobility, baseline frames, baseline wavevectors)
CASES = {"trajectory": (1000, 1875, 40.0, False, 4, 544), "trajectory_periodic": (1000, 1875, 40.0, True, 2, 544),
         "large": (1, 262144, 473.0, False, 1, 4)}
A, ETA, N_MAX = 0.3, 1.0, 16


def points(n_frames, n, side, seed):
  g = torch.Generator(device="cuda")
  g.manual_seed(seed)
  x = torch.rand((n_frames, n, 3), dtype=torch.float64, device="cuda", generator=g)
  x[:, :, :2] *= side
  x[:, :, 2] = A + 2.0 * A * x[:, :, 2]
  return x


def event_ms(call):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  out = call()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1), out


def baseline(ctx, frames, L, mob_L, coef, pol, k_idx):
  """(len(frames), len(k_idx)) sums by the product route"""
  out = torch.empty((frames.shape[0], len(k_idx)), dtype=torch.float64, device="cuda")
  n = frames.shape[1]
  for f in range(frames.shape[0]):
    ctx.set_positions(frames[f], A, periodic_length=mob_L, wall=True)
    turns = frames[f] @ coef[k_idx].T                                      # (n, k)
    theta = 2.0 * np.pi * (turns - torch.round(turns))
    vc = (torch.cos(theta).T[:, :, None] * pol[k_idx][:, None, :]).reshape(len(k_idx), 3 * n).contiguous()
    vs = (torch.sin(theta).T[:, :, None] * pol[k_idx][:, None, :]).reshape(len(k_idx), 3 * n).contiguous()
    for j in range(len(k_idx)):
      uc, us = ctx.matvec2_device("tt", vc[j], vs[j], ETA)
      out[f, j] = torch.dot(vc[j], uc) + torch.dot(vs[j], us)
  return out


def run(name, args, ctx):
  from rigidmultiblobswall_amd import hydrofunction as hf
  from rigidmultiblobswall_amd.scattering import wavevectors
  F, n, side, periodic, bf, bk = CASES[name]
  L = (side, side, 0.0)
  mob_L = L if periodic else None
  wv = wavevectors(L, n_max=N_MAX, plane="xy")
  K = int(wv.shape[0])
  pol = hf.polarisations(L, wv, "longitudinal")
  frames = points(F, n, side, seed=32)
  out = torch.empty((F, K, 2), dtype=torch.float64, device="cuda")
  coef = torch.from_numpy(wv / side).cuda()
  pol_dev = torch.from_numpy(pol).cuda()
  k_idx = torch.linspace(0, K - 1, bk).round().long().cuda() if bk < K else torch.arange(K, device="cuda")
  sub = frames[:bf].contiguous()

  def sweep():
    return ctx.hydrodynamic_function_frames_device(frames, A, ETA, L, wv, pol, wall=True, mobility_periodic_length=mob_L, out=out)

  def base():
    return baseline(ctx, sub, L, mob_L, coef, pol_dev, k_idx)
  sweep(); base()      # primed
  s_ms, b_ms = [], []
  for _ in range(args.events):
    s_ms.append(event_ms(sweep)[0])
    ms, ref = event_ms(base)
    b_ms.append(ms)
  got = out[:bf].sum(dim=2)[:, k_idx]
  scale = (F * K) / float(bf * len(k_idx))
  pairs = F * n * (n - 1) // 2
  s_med, b_med = float(np.median(s_ms)), float(np.median(b_ms))
  H = (out.sum(dim=2).mean(dim=0) * (6.0 * np.pi * ETA * A / n)).cpu().numpy()
  return dict(kind=name, frames=F, points=n, box=side, wavevectors=K, wall=True, periodic_mobility=periodic, radius=A, eta=ETA, pairs=pairs,
              events=args.events, sweep_ms_median=s_med, sweep_ms_min=float(np.min(s_ms)), baseline_frames=bf, baseline_wavevectors=int(len(k_idx)),
              baseline_ms_subset_median=b_med, baseline_ms_subset_min=float(np.min(b_ms)), baseline_ms_scaled=b_med * scale,
              ratio=b_med * scale / s_med, ns_per_pair_wavevector=s_med * 1e6 / (float(pairs) * K),
              max_rel_difference=float(((got - ref).abs() / ref.abs()).max()), H_min=float(H.min()), H_max=float(H.max()))


def main():
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("--out", default=None)
  ap.add_argument("--events", type=int, default=3)
  ap.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
  args = ap.parse_args()
  from rigidmultiblobswall_amd import MobilityContext
  ctx = MobilityContext(0)
  rows = []
  try:
    for case in args.cases:
      rows.append(run(case, args, ctx))
      print(json.dumps(rows[-1]), flush=True)
  finally:
    ctx.close()
  if args.out:
    kept = []
    if os.path.exists(args.out):
      with open(args.out) as f:
        kept = [r for r in json.load(f)["rows"] if r["kind"] not in args.cases]
    with open(args.out, "w") as f:
      json.dump(dict(tool="tools/bench_hydrodynamic_function.py", device=torch.cuda.get_device_name(0), rows=kept + rows), f, indent=1)
      f.write("\n")


if __name__ == "__main__":
  main()
