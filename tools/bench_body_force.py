#!/usr/bin/env python
"""Time of the body-body force sweep (csrc/sym_force_kernels.h, BodyYukawaLaw) next to rmb_blob_blob_force_device on the
SAME resident positions in the same process: both primed by untimed calls, then alternating, HIP events around batches of
calls, median over the repetitions.  4096 centres and the 262 144-roller monolayer of configs[4] (area fraction 0.4,
periodic in x and y), the deck's repulsion parameters for both laws.

  python tools/bench_body_force.py [--out FILE.txt] [--reps 9]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A, EPS, B = 0.656, 0.0165677856, 0.0656      # roller radius, repulsion strength, Debye length 0.1 a


def _batch_ms(fn, calls):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(calls):
    fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--reps", type=int, default=9)
  args = ap.parse_args()
  from rigidmultiblobswall_amd.context import MobilityContext
  from rigidmultiblobswall_amd.structures import roller_monolayer
  ctx = MobilityContext(0)
  lines = ["body-body force sweep next to the blob-blob force sweep, same resident positions, ms per call (median of %d batches, "
           "min .. max)" % args.reps]
  for n in (4096, 262144):
    loc, _, side = roller_monolayer(n, radius=A, phi2d=0.4, seed=1)
    ctx.set_positions(torch.as_tensor(loc, device="cuda:0").reshape(-1), A, np.array([side, side, 0.0]), wall=False)
    out_blob = torch.empty(3 * n, dtype=torch.float64, device="cuda:0")
    out_body = torch.empty(3 * n, dtype=torch.float64, device="cuda:0")
    blob = lambda: ctx.blob_blob_force_device(EPS, B, A, out=out_blob)      # noqa: E731
    body = lambda: ctx.body_body_force_device(EPS, B, out=out_body)         # noqa: E731
    calls = 200 if n <= 4096 else 20
    for fn in (blob, body, blob, body):       # primed: code objects, the Morton sort of this configuration, clocks
      _batch_ms(fn, calls)
    t = {"blob": [], "body": []}
    for _ in range(args.reps):
      t["blob"].append(_batch_ms(blob, calls))
      t["body"].append(_batch_ms(body, calls))
    assert bool(torch.all(torch.isfinite(out_body))) and bool(torch.all(torch.isfinite(out_blob)))
    mb, my = np.median(t["blob"]), np.median(t["body"])
    lines.append("n = %6d  blob_blob_force_device %.4f (%.4f .. %.4f)   body_body_force_device %.4f (%.4f .. %.4f)   body / blob = %.2f"
                 % (n, mb, min(t["blob"]), max(t["blob"]), my, min(t["body"]), max(t["body"]), my / mb))
  ctx.close()
  text = "\n".join(lines) + "\n"
  print(text, end="")
  if args.out:
    with open(args.out, "w") as fh:
      fh.write(text)


if __name__ == "__main__":
  main()
