#!/usr/bin/env python
"""Time per product of the rotational free-surface operations (grand mobility, fused row u = M_tt f + M_tr tau, M_rr)
next to their unbounded twins, which evaluate RPY(d) alone where the free surface evaluates RPY(d) and RPY(R): the
expectation is about twice the unbounded sweep.

One process, kernel times from the context's own events ("timing" = 1: sweep + finalize of every product), clocks primed
by warm-up products, free-surface and unbounded products interleaved round by round, median over the rounds.

  python tools/bench_free_surface_rotation.py [--n 10000 100000] [--rounds 12] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rigidmultiblobswall_amd import MobilityContext      # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--n", type=int, nargs="+", default=[10000, 100000])
  ap.add_argument("--rounds", type=int, default=12)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("no GPU: these are device timings, nothing is measured without one")
  eta, a = 1.0, 0.3
  lines = ["# n  operation  free_surface_ms  unbounded_per_wave_ms  ratio   (median of %d interleaved rounds; spread = (max - min) / median)" % args.rounds]
  for n in args.n:
    rng = np.random.RandomState(n)
    side = 2.2 * a * n ** (1.0 / 3.0)
    r = np.column_stack([side * rng.rand(n), side * rng.rand(n), 0.05 * a + side * rng.rand(n)])
    rd = torch.as_tensor(r.reshape(-1), device="cuda")
    f, t = (torch.as_tensor(rng.randn(3 * n), device="cuda") for _ in range(2))
    ctxs = {}
    # "open": the per-wave kernel, the one variant the free-surface operations have; "open_default": whatever variant
    # the unbounded product picks by itself (cooperative / two targets per lane)
    for name, wall in (("free", "free_surface"), ("open", False), ("open_default", False)):
      c = MobilityContext(0)
      c.set_option("timing", 1)
      c.set_option("free_surface_rotation", 1)
      if name == "open":
        c.set_option("sym_coop", 0)
        c.set_option("sym_two_targets", 0)
        c.set_option("symx_single", 1)       # rr through the generic skeleton, as the free-surface rr
      c.set_positions(rd, a, None, wall=wall)
      ctxs[name] = c
    ops = {"grand": lambda c: c.matvec_op_device("grand", (f, t), eta),
           "fused_row": lambda c: c.matvec_op_device("velocity_from_force_torque", (f, t), eta),
           "rr": lambda c: c.matvec_device("rr", t, eta)}
    for op, run in ops.items():
      for c in ctxs.values():        # warm-up: code objects, clocks, plans
        for _ in range(3):
          run(c)
      torch.cuda.synchronize()
      ms = {k: [] for k in ctxs}
      for _ in range(args.rounds):
        for name, c in ctxs.items():
          c.timing_reset()
          run(c)
          ms[name].append(float(np.sum(c.timing_collect(64))))
      med = {k: float(np.median(v)) for k, v in ms.items()}
      spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
      lines.append("%7d  %-10s %10.4f  %10.4f  %6.2f   (spread %.1f %% / %.1f %%; unbounded product as served by default %.4f ms)" %
                   (n, op, med["free"], med["open"], med["free"] / med["open"], 100 * spread["free"], 100 * spread["open"], med["open_default"]))
      print(lines[-1], flush=True)
    for c in ctxs.values():
      c.close()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
