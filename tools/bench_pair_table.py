#!/usr/bin/env python
"""Time of the tabulated pair law's sweeps (csrc/pair_table_kernels.h: TableLaw of sym_force_kernel, the TABLE instances of
potential_kernel) next to the contact law / `soft` form on the SAME resident positions in the same process: all primed by
untimed calls, then alternating, HIP events around batches of calls, median over the repetitions.  4096 points and the
262 144-roller monolayer of configs[4] (area fraction 0.4, periodic in x and y), as tools/bench_body_force.py.

Tables: K = 1024 and K = 16 intervals of a force-shifted screened repulsion, with r_cut = 2a + 30 b (tile culling live: the
reach of the reference's tree_numba) and r_cut = the box side (every pair met).  The baselines are the contact law with
its own culling (reach 2a + 750 b) and with "force_cull" = 0 (every pair met).  No target ratio is set: the ratios are
reported.

  python tools/bench_pair_table.py [--out profiles/r27_pair_table.json] [--reps 5]
"""
import argparse
import json
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


def _table(K, r_cut):
  from rigidmultiblobswall_amd.pair_table import PairTable
  s = 30.0 / (r_cut - 2 * A)          # exp(-30) at r_cut on either reach: the same shape
  U = lambda r: EPS * np.exp(-(r - 2 * A) * s)      # noqa: E731
  dU = lambda r: -s * U(r)      # noqa: E731
  return PairTable.from_function(U, dU, A, r_cut, K, shift="force")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--sizes", default="4096,262144")
  args = ap.parse_args()
  from rigidmultiblobswall_amd.context import MobilityContext
  from rigidmultiblobswall_amd.structures import roller_monolayer
  result = {"what": "ms per call, median of %d batches; ratio = table / baseline (the baseline meets the pairs within baseline_reach)" % args.reps, "a": A, "eps": EPS, "b": B,
            "device": torch.cuda.get_device_name(0), "cases": []}
  for n in [int(x) for x in args.sizes.split(",")]:
    loc, _, side = roller_monolayer(n, radius=A, phi2d=0.4, seed=1)
    L = np.array([side, side, 0.0])
    r_dev = torch.as_tensor(loc, device="cuda:0").reshape(-1)
    out_f = torch.empty(3 * n, dtype=torch.float64, device="cuda:0")
    out_u = torch.empty(2, dtype=torch.float64, device="cuda:0")
    for reach_name, r_cut in (("culled", 2 * A + 30 * B), ("all", float(side))):
      ctx = MobilityContext(0)
      ctx.set_option("force_cull", 1 if reach_name == "culled" else 0)      # the baseline's reach; a table's own r_cut culls below
      ctx.set_positions(r_dev, A, L, wall=False)
      tables = {K: _table(K, r_cut) for K in (1024, 16)}
      calls = 100 if n <= 4096 else (10 if reach_name == "culled" else 1)
      ctx_t = {K: MobilityContext(0) for K in tables}          # one context per table: no re-upload between timed calls
      for K, c in ctx_t.items():
        c.set_positions(r_dev, A, L, wall=False)
        c.set_pair_table(tables[K])
      fns = {"force_contact": lambda: ctx.blob_blob_force_device(EPS, B, A, out=out_f),
             "energy_soft": lambda: ctx.blob_potential_device(EPS, B, A, out=out_u)}
      for K, c in ctx_t.items():
        fns["force_table_K%d" % K] = lambda c=c: c.pair_table_force_device(out=out_f)
        fns["energy_table_K%d" % K] = lambda c=c, K=K: c.blob_potential_device(0.0, 1.0, A, out=out_u, pair_table=tables[K])
      for fn in list(fns.values()) * 2:       # primed: code objects, the Morton sort of this configuration, clocks
        _batch_ms(fn, 1 if calls == 1 else 2)
      t = {k: [] for k in fns}
      for _ in range(args.reps):
        for k, fn in fns.items():
          t[k].append(_batch_ms(fn, calls))
      assert bool(torch.all(torch.isfinite(out_f))) and bool(torch.all(torch.isfinite(out_u)))
      med = {k: float(np.median(v)) for k, v in t.items()}
      case = {"n": n, "reach": reach_name, "r_cut": r_cut, "baseline_reach": 2 * A + 750 * B if reach_name == "culled" else float(side),
              "calls_per_batch": calls, "ms": med, "ms_min": {k: float(min(v)) for k, v in t.items()}, "ms_max": {k: float(max(v)) for k, v in t.items()},
              "ratio": {"force_K1024": med["force_table_K1024"] / med["force_contact"], "force_K16": med["force_table_K16"] / med["force_contact"],
                        "energy_K1024": med["energy_table_K1024"] / med["energy_soft"], "energy_K16": med["energy_table_K16"] / med["energy_soft"],
                        "force_K1024_over_K16": med["force_table_K1024"] / med["force_table_K16"],
                        "energy_K1024_over_K16": med["energy_table_K1024"] / med["energy_table_K16"]}}
      result["cases"].append(case)
      print(json.dumps(case), flush=True)
      ctx.close()
      for c in ctx_t.values():
        c.close()
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(result, fh, indent=1)
      fh.write("\n")


if __name__ == "__main__":
  main()
