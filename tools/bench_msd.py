#!/usr/bin/env python
"""The mean-square displacement lag sweep (rmb_msd_frames_device) on one GPU, next to vectorised numpy on the host.

Sizes:
  single_body   1 body, 10^6 frames, 100 lags: the reference's own use (one tracked body, a long run)
  suspension    4096 bodies x 10 000 frames x 100 lags: a deck of a few thousand shells
Both with origins="window" and a tracking offset.  The trajectories are seeded random walks made on the device (steps of
0.05, orientation steps of 0.02 followed by normalisation).

Per size: device time of the WHOLE call (record pass + lag sweep + finishing launch) from torch events around it, primed (3
calls), median and minimum of --events calls; pairs = bodies x origins x lags and pairs/s; the executed-instruction
fraction of the fp64 issue rate: pairs x fp64 VALU instructions per lane-step of the sweep's inner loop (read off the gfx950
assembly of this tree, tools/kernel_resources.py) / 64 lanes, over the call time, against the rate of independent v_fma_f64
measured in the same process right after (rmb_ubench_fp64_issue); the same for all VALU instructions.  The host column:
the restatement of the tests (tests/_msd_numpy.py, rotation-matrix form, fp64, one vectorised pass per lag) on the same
frames -- all of them for single_body, the first --host-bodies bodies for suspension (the rate is per pair) -- with its
wall time and the largest difference of its sums from the kernel's on those bodies, relative to the largest entry.

  python tools/bench_msd.py [--out FILE.json] [--events 11] [--host-bodies 16] [--sizes single_body suspension]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _msd_numpy as mnp  # noqa: E402

SIZES = {"single_body": (1, 1000000, 100), "suspension": (4096, 10000, 100)}
OFFSET = (0.3, -0.2, 0.45)


def make_frames(n_bodies, n_frames, seed):
  g = torch.Generator(device="cuda")
  g.manual_seed(seed)
  frames = torch.empty((n_frames, n_bodies, 7), dtype=torch.float64, device="cuda")
  frames[..., :3] = 10.0 + torch.cumsum(0.05 * torch.randn((n_frames, n_bodies, 3), dtype=torch.float64, device="cuda", generator=g), dim=0)
  q = torch.cumsum(0.02 * torch.randn((n_frames, n_bodies, 4), dtype=torch.float64, device="cuda", generator=g), dim=0)
  q[..., 0] += 1.0
  frames[..., 3:] = q / torch.linalg.norm(q, dim=-1, keepdim=True)
  return frames


def loop_stats():
  """(VALU, fp64 VALU, LDS) instructions per lane-step of the sweep's unmasked inner loop, from the assembly of this tree"""
  import subprocess
  import isa_stats
  import kernel_resources as kr
  asm = subprocess.run([isa_stats.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-S", "--cuda-device-only", "-o", "-",
                        os.path.join(ROOT, "rigidmultiblobswall_amd", "csrc", "rmb_msd.hip")], check=True, capture_output=True, text=True).stdout
  m = next(m for m in kr.INFO.finditer(asm) if "msd_sweep_kernel" in m.group(1))
  loops = kr.pair_loops(asm, m.group(1))      # the unmasked loop and the masked one of the last origins
  assert len(loops) == 2, loops
  return min(loops, key=lambda l: l[1])[1:]


def run(name, events, host_bodies, stats, ctx):
  n_bodies, n_frames, n_lags = SIZES[name]
  frames = make_frames(n_bodies, n_frames, seed=20)
  offsets = torch.tensor(np.tile(OFFSET, (n_bodies, 1)), dtype=torch.float64, device="cuda")
  out = torch.zeros((n_lags, 6, 6), dtype=torch.float64, device="cuda")
  call = lambda: ctx.msd_frames_device(frames, n_lags, offsets=offsets, origins="window", out=out)   # noqa: E731
  for _ in range(3):
    call()
  ms = []
  for _ in range(events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _, counts = call()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
  issue = ctx.ubench_fp64_issue(40)      # G wave-instructions / s, clocks still primed
  pairs = int(counts.sum())
  med = float(np.median(ms))
  valu, f64, lds = stats
  row = dict(kind=name, bodies=n_bodies, frames=n_frames, lags=n_lags, origins="window", pairs=pairs, events=events, device_ms_median=med,
             device_ms_min=float(np.min(ms)), gpairs_per_s=pairs / med * 1e-6, fp64_issue_g_wave_instr_per_s=issue,
             loop_valu_per_step=valu, loop_fp64_valu_per_step=f64, loop_lds_per_step=lds,
             fp64_executed_fraction=pairs * f64 / 64.0 / (med * 1e-3) / (issue * 1e9),
             valu_executed_fraction=pairs * valu / 64.0 / (med * 1e-3) / (issue * 1e9))
  # the host: vectorised numpy on the same frames (a subset of the bodies when there are many)
  hb = min(n_bodies, host_bodies)
  sub = frames[:, :hb].contiguous()
  sums, sub_counts = ctx.msd_frames_device(sub, n_lags, offsets=offsets[:hb].contiguous(), origins="window")
  host_frames = sub.cpu().numpy()
  t0 = time.time()
  S, n = mnp.sums(host_frames, n_lags, offsets=np.tile(OFFSET, (hb, 1)), origins="window")
  host_s = time.time() - t0
  assert np.array_equal(n, sub_counts)
  row.update(host_bodies=hb, host_pairs=int(n.sum()), host_numpy_s=host_s, host_gpairs_per_s=int(n.sum()) / host_s * 1e-9,
             max_rel_difference_from_host=float(np.abs(sums.cpu().numpy() - S).max() / np.abs(S).max()))
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--events", type=int, default=11)
  ap.add_argument("--host-bodies", type=int, default=16)
  ap.add_argument("--sizes", nargs="*", default=list(SIZES))
  args = ap.parse_args()
  from rigidmultiblobswall_amd import MobilityContext
  stats = loop_stats()
  ctx = MobilityContext(0)
  rows = []
  try:
    for name in args.sizes:
      rows.append(run(name, args.events, args.host_bodies, stats, ctx))
      print(json.dumps(rows[-1]), flush=True)
  finally:
    ctx.close()
  res = dict(device=torch.cuda.get_device_name(0), rows=rows)
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(res, fh, indent=1)


if __name__ == "__main__":
  main()
