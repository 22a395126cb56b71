#!/usr/bin/env python
"""The scattering sweeps (rmb_density_modes_frames_device, rmb_scattering_lags_device, rmb_self_scattering_frames_device) on one
GPU, next to the same sums evaluated with torch on the same device and with vectorised numpy on the host.

Cases, all with wavevectors(n_max=16, plane="xy") of a 40 x 40 box unless said otherwise:
  modes_trajectory   1000 frames x 1875 points: density modes
  modes_one_frame    one frame of 262 144 points: density modes (point ranges + finishing launch)
  collective_lags    10 000 frames x 100 lags over the modes of those wavevectors
  self_lags          4096 points x 10 000 frames x 100 lags x 8 wavevectors
Lag sums with origins="window".  The trajectories are seeded random walks made on the device.

Per case: device time of the WHOLE call from torch events around it, primed (3 calls), median and minimum of --events calls;
work = phase evaluations (modes), or (origin, lag, wavevector[, point]) products (lag sums), and work per second.
Yardsticks, never the code under test itself:
  torch   the same sums in chunks on the same device, same run: phases as tensors (frames @ (n / L)^T, minus its rounding,
          times 2 pi), cos / sin / sum; per lag a product of two slices and a sum.  Primed once, median of --torch-events.
  numpy   the restatement of the tests (tests/_scattering_numpy.py, fp64) on a subset (--host-frames frames for the modes,
          --host-points points for the self part, --host-k wavevectors for the collective sums); its rate is per unit of work.
Each row also carries the largest difference of the kernel's result from the torch one, relative to the largest entry.

  python tools/bench_scattering.py [--out FILE.json] [--events 11] [--torch-events 3] [--cases ...]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _scattering_numpy as snp  # noqa: E402
from rigidmultiblobswall_amd import scattering  # noqa: E402

BOX = (40.0, 40.0, 0.0)
CASES = ("modes_trajectory", "modes_one_frame", "collective_lags", "self_lags")
TORCH_CHUNK_BYTES = 256 << 20


def walk(n_frames, n_points, seed, step=0.05):
  g = torch.Generator(device="cuda")
  g.manual_seed(seed)
  x0 = torch.rand((1, n_points, 3), dtype=torch.float64, device="cuda", generator=g) * torch.tensor([BOX[0], BOX[1], 1.0], dtype=torch.float64, device="cuda")
  frames = torch.empty((n_frames, n_points, 3), dtype=torch.float64, device="cuda")
  for f0 in range(0, n_frames, 1000):      # in pieces: the normal deviates of 4096 x 10 000 x 3 need not exist at once
    f1 = min(f0 + 1000, n_frames)
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


def torch_phases(x, coef):
  """(cos, -sin) of the phases of points x (..., 3) for coef (K, 3) = n / L: tensors of shape (..., K)"""
  t = x @ coef.T
  theta = (2.0 * np.pi) * (t - torch.round(t))
  return torch.cos(theta), -torch.sin(theta)


def torch_modes(frames, coef):
  F, N, K = frames.shape[0], frames.shape[1], coef.shape[0]
  out = torch.zeros((F, K, 2), dtype=torch.float64, device="cuda")
  per_frame = N * K * 8
  if per_frame <= TORCH_CHUNK_BYTES:
    step = max(1, TORCH_CHUNK_BYTES // per_frame)
    for f0 in range(0, F, step):
      re, im = torch_phases(frames[f0:f0 + step], coef)
      out[f0:f0 + step, :, 0], out[f0:f0 + step, :, 1] = re.sum(dim=1), im.sum(dim=1)
  else:
    step = max(1, TORCH_CHUNK_BYTES // (K * 8))
    for f in range(F):
      for j0 in range(0, N, step):
        re, im = torch_phases(frames[f, j0:j0 + step], coef)
        out[f, :, 0] += re.sum(dim=0)
        out[f, :, 1] += im.sum(dim=0)
  return out


def torch_collective(modes, n_lags):
  n_o = modes.shape[0] - n_lags + 1
  out = torch.empty((n_lags, modes.shape[1]), dtype=torch.float64, device="cuda")
  for lag in range(n_lags):
    out[lag] = (modes[:n_o] * modes[lag:lag + n_o]).sum(dim=(0, 2))
  return out


def torch_self(frames, coef, n_lags):
  re, im = torch_phases(frames, coef)      # (F, N, K) each
  n_o = frames.shape[0] - n_lags + 1
  out = torch.empty((n_lags, coef.shape[0]), dtype=torch.float64, device="cuda")
  for lag in range(n_lags):
    out[lag] = (re[:n_o] * re[lag:lag + n_o] + im[:n_o] * im[lag:lag + n_o]).sum(dim=(0, 1))
  return out


def rel_diff(a, b):
  return float((a - b).abs().max() / b.abs().max())


def run(name, args, ctx):
  wv = scattering.wavevectors(BOX, n_max=16, plane="xy")
  coef = torch.tensor(snp.coefficients(BOX, wv), dtype=torch.float64, device="cuda")
  row = dict(kind=name, events=args.events, torch_events=args.torch_events)
  if name in ("modes_trajectory", "modes_one_frame"):
    F, N = (1000, 1875) if name == "modes_trajectory" else (1, 262144)
    frames = walk(F, N, seed=23)
    out = torch.empty((F, len(wv), 2), dtype=torch.float64, device="cuda")
    med, low = timed(lambda: ctx.density_modes_frames_device(frames, BOX, wv, out=out), 3, args.events)
    t_med, _ = timed(lambda: torch_modes(frames, coef), 1, args.torch_events)
    work = F * N * len(wv)
    hf = min(F, args.host_frames)
    host = frames[:hf, :min(N, 16384)].cpu().numpy()
    t0 = time.time()
    snp.modes(host, BOX, wv)
    host_s, host_work = time.time() - t0, host.shape[0] * host.shape[1] * len(wv)
    row.update(frames=F, points=N, wavevectors=len(wv), work="phase evaluations", difference_from_torch=rel_diff(out, torch_modes(frames, coef)))
  elif name == "collective_lags":
    F, n_lags = 10000, 100
    g = torch.Generator(device="cuda")
    g.manual_seed(24)
    modes = torch.randn((F, len(wv), 2), dtype=torch.float64, device="cuda", generator=g) * 30.0
    out = torch.zeros((n_lags, len(wv)), dtype=torch.float64, device="cuda")
    med, low = timed(lambda: ctx.scattering_lags_device(modes, n_lags, origins="window", out=out), 3, args.events)
    t_med, _ = timed(lambda: torch_collective(modes, n_lags), 1, args.torch_events)
    work = (F - n_lags + 1) * n_lags * len(wv)
    once, _ = ctx.scattering_lags_device(modes, n_lags, origins="window")
    hk = min(len(wv), args.host_k)
    host = modes[:, :hk].cpu().numpy()
    t0 = time.time()
    snp.collective(host, n_lags, origins="window")
    host_s, host_work = time.time() - t0, (F - n_lags + 1) * n_lags * hk
    row.update(frames=F, lags=n_lags, wavevectors=len(wv), work="(origin, lag, wavevector) products",
               difference_from_torch=rel_diff(once, torch_collective(modes, n_lags)))
  else:
    F, N, n_lags, wv = 10000, 4096, 100, wv[:8]
    coef = coef[:8]
    frames = walk(F, N, seed=25)
    out = torch.zeros((n_lags, 8), dtype=torch.float64, device="cuda")
    med, low = timed(lambda: ctx.self_scattering_frames_device(frames, BOX, wv, n_lags, origins="window", out=out), 3, args.events)
    t_med, _ = timed(lambda: torch_self(frames, coef, n_lags), 1, args.torch_events)
    work = (F - n_lags + 1) * n_lags * 8 * N
    once, _ = ctx.self_scattering_frames_device(frames, BOX, wv, n_lags, origins="window")
    hp = min(N, args.host_points)
    host = frames[:, :hp].cpu().numpy()
    t0 = time.time()
    snp.self_sums(host, BOX, wv, n_lags, origins="window")
    host_s, host_work = time.time() - t0, (F - n_lags + 1) * n_lags * 8 * hp
    row.update(frames=F, points=N, lags=n_lags, wavevectors=8, work="(origin, lag, wavevector, point) products",
               phase_evaluations=F * N * 8, difference_from_torch=rel_diff(once, torch_self(frames, coef, n_lags)))
  row.update(work_items=work, device_ms_median=med, device_ms_min=low, g_items_per_s=work / med * 1e-6, torch_ms_median=t_med,
             torch_over_hip=t_med / med, host_work_items=host_work, host_numpy_s=host_s, host_g_items_per_s=host_work / host_s * 1e-9,
             host_threads=torch.get_num_threads(), numpy_over_hip=(host_s / host_work) / (med * 1e-3 / work))
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--events", type=int, default=11)
  ap.add_argument("--torch-events", type=int, default=3)
  ap.add_argument("--host-frames", type=int, default=4)
  ap.add_argument("--host-points", type=int, default=16)
  ap.add_argument("--host-k", type=int, default=16)
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
