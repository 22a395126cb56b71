#!/usr/bin/env python
"""Timings of the Laplace layer sweeps of phoretic bodies (csrc/laplace_kernels.h) and of one deterministic step of a
phoretic suspension, HIP events around the device work.

  * the fused operator sweep (alpha c - D[p] + S[q], one per GMRES iteration of the concentration solve) and the fused
    gradient sweep (2 G[p] - 2 P[q]), with and without the wall, at 1e4, 4.2e4 and 1e5 nodes;
  * one deterministic_forward_euler step of 1000 Janus shells of 42 nodes above the wall (42 000 nodes): whole step,
    the phoretic slip inside it (RHS + GMRES + gradient), its share, the Laplace and rigid GMRES iterations.

  python tools/bench_laplace.py [--out FILE.json] [--reps 5]
  RMB_AB_LIB=<other build of librmb_mobility.so>   time that build instead (same-box A/B of two builds, as bench_ops.py)
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
from rigidmultiblobswall_amd import _lib as _rmb_lib
if os.environ.get("RMB_AB_LIB"):
  _rmb_lib.LIB_PATH = os.path.abspath(os.environ["RMB_AB_LIB"])


def _cloud(n, seed):
  rng = np.random.RandomState(seed)
  L = (n / 0.05) ** (1.0 / 3.0)
  r = np.column_stack([L * rng.rand(n), L * rng.rand(n), 0.5 + 0.3 * L * rng.rand(n)])
  nrm = rng.randn(n, 3)
  nrm /= np.linalg.norm(nrm, axis=1)[:, None]
  t = lambda a: torch.as_tensor(np.ascontiguousarray(a).reshape(-1), device="cuda:0")  # noqa: E731
  return t(r), t(nrm), t(rng.randn(n)), t(0.2 + rng.rand(n)), t(rng.randn(n))


def _time(fn, reps):
  fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
  return float(np.median(ms)), float(np.min(ms))


def sweeps(reps):
  from rigidmultiblobswall_amd.context import MobilityContext
  ctx = MobilityContext(0)
  rows = []
  for n in (10000, 42000, 100000):
    r, nrm, p, w, q = _cloud(n, 1)
    out1 = torch.empty(n, dtype=torch.float64, device="cuda:0")
    out3 = torch.empty(3 * n, dtype=torch.float64, device="cuda:0")
    for wall in (False, True):
      op = _time(lambda: ctx.laplace_operator_device(r, w, p=p, q=q, normals=nrm, alpha=0.5, wall=wall, out=out1), reps)
      gr = _time(lambda: ctx.laplace_gradient_device(r, w, p=p, q=q, normals=nrm, wall=wall, out=out3), reps)
      row = dict(n=n, wall=wall, operator_ms=op[0], operator_min_ms=op[1], gradient_ms=gr[0], gradient_min_ms=gr[1],
                 operator_pairs_per_ns=n * n / (op[0] * 1e6), gradient_pairs_per_ns=n * n / (gr[0] * 1e6))
      print(json.dumps(row), flush=True)
      rows.append(row)
  ctx.close()
  return rows


def janus_step(nb=1000):
  from rigidmultiblobswall_amd.rigid_integrator import RigidIntegrator
  from rigidmultiblobswall_amd.laplace import PhoreticSlip
  g = np.load(os.path.join(ROOT, "tests", "golden", "g12_laplace_slip_janus_wall.npz"))
  shell, lap = g["vertex"], g["laplace"]
  m = int(np.ceil(np.sqrt(nb)))
  rng = np.random.RandomState(2)
  loc = np.array([[3.0 * (k % m), 3.0 * (k // m), 1.5 + 0.5 * rng.rand()] for k in range(nb)])
  q = rng.randn(nb, 4)
  q /= np.linalg.norm(q, axis=1)[:, None]
  integ = RigidIntegrator([shell] * nb, loc, q, "deterministic_forward_euler", float(g["blob_radius"]), 1.0, tolerance=1e-8,
                          device="cuda:0")
  integ.g = 0.3
  ps = PhoreticSlip(integ.susp, np.tile(lap, (nb, 1)), background=g["background"], diffusion_coefficient=0.7, tolerance=1e-8)
  slip_ms = []

  def timed_slip(it):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = ps(it)
    torch.cuda.synchronize()
    slip_ms.append(1e3 * (time.perf_counter() - t0))
    return s
  integ.calc_slip = timed_slip
  integ.advance_time_step(0.01, step=0)          # warm-up (preconditioner build, first launches)
  torch.cuda.synchronize()
  slip_ms.clear()
  its0, det0 = ps.iterations, integ.det_iterations_count
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  integ.advance_time_step(0.01, step=1)
  e1.record()
  e1.synchronize()
  step_ms = e0.elapsed_time(e1)
  row = dict(bodies=nb, nodes=integ.Nblobs, step_ms=step_ms, laplace_ms=float(sum(slip_ms)),
             laplace_share=float(sum(slip_ms)) / step_ms, laplace_gmres_iterations=ps.iterations - its0,
             rigid_gmres_iterations=integ.det_iterations_count - det0)
  print(json.dumps(row), flush=True)
  ps.close()
  integ.close()
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--reps", type=int, default=5)
  args = ap.parse_args()
  res = dict(device=torch.cuda.get_device_name(0), sweeps=sweeps(args.reps), janus_step=janus_step())
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(res, fh, indent=1)


if __name__ == "__main__":
  main()
