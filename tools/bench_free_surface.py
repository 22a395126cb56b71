#!/usr/bin/env python
"""Small rigid decks, wall against free surface, one JSON line per run.

  python tools/bench_free_surface.py steps [--tree TREE]    the shell decks of bench.py's `small_deck_steps` stage (64 / 256
        twelve-blob shells above a WALL, whole time steps): the same decks, parameters and timing as that stage, so that two
        source trees can be compared in alternating processes on one device (--tree: import the package from another tree)
  python tools/bench_free_surface.py solve                  rmb_rigid_gmres_device at 64 and 256 shells: time per GMRES iteration
        above a wall and above a free surface (with unbounded and with free-surface preconditioner blocks)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shells(st, nb):
  R = 1.0155
  shell = st.icosahedron_shell(0.792079207921 * R)
  loc, quat, _ = st.roller_monolayer(nb, radius=R, seed=5)
  return shell, st.min_blob_separation(shell) / 2, loc, quat


def steps(torch, st, device):
  from rigidmultiblobswall_amd.rigid_integrator import RigidIntegrator
  rows = []
  for nb, scheme, tol, n_steps in ((64, "deterministic_adams_bashforth", 1e-8, 30), (64, "stochastic_Slip_Trapz", 1e-6, 10),
                                   (256, "deterministic_adams_bashforth", 1e-8, 30)):
    shell, a, loc, quat = shells(st, nb)
    best = None
    for rep in range(3):
      integ = RigidIntegrator([shell] * nb, loc, quat, scheme, a, 0.957e-3, tolerance=tol, device=device, seed=9)
      integ.kT, integ.g = 0.0041419464, 0.0024892 * 12
      integ.repulsion_strength_wall, integ.debye_length_wall = 0.0165677856, 0.0656
      integ.repulsion_strength, integ.debye_length = 0.0165677856, 0.0656
      for step in range(4):
        integ.advance_time_step(0.002, step=step)
      torch.cuda.synchronize(device)
      t0 = time.perf_counter()
      for step in range(4, 4 + n_steps):
        integ.advance_time_step(0.002, step=step)
      torch.cuda.synchronize(device)
      ms = 1e3 * (time.perf_counter() - t0) / n_steps
      best = ms if best is None else min(best, ms)
      integ.close()
    rows.append({"bodies": nb, "scheme": scheme, "ms_per_step": round(best, 3)})
  return rows


def solve(torch, st, device):
  from rigidmultiblobswall_amd.rigid import RigidSuspension
  rows = []
  for nb in (64, 256):
    shell, a, loc, quat = shells(st, nb)
    for boundary, blocks in (("single_wall", None), ("free_surface", "no_wall"), ("free_surface", "free_surface")):
      rs = RigidSuspension([shell] * nb, loc, quat, a, 0.957e-3, boundary=boundary, block_boundary=blocks, device=device)
      rs.build_preconditioner()
      rhs = torch.as_tensor(np.random.RandomState(1).randn(rs.size), device=device)
      for _ in range(3):
        x, info = rs.solve(rhs, tol=1e-8)
      torch.cuda.synchronize(device)
      assert info.get("native_gmres") and info["converged"]
      times = []
      for _ in range(20):
        t0 = time.perf_counter()
        x, info = rs.solve(rhs, tol=1e-8)
        torch.cuda.synchronize(device)
        times.append(time.perf_counter() - t0)
      rows.append({"bodies": nb, "boundary": boundary, "blocks": blocks or boundary, "iterations": info["iterations"],
                   "us_per_solve": round(1e6 * float(np.median(times)), 1),
                   "us_per_iteration": round(1e6 * float(np.median(times)) / info["iterations"], 2)})
      rs.close()
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("what", choices=("steps", "solve"))
  ap.add_argument("--tree", default=ROOT)
  args = ap.parse_args()
  tree = os.path.abspath(args.tree)
  sys.path.insert(0, tree)
  import torch
  from rigidmultiblobswall_amd import structures as st
  import rigidmultiblobswall_amd
  assert os.path.dirname(os.path.dirname(os.path.abspath(rigidmultiblobswall_amd.__file__))) == tree
  device = torch.device("cuda:0")
  rows = steps(torch, st, device) if args.what == "steps" else solve(torch, st, device)
  print(json.dumps({"what": args.what, "tree": os.path.relpath(tree, ROOT), "rows": rows}), flush=True)


if __name__ == "__main__":
  main()
