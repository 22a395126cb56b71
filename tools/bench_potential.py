#!/usr/bin/env python
"""Timings of the potential-energy sweep (csrc/potential_kernels.h) and of one Metropolis step, HIP events around the
device work (clocks primed by an untimed call first, as tools/bench_laplace.py).

  * the energy sweep at 1e4, 1e5 and 262 144 blobs on three layouts -- the roller monolayer of configs[4] (area fraction
    0.4), a random dilute cloud, the monolayer with culling off -- next to rmb_blob_blob_force_device on the SAME resident
    configuration in the same process, the two alternating;
  * the Morton permutation rebuilt on every evaluation against reused for 4 / 16 / 64 ("potential_resort"):
    set_positions + energy along a random walk of 0.1 a per evaluation, averaged over 64 evaluations;
  * the sweep with and without its one-blob terms;
  * one MCMC step of 1000 and of 21 845 twelve-blob shells, split into draws (host), upload, proposal launch, energy
    sweep + read-back, for rng = reference and batched.

  python tools/bench_potential.py [--out FILE.json] [--reps 7] [--skip-mcmc]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A, EPS, B = 0.656, 0.03, 0.0656      # roller radius, repulsion strength, Debye length 0.1 a
WALL = dict(repulsion_strength_wall=0.03, debye_length_wall=0.0656, weight=0.0124)


def _event_ms(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def _layout(kind, n):
  from rigidmultiblobswall_amd.structures import roller_monolayer
  if kind == "cloud":
    rng = np.random.RandomState(7)
    side = (n * 4.0 / 3.0 * np.pi * A ** 3 / 0.02) ** (1.0 / 3.0)        # volume fraction 0.02
    return np.column_stack([side * rng.rand(n), side * rng.rand(n), A + side * rng.rand(n)]), np.zeros(3)
  loc, _, side = roller_monolayer(n, radius=A, phi2d=0.4, seed=1)
  return loc, np.array([side, side, 0.0])


def sweeps(reps):
  from rigidmultiblobswall_amd.context import MobilityContext
  ctx = MobilityContext(0)
  out2 = torch.empty(2, dtype=torch.float64, device="cuda:0")
  rows = []
  for n in (10000, 100000, 262144):
    for kind in ("monolayer", "cloud", "monolayer_cull_off"):
      r, L = _layout("cloud" if kind == "cloud" else "monolayer", n)
      ctx.set_option("force_cull", 0 if kind.endswith("cull_off") else 1)
      ctx.set_option("potential_resort", 1)             # call times: the energy pays its sort on every call, the forces reuse it
      ctx.set_option("timing", 1)                       # kernel times: the library's own events around each sweep
      rd = torch.as_tensor(r.reshape(-1), device="cuda:0")
      ctx.set_positions(rd, A, L, wall=False)
      fout = torch.empty(3 * n, dtype=torch.float64, device="cuda:0")
      pot = lambda: ctx.blob_potential_device(EPS, B, A, out=out2, **WALL)     # noqa: E731
      frc = lambda: ctx.blob_blob_force_device(EPS, B, A, out=fout)            # noqa: E731
      pot(); frc(); pot(); frc()
      torch.cuda.synchronize()
      tp, tf = [], []
      ctx.timing_reset()
      for _ in range(reps):                # alternating: both see the same clocks and the same neighbours on the chip
        tp.append(_event_ms(pot)); tf.append(_event_ms(frc))
      ring = ctx.timing_collect()          # potential sweep, force sweep, potential, ... (each without its finishing launch)
      kp, kf = ring[0::2], ring[1::2]
      row = dict(n=n, layout=kind, potential_kernel_ms=float(np.median(kp)), force_kernel_ms=float(np.median(kf)),
                 kernel_ratio=float(np.median(kp) / np.median(kf)), potential_call_ms=float(np.median(tp)), force_call_ms=float(np.median(tf)),
                 potential_kernel_min_ms=float(np.min(kp)), force_kernel_min_ms=float(np.min(kf)), U=out2.cpu().tolist())
      print(json.dumps(row), flush=True)
      rows.append(row)
  ctx.set_option("force_cull", 1)
  ctx.set_option("timing", 0)
  ctx.close()
  return rows


def sort_reuse(reps):
  """set_positions + energy along a random walk: before every evaluation every blob moves by 0.1 a times a fresh uniform
  draw in (-1, 1) in x and in y (a Metropolis proposal that is always accepted; heights stay, so no blob crosses the wall
  and the walk can go on), 64 evaluations per timing, the walk going on from timing to timing.  At K = 64 the last
  evaluations before a rebuild run on a permutation that is 0.46 a r.m.s. per coordinate old.  The draw is one small
  launch inside the timing, the same for every K."""
  from rigidmultiblobswall_amd.context import MobilityContext
  ctx = MobilityContext(0)
  out2 = torch.empty(2, dtype=torch.float64, device="cuda:0")
  rows = []
  for n in (10000, 100000, 262144):
    for kind in ("monolayer", "cloud"):
      r, L = _layout(kind, n)
      gen = torch.Generator(device="cuda:0")
      gen.manual_seed(3)
      mask = torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64, device="cuda:0")
      row = dict(n=n, layout=kind)
      for every in (1, 4, 16, 64):
        ctx.set_option("potential_resort", every)
        pos = torch.as_tensor(r, device="cuda:0").clone()

        def cycle():
          for k in range(64):
            pos.add_((2 * torch.rand(pos.shape, dtype=torch.float64, device="cuda:0", generator=gen) - 1) * mask, alpha=0.1 * A)
            ctx.set_positions(pos, A, L, wall=False)
            ctx.blob_potential_device(EPS, B, A, out=out2, **WALL)
        cycle()
        torch.cuda.synchronize()
        row["resort_%d_ms_per_eval" % every] = float(np.median([_event_ms(cycle) for _ in range(max(3, reps // 2))])) / 64
      print(json.dumps(row), flush=True)
      rows.append(row)
  ctx.close()
  return rows


def one_blob_cost(reps):
  """The sweep with and without its one-blob terms (weight and wall strength zero: step 0 of a diagonal unit then adds
  w z = 0 and skips the exponential) -- what carrying them on the diagonal units costs the launch."""
  from rigidmultiblobswall_amd.context import MobilityContext
  ctx = MobilityContext(0)
  ctx.set_option("timing", 1)
  out2 = torch.empty(2, dtype=torch.float64, device="cuda:0")
  rows = []
  for n in (10000, 262144):
    r, L = _layout("monolayer", n)
    ctx.set_positions(torch.as_tensor(r.reshape(-1), device="cuda:0"), A, L, wall=False)
    with_terms = lambda: ctx.blob_potential_device(EPS, B, A, out=out2, **WALL)     # noqa: E731
    without = lambda: ctx.blob_potential_device(EPS, B, A, out=out2)                # noqa: E731
    with_terms(); without()
    ctx.timing_reset()
    for _ in range(2 * reps):
      with_terms(); without()
    ring = ctx.timing_collect()
    row = dict(n=n, with_one_blob_terms_ms=float(np.median(ring[0::2])), pair_terms_only_ms=float(np.median(ring[1::2])))
    print(json.dumps(row), flush=True)
    rows.append(row)
  ctx.close()
  return rows


def mcmc_steps(steps=30):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd.structures import icosahedron_shell, roller_monolayer
  rows = []
  cwd = os.getcwd()
  for nb in (1000, 21845):
    for rng in ("reference", "batched"):
      with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
          shell = icosahedron_shell(0.7921)
          loc, q, side = roller_monolayer(nb, radius=1.0, phi2d=0.25, seed=2)
          with open("shell.vertex", "w") as f:
            f.write("12\n" + "".join("%.17g %.17g %.17g\n" % tuple(x) for x in shell))
          with open("shell.clones", "w") as f:
            f.write("%d\n" % nb + "".join("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" % (tuple(x) + tuple(p)) for x, p in zip(loc, q)))
          with open("data.main", "w") as f:
            f.write("n_steps %d\nn_save %d\ninitial_step 0\ng 0.0124\nblob_radius 0.416\nkT 0.0041419464\nperiodic_length %r %r 0\n"
                    "repulsion_strength_wall 0.03\ndebye_length_wall 0.04\nrepulsion_strength 0.03\ndebye_length 0.04\nseed 1\n"
                    "output_name run\nstructure shell.vertex shell.clones\n" % (steps, 10 * steps, float(side), float(side)))
          s = MCMCSampler(ReadInput("data.main"), device=0, rng=rng, write_files=False)
          tm = dict(upload=[], proposal=[], sweep_readback=[])

          def timed(fn, key):           # the stages of _DeviceState.propose, each followed by a device synchronisation
            def call(*args):
              t0 = time.perf_counter()
              res = fn(*args)
              torch.cuda.synchronize()
              tm[key].append(time.perf_counter() - t0)
              return res
            return call
          st = s.state
          st.upload, st.compose, st._energy = timed(st.upload, "upload"), timed(st.compose, "proposal"), timed(st._energy, "sweep_readback")
          torch.cuda.synchronize()
          t0 = time.perf_counter()
          s.run()
          wall = time.perf_counter() - t0
          tm = {k: 1e3 * float(np.median(v[3:])) for k, v in tm.items()}
          row = dict(bodies=nb, blobs=s.n_blobs, rng=rng, draws_ms=1e3 * s.draw_seconds / steps, upload_ms=tm["upload"], proposal_ms=tm["proposal"],
                     sweep_readback_ms=tm["sweep_readback"], step_ms_wall_with_syncs=1e3 * wall / steps, acceptance=s.accepted_moves / steps)
          s.close()
        finally:
          os.chdir(cwd)
      print(json.dumps(row), flush=True)
      rows.append(row)
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--reps", type=int, default=7)
  ap.add_argument("--skip-mcmc", action="store_true")
  args = ap.parse_args()
  res = dict(device=torch.cuda.get_device_name(0), sweeps=sweeps(args.reps), one_blob_cost=one_blob_cost(args.reps),
             sort_reuse=sort_reuse(args.reps))
  if not args.skip_mcmc:
    res["mcmc_step"] = mcmc_steps()
  if args.out:
    with open(args.out, "w") as fh:
      json.dump(res, fh, indent=1)


if __name__ == "__main__":
  main()
