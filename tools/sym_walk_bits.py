#!/usr/bin/env python
"""Results of the seven wave-owned symmetric kernels with one target blob per lane (sym_kernel, sym2_kernel, symx_kernel and
its DET variant, sym32_tt_kernel, symx32_kernel, sym_force_kernel, sym_force32_kernel) as bit patterns, under every cut of
the step range the options offer -- to compare two builds on one machine, and the cases of tests/test_gpu_sym_walk.py.

The inputs make the result words independent of the order in which the atomics land, so every plan of a case must give
the same words, and so must two builds whose walk over the step range (csrc/sym_walk.h) visits the same pairs:
  * mobility products: 257 blobs (5 tiles, the last one partial, blobs below z = a: the cloud of
    tools/sym_single_source_bits.py) with the force -- and the torque, for the multi-block operations -- on ONE blob, so
    every target's sum has a single term;
  * pair forces: isolated dimers.  Blob i is paired with blob (i + 97) mod 257 where both are still free (i ascending);
    97 > 64 puts those pairs into off-diagonal units, and the blobs left over are paired inside their tile (diagonal
    units).  Dimers sit 50 apart, beyond the reach of every law here, so every non-partner term is exactly +-0.
Plans: the default, `sym_chunk_steps` 16 with `sym_min_steps` 7, `sym_order` flipped, `sym_xcd` flipped, and -- where the
entry point has pair shards -- the sum of three.  One line per case and plan: the SHA-256 of the result words.

  python tools/sym_walk_bits.py [--root OTHER_TREE] > bits.txt      (--root: the built tree whose package is loaded)
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
  if p not in sys.path:
    sys.path.insert(0, p)
import sym_single_source_bits as single      # noqa: E402

N = single.N
SOURCES = single.SOURCES
KINDS = ("tt", "tr", "rt", "rr")
BOX = np.array([1.0, 1.5, 0.0])
WAVE = {"sym_two_targets": 0, "sym_coop": 0}      # the per-wave kernels at every size
PLANS = ("default", "chunk16_min7", "order_flipped", "xcd_flipped")
SHARDS = 3
# pair forces
SPACING = 50.0
FORCE = dict(eps=0.7, b=0.02, a=0.13)             # reach 2a + 750 b = 15.26 (fp32: 2a + 110 b)
TABLE_K = 16


def set_plan(ctx, plan):
  if plan == "chunk16_min7":
    ctx.set_option("sym_chunk_steps", 16)
    ctx.set_option("sym_min_steps", 7)
  elif plan == "order_flipped":
    ctx.set_option("sym_order", 1 - ctx.get_option("sym_order"))
  elif plan == "xcd_flipped":
    ctx.set_option("sym_xcd", 1 - ctx.get_option("sym_xcd"))
  else:
    assert plan == "default"


def one_blob(source, seed):
  """(force, torque) as 3N vectors that are zero but on blob `source`"""
  rng = np.random.RandomState(1000 * seed + source)
  out = []
  for _ in range(2):
    v = np.zeros((N, 3))
    v[source] = rng.randn(3)
    out.append(v.reshape(-1))
  return out


def dimer_pairs():
  free = np.ones(N, dtype=bool)
  pairs = []
  for i in range(N):
    j = (i + 97) % N
    if free[i] and free[j]:
      pairs.append((i, j)); free[i] = free[j] = False
  for t in range(0, N, 64):      # the blobs left over: pairs inside a tile
    left = [i for i in range(t, min(N, t + 64)) if free[i]]
    for i, j in zip(left[0::2], left[1::2]):
      pairs.append((i, j)); free[i] = free[j] = False
  return pairs


def dimers(lo, hi):
  """(N, 3) positions: dimer centres on a cubic lattice of SPACING, partners between lo and hi apart; loners on it too."""
  rng = np.random.RandomState(97)
  side = int(np.ceil(N ** (1.0 / 3.0)))
  sites = SPACING * np.array([(x, y, z) for x in range(side) for y in range(side) for z in range(side)], dtype=np.float64)
  r = np.zeros((N, 3))
  pairs = dimer_pairs()
  used = np.zeros(N, dtype=bool)
  for k, (i, j) in enumerate(pairs):
    d = rng.randn(3)
    d *= rng.uniform(lo, hi) / np.linalg.norm(d)
    r[i] = sites[k] - 0.5 * d; r[j] = sites[k] + 0.5 * d
    used[i] = used[j] = True
  for k, i in enumerate(np.flatnonzero(~used)):
    r[i] = sites[len(pairs) + k]
  return r, pairs


def radii():
  return FORCE["a"] * (0.6 + 0.8 * np.random.RandomState(N).rand(N))


def pair_table():
  import _pair_table_numpy as pt
  return pt.lj_table(TABLE_K)


class Case(object):
  """One entry point on one kernel.  run(ctx, shard, nshards) -> tuple of CUDA tensors; `path` = last_path after it."""
  def __init__(self, name, kernel, path, run, shards, ref=None, tol=None):
    self.name, self.kernel, self.path, self.run, self.shards, self.ref, self.tol = name, kernel, path, run, shards, ref, tol


class Group(object):
  """Cases that share a context: geometry (r, a, L, wall), options, and what else the context needs (`prepare`)."""
  def __init__(self, name, geometry, options, cases, prepare=None):
    self.name, self.geometry, self.options, self.cases, self.prepare = name, geometry, dict(options), cases, prepare


def _dev(v):
  import torch
  return torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")


def mobility_groups():
  r, _, eta, a = single.cloud(N)
  groups = []
  for gname, L, wall in (("wall", None, True), ("no_wall", None, False), ("wall_box", BOX, True)):
    box = L is not None
    kw = dict(periodic_length=L) if box else {}
    w = int(wall)

    def orc(kind, v, _w=w, _kw=kw):
      return lambda o: o._wrapped(kind, _w, r, v, eta, a, **_kw)

    def single_run(kind, v):
      return lambda ctx, g, G: (ctx.matvec_device(kind, _dev(v), eta) if G == 1 else ctx.matvec_pairshard_device(kind, _dev(v), eta, g, G),)

    def op_run(op, vs):
      return lambda ctx, g, G: ctx.matvec_op_device(op, [_dev(v) for v in vs], eta, shard=g, nshards=G)

    f64, det, f32 = [], [], []
    for s in SOURCES:
      f, t = one_blob(s, 1)
      f2, _ = one_blob(s, 2)
      grand = lambda o, f=f, t=t, orc=orc: [orc("tt", f)(o) + orc("tr", t)(o), orc("rt", f)(o) + orc("rr", t)(o)]      # noqa: E731
      fused = lambda o, f=f, t=t, orc=orc: [orc("tt", f)(o) + orc("tr", t)(o)]                                           # noqa: E731
      for kind in (("tt",) if box else KINDS):
        v = f if kind in ("tt", "rt") else t
        f64.append(Case("sym_kernel %s %s source %d" % (kind, gname, s), "sym_kernel", 1, single_run(kind, v), True,
                        lambda o, k=kind, v=v, orc=orc: [orc(k, v)(o)], 1e-12))
      f64.append(Case("symx_kernel grand %s source %d" % (gname, s), "symx_kernel", 1, op_run("grand", (f, t)), True, grand, 1e-12))
      if not box:
        f64.append(Case("sym2_kernel tt %s source %d" % (gname, s), "sym2_kernel", 1,
                        lambda ctx, g, G, f=f, f2=f2: ctx.matvec2_device("tt", _dev(f), _dev(f2), eta, shard=g, nshards=G), True,
                        lambda o, f=f, f2=f2, orc=orc: [orc("tt", f)(o), orc("tt", f2)(o)], 1e-12))
        f64.append(Case("symx_kernel fused row %s source %d" % (gname, s), "symx_kernel", 1, op_run("velocity_from_force_torque", (f, t)), True,
                        fused, 1e-12))
        det.append(Case("symx_kernel DET grand %s source %d" % (gname, s), "symx_kernel<DET>", 2, op_run("grand", (f, t)), True, grand, 1e-12))
        f32.append(Case("sym32_tt_kernel tt %s source %d" % (gname, s), "sym32_tt_kernel", 1, single_run("tt", f), True,
                        lambda o, f=f, orc=orc: [orc("tt", f)(o)], 1e-5))
        f32.append(Case("symx32_kernel grand %s source %d" % (gname, s), "symx32_kernel", 1, op_run("grand", (f, t)), True, grand, 2e-5))
    geometry = (r, a, L, wall)
    groups.append(Group("mobility " + gname, geometry, WAVE, f64))
    if not box:
      groups.append(Group("mobility deterministic " + gname, geometry, dict(WAVE, deterministic=2), det))
      groups.append(Group("mobility precision 32 " + gname, geometry, dict(WAVE, precision=32), f32))
  return groups


def force_groups():
  eps, b, a = FORCE["eps"], FORCE["b"], FORCE["a"]
  r, _ = dimers(a, 3 * a)                      # (r - 2a)/b in [-6.5, 6.5]
  rad = radii()
  T = pair_table()
  rt, _ = dimers(0.9, 2.4)                     # inside [r0, r_cut) of the table
  zero = np.zeros(3)

  def contact(ctx, g, G):
    return (ctx.blob_blob_force_device(eps, b, a) if G == 1 else ctx.blob_blob_force_pairshard_device(eps, b, a, g, G),)

  def by_radii(ctx, g, G):
    return (ctx.blob_blob_force_radii_device(_dev(rad), eps, b),)

  def table(ctx, g, G):
    return (ctx.pair_table_force_device(),)

  ref_contact = lambda o: [o.calc_blob_blob_forces_oracle(r, repulsion_strength=eps, debye_length=b, blob_radius=a, periodic_length=zero)]      # noqa: E731
  ref_radii = lambda o: [o.calc_blob_blob_forces_radii_oracle(r, rad, repulsion_strength=eps, debye_length=b, periodic_length=zero)]              # noqa: E731
  sym = {"deterministic": 0}
  return [
      Group("forces", (r, a, None, False), sym,
            [Case("sym_force_kernel contact", "sym_force_kernel", 1, contact, True, ref_contact, 1e-12),
             Case("sym_force_kernel radii", "sym_force_kernel", 1, by_radii, False, ref_radii, 1e-12)]),
      Group("forces table", (rt, 1.0, None, False), sym, [Case("sym_force_kernel table", "sym_force_kernel", 1, table, False, "table", None)],
            prepare=lambda ctx: ctx.set_pair_table(T)),
      Group("forces precision 32", (r, a, None, False), dict(sym, precision=32),
            [Case("sym_force32_kernel contact", "sym_force32_kernel", 1, contact, True, ref_contact, 1e-5),
             Case("sym_force32_kernel radii", "sym_force32_kernel", 1, by_radii, False, ref_radii, 1e-5)]),
  ]


def groups():
  return mobility_groups() + force_groups()


def open_context(Ctx, group, plan):
  r, a, L, wall = group.geometry
  ctx = Ctx(0)
  for k, v in group.options.items():
    ctx.set_option(k, v)
  set_plan(ctx, plan)
  ctx.set_positions(np.ascontiguousarray(r), a, L, wall)
  if group.prepare:
    group.prepare(ctx)
  return ctx


def run_group(Ctx, group):
  """{(case name, plan): (3N k,) float64 result}; plan "shards3" = the sum of the three pair shards under the default plan.
  last_path is asserted after every launch."""
  out = {}
  for plan in PLANS:
    ctx = open_context(Ctx, group, plan)
    try:
      for case in group.cases:
        res = case.run(ctx, 0, 1)
        path = ctx.get_option("last_path")
        assert path == case.path, "%s under %s: last_path %d, expected %d" % (case.name, plan, path, case.path)
        out[case.name, plan] = np.concatenate([t.cpu().numpy().reshape(-1) for t in res])
        if plan == "default" and case.shards:
          parts = []
          for g in range(SHARDS):
            parts.append([t.clone() for t in case.run(ctx, g, SHARDS)])
            assert ctx.get_option("last_path") == case.path, (case.name, "shard", g)
          out[case.name, "shards3"] = np.concatenate([(parts[0][c] + parts[1][c] + parts[2][c]).cpu().numpy().reshape(-1)
                                                      for c in range(len(parts[0]))])
    finally:
      ctx.close()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--root", default=ROOT)
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  from rigidmultiblobswall_amd import MobilityContext
  for group in groups():
    res = run_group(MobilityContext, group)
    for (name, plan), u in res.items():
      print("%s | %s | %s" % (name, plan, hashlib.sha256(np.ascontiguousarray(u).view(np.uint64).tobytes()).hexdigest()))


if __name__ == "__main__":
  main()
