#!/usr/bin/env python
"""Single-source wall-tt products of the three one-vector symmetric kernels as hex bit patterns, to compare two builds on
one machine.  With ONE nonzero source blob every target's sum has a single term, so the result words do not depend on
the order in which the atomics land: sym2t_kernel (`sym_two_targets` 2), sym_kernel (`sym_two_targets` 0, `sym_coop` 0)
and sym_coop_kernel (`sym_coop` 2) must print the same words, and so must two builds whose pair blocks are bit-identical.
257 blobs (5 tiles, the last one partial; ~1/7 of them below z = a), source blobs in the first, a middle and the last
tile.  Per product: the kernel family that ran (`last_path`), a SHA-256 of the 3N result words, and -- once per source --
the words themselves; `diff` of two runs is the check.

  python tools/sym_single_source_bits.py [--root OTHER_TREE] > bits.txt      (--root: the built tree whose package is loaded)
"""
import argparse
import hashlib
import os
import sys

import numpy as np

N = 257
SOURCES = (5, 130, 256)
KERNELS = (("sym2t_kernel", {"sym_two_targets": 2}), ("sym_kernel", {"sym_two_targets": 0, "sym_coop": 0}),
           ("sym_coop_kernel", {"sym_two_targets": 0, "sym_coop": 2}))


def cloud(n=N):
  """mobility/test_blobs.py:31-44 at constant number density: dense, overlapping, blobs below z = a."""
  rng = np.random.RandomState(n)
  eta, a = 7.0, 0.13
  return 5 * a * (n / 1000.0) ** (1.0 / 3.0) * rng.rand(n, 3), rng.randn(n, 3), eta, a


def products(Ctx, source, n=N):
  """name -> (last_path, result of the wall-tt product with the force of blob `source` alone), one fresh context each."""
  r, f, eta, a = cloud(n)
  f1 = np.zeros_like(f)
  f1[source] = f[source]
  out = {}
  for name, opts in KERNELS:
    ctx = Ctx(0)
    try:
      for k, v in opts.items():
        ctx.set_option(k, v)
      ctx.set_positions(r, a, None, wall=True)
      u = ctx.matvec("tt", f1.reshape(-1), eta)
      out[name] = (ctx.get_option("last_path"), u)
    finally:
      ctx.close()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  from rigidmultiblobswall_amd import MobilityContext
  for s in SOURCES:
    res = products(MobilityContext, s)
    for name, (path, u) in res.items():
      print("n=%d source=%d %s last_path %d sha256 %s" % (N, s, name, path, hashlib.sha256(u.view(np.uint64).tobytes()).hexdigest()))
    w = res[KERNELS[0][0]][1].view(np.uint64)
    for i in range(N):
      print("n=%d source=%d u[%d] %016x %016x %016x" % (N, s, i, w[3 * i], w[3 * i + 1], w[3 * i + 2]))


if __name__ == "__main__":
  main()
