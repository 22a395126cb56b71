#!/usr/bin/env python
"""Every result of the pair-once sweeps (pair_once_kernels.h) as hex bit patterns, to compare two builds on one machine:
(U_one, U_pair) of the soft and the yukawa blob energy, U_body, and the pair histogram (64 bins, r_max = side / 5), on
seeded clouds of 129, 2200 and 24577 points, open and periodic in x and y, tile culling on and off, each in a fresh context
with "potential_resort" 1.  The energies are bit-reproducible for a given launch plan and permutation, so two builds that
plan and add alike print the same text; `diff` is the check.

  python tools/pair_once_bits.py [--root OTHER_TREE] > bits.txt      (--root: the built tree whose package is loaded)
"""
import argparse
import os
import struct
import sys

import numpy as np

A = 0.31
SIZES = (129, 2200, 24577)
N_BINS = 64


def hex64(v):
  return struct.pack(">d", float(v)).hex()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  from rigidmultiblobswall_amd import MobilityContext
  for n in SIZES:
    rng = np.random.RandomState(n)
    side = 2.2 * A * n ** (1.0 / 3.0)
    r = np.column_stack([side * rng.rand(n), side * rng.rand(n), 0.2 * A + side * rng.rand(n)])
    r[::97, 2] -= 0.5 * A      # some blobs below z = a and behind the wall: the guarded loop runs
    for periodic in (0, 1):
      L = np.array([side, side, 0.0]) * periodic
      for cull in (1, 0):
        ctx = MobilityContext(0)
        try:
          ctx.set_option("potential_resort", 1)
          ctx.set_option("force_cull", cull)
          ctx.set_positions(r, A, L, wall=False)
          tag = "n=%d periodic=%d cull=%d" % (n, periodic, cull)
          for form in ("soft", "yukawa"):
            u = ctx.blob_potential(0.7, 0.02 * A, A, repulsion_strength_wall=1.3, debye_length_wall=0.5 * A, weight=0.9, potential=form)
            print("%s %s U_one %s U_pair %s" % (tag, form, hex64(u[0]), hex64(u[1])))
          print("%s U_body %s" % (tag, hex64(ctx.body_body_potential(1.7, 0.01))))
          print("%s hist %s" % (tag, " ".join("%x" % int(c) for c in ctx.pair_histogram(0.2 * side, N_BINS))))
        finally:
          ctx.close()


if __name__ == "__main__":
  main()
