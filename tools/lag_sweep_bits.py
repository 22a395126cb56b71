#!/usr/bin/env python
"""Every result of the lag sweeps (lag_sweep_kernels.h: a lane owns a lag) as bit patterns, to compare two builds on one
machine: the 6 x 6 MSD sums, the collective and self scattering sums, and the three streaming classes (MSD, scattering, van
Hove) fed in pieces.  One line per case: a tag, the SHA-256 of the result tensor's bytes, the hex pattern of its last entry.
The inputs are seeded and the sums are bit-reproducible for a given launch plan, so two builds that plan and add alike
print the same text; `cmp` is the check.  The plan depends on the CU count: run both on the same machine.

Shapes (n_lags, F): (1, 1), (64, 64), (65, 70), (130, 40) under "all" only, (130, 600) -- the last is three staged windows
at chunk 256 and enters the masked tail.

  python tools/lag_sweep_bits.py [--root OTHER_TREE] > bits.txt      (--root: the built tree whose package is loaded)
"""
import argparse
import hashlib
import os
import struct
import sys

import numpy as np

SHAPES = ((1, 1), (64, 64), (65, 70), (130, 40), (130, 600))
BOX = (6.0, 4.5, 3.0)


def line(tag, t):
  a = np.ascontiguousarray(t.cpu().numpy())
  last = a.reshape(-1)[-1:]
  print("%s %s %s" % (tag, hashlib.sha256(a.tobytes()).hexdigest(), last.tobytes()[::-1].hex() if last.size else "-"))


def conventions(n_lags, F):
  return ("all",) if F < n_lags else ("window", "all")


def rigid_frames(F, N, seed):
  """a random walk of N bodies: rows x y z s p1 p2 p3, unit quaternions to rounding"""
  rng = np.random.RandomState(seed)
  x = np.cumsum(0.05 * rng.randn(F, N, 3), axis=0) + rng.uniform(0, 5, (1, N, 3))
  q = np.cumsum(0.03 * rng.randn(F, N, 4), axis=0) + rng.randn(1, N, 4)
  return np.ascontiguousarray(np.concatenate([x, q / np.linalg.norm(q, axis=-1, keepdims=True)], axis=-1))


def point_frames(F, N, seed):
  rng = np.random.RandomState(seed)
  return np.ascontiguousarray(np.cumsum(0.05 * rng.randn(F, N, 3), axis=0) + rng.uniform(0, 1, (1, N, 3)) * np.array(BOX))


def wavevectors(K, seed):
  wv = np.random.RandomState(seed).randint(-4, 5, (K, 3)).astype(np.int32)
  wv[np.all(wv == 0, axis=1), 0] = 1
  return wv


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import torch
  from rigidmultiblobswall_amd import MobilityContext, msd, scattering, vanhove
  ctx = MobilityContext(0)
  dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
  try:
    for n_lags, F in SHAPES:
      for N in (1, 3, 65):
        frames = dev(rigid_frames(F, N, 1000 * n_lags + N))
        offsets = np.random.RandomState(N).uniform(-0.5, 0.5, (N, 3))
        for origins in conventions(n_lags, F):
          for chunk in (0, 1, 7):
            for off in (None, offsets):
              S, _ = ctx.msd_frames_device(frames, n_lags, offsets=off, origins=origins, origin_chunk=chunk)
              line("msd L=%d F=%d N=%d %s chunk=%d off=%d" % (n_lags, F, N, origins, chunk, off is not None), S)
      for N in (1, 65):
        frames = dev(point_frames(F, N, 2000 * n_lags + N))
        for K in (1, 3, 4, 5, 65):      # self passes in groups 3 | 3 + 1 | 3 + 2; 65 grid rows of the collective sweep
          wv = wavevectors(K, K)
          modes = ctx.density_modes_frames_device(frames, BOX, wv)
          ranges = [(o, 0, None) for o in conventions(n_lags, F)] + ([("all", 3, None)] if (n_lags, F, N) == (65, 70, 65) else [])
          for origins, o_begin, o_end in ranges:
            tag = "L=%d F=%d N=%d K=%d %s o_begin=%d" % (n_lags, F, N, K, origins, o_begin)
            line("scat C " + tag, ctx.scattering_lags_device(modes, n_lags, origins=origins, o_begin=o_begin, o_end=o_end)[0])
            line("scat Sf " + tag, ctx.self_scattering_frames_device(frames, BOX, wv, n_lags, origins=origins, o_begin=o_begin, o_end=o_end)[0])
    # the streaming classes: (130, 600) in pieces of 1, 7 and the rest, under "all"
    n_lags, F = 130, 600
    feed = lambda acc, f: acc.add_frames(f[:1]).add_frames(dev(f[1:8])).add_frames(f[8:]).finish()      # noqa: E731
    acc = feed(msd.MeanSquareDisplacement(3, n_lags, origins="all", offsets=(0.2, 0.1, -0.3), ctx=ctx), rigid_frames(F, 3, 7))
    line("class msd sums", acc._sums)
    acc = feed(scattering.IntermediateScattering(3, BOX, wavevectors(5, 5), n_lags=n_lags, origins="all", self_part=True, ctx=ctx), point_frames(F, 3, 8))
    line("class scat C", acc._C)
    line("class scat Sf", acc._Sf)
    acc = feed(vanhove.VanHove(65, BOX, n_lags, r_max=1.5, n_bins=64, origins="all", ctx=ctx), point_frames(F, 65, 9))
    line("class vh moments", acc._M)
    line("class vh Hs", acc._Hs)
    line("class vh Hd", acc._Hd)
  finally:
    ctx.close()


if __name__ == "__main__":
  main()
