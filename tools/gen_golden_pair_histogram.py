"""Goldens of the pair-distance histogram from the reference's OWN g(r) program.  Build-container only (needs the reference
tree and a C++ compiler).

Compiles multi_bodies/examples/Radial_Dist_Test/gr_pseudo2D_single_blob.cpp UNCHANGED into a temporary directory (never into
this repository), runs it on small generated `.config` files and writes tests/golden/g17_gr_<name>.npz: the frames, the
program's arguments (np, lx, ly, lz), its bin count and the text it printed (`r g hist` per bin, hist = ordered pairs).

  quasi2d   4 frames x 150 points in a 40 x 16 box, heights in a thin layer (lz = 0: the program never images z)
  shifted   the same points, each moved by whole periods in x and y out of the primary cell

A quirk of the program: it loops on `!eof()`, so a file that ENDS IN A NEWLINE gets one more pass through the loop body -- the
read fails, the coordinate arrays keep the last frame, which is counted a second time, and the result is normalised by
frames + 1.  A file without the final newline hits end-of-file inside the last read and is counted correctly.  The files
written here have no final newline.

Every input satisfies the edge-margin precondition of the tests (tests/_pair_hist_numpy.py): in long double no pair has r / dr
within 1e-9 of an integer, so a last-bit difference in r cannot move a pair across a bin edge and exact equality of the
integer column is a fair demand.  A set that fails gets another seed.

Usage:  python tools/gen_golden_pair_histogram.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pair_hist_numpy as phnp  # noqa: E402

PROGRAM = os.path.join("multi_bodies", "examples", "Radial_Dist_Test", "gr_pseudo2D_single_blob.cpp")
N_BINS = 2000      # fixed in the program
N_FRAMES, N_POINTS, LX, LY, LZ = 4, 150, 40.0, 16.0, 0.0


def make_frames(rng, shifted):
  x = np.column_stack([rng.uniform(0, LX, N_FRAMES * N_POINTS), rng.uniform(0, LY, N_FRAMES * N_POINTS),
                       rng.uniform(0.3, 1.5, N_FRAMES * N_POINTS)]).reshape(N_FRAMES, N_POINTS, 3)
  if shifted:
    x[:, :, 0] += LX * rng.randint(-3, 4, (N_FRAMES, N_POINTS))
    x[:, :, 1] += LY * rng.randint(-3, 4, (N_FRAMES, N_POINTS))
  return x


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--ref", default="/root/reference")
  ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
  args = ap.parse_args()
  L = (LX, LY, LZ)
  with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "gr")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-o", exe, os.path.join(args.ref, PROGRAM)])
    for name, shifted, seed in (("quasi2d", False, 1700), ("shifted", True, 1750)):
      frames = phnp.points_with_margin(lambda rng: make_frames(rng, shifted), L, 0.5 * LX, N_BINS, seed)
      path = os.path.join(tmp, name + ".config")
      with open(path, "w") as f:
        f.write(phnp.config_text(frames, final_newline=False))
      out = subprocess.check_output([exe, path, str(N_POINTS), repr(LX), repr(LY), repr(LZ)]).decode()
      r, g, hist = phnp.parse_gr(out)
      assert len(r) == N_BINS and hist.sum() > 0
      assert np.array_equal(hist, 2 * phnp.counts(frames, L, 0.5 * LX, N_BINS).astype(np.int64)), name
      target = os.path.join(args.out, "g17_gr_%s.npz" % name)
      np.savez_compressed(target, frames=frames, n_points=N_POINTS, periodic_length=np.array(L), n_bins=N_BINS, output=np.array(out),
                          margin=phnp.edge_margin(frames, L, 0.5 * LX, N_BINS))
      print("%s: %d bytes, %d ordered pairs counted" % (target, os.path.getsize(target), hist.sum()))


if __name__ == "__main__":
  main()
