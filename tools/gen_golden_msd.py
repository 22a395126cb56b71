"""Golden of the mean-square displacement from the reference's OWN calc_msd_data_from_trajectory.  Build-container only
(needs the reference tree; nothing of it is copied).

Imports general_application_utils from the reference tree, runs calc_msd_data_from_trajectory on seeded single-body random
walks (tests/_msd_numpy.py: random_walk, 400 frames, bodies near 10, steps of about 0.05, rotations of about 0.05 rad) and
writes tests/golden/g18_msd_reference.npz: per case the inputs (locations, orientations, dt, end, burn_in,
trajectory_length, the body-frame offset of the tracking function), the returned (trajectory_length, 6, 6) array, and what
the run itself showed of the frame selection: how often the tracking function was called (= kept frames) and how many
origins were taken (calls of calc_total_msd_from_matrix_and_center / trajectory_length).

  plain     burn_in 0,  trajectory_length 20, end 1.0: data_interval 1, the location itself is tracked
  interval  burn_in 7,  trajectory_length 10, end 2.0: data_interval 3 (131 kept frames)
  tracked   burn_in 25, trajectory_length 15, end 2.5: data_interval 2, tracking function location + R(q) p

Usage:  python tools/gen_golden_msd.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _msd_numpy as mnp  # noqa: E402

N_FRAMES, DT = 400, 0.1
CASES = (("plain", 1800, 0, 20, 1.0, None), ("interval", 1810, 7, 10, 2.0, None), ("tracked", 1820, 25, 15, 2.5, (0.3, -0.2, 0.45)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--ref", default="/root/reference")
  ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
  args = ap.parse_args()
  sys.path.insert(0, args.ref)
  import general_application_utils as gau
  data = {"cases": np.array([c[0] for c in CASES])}
  for name, seed, burn_in, length, end, offset in CASES:
    frames = mnp.random_walk(N_FRAMES, 1, seed)[:, 0]
    loc, quat = frames[:, :3], frames[:, 3:]
    calls = {"center": 0, "pair": 0}
    p = np.zeros(3) if offset is None else np.array(offset)

    def center(location, orientation):
      calls["center"] += 1
      return location + np.dot(orientation.rotation_matrix(), p) if offset is not None else location

    pair = gau.calc_total_msd_from_matrix_and_center

    def counted(*a):
      calls["pair"] += 1
      return pair(*a)
    gau.calc_total_msd_from_matrix_and_center = counted
    try:
      with contextlib.redirect_stdout(io.StringIO()):
        msd = gau.calc_msd_data_from_trajectory([list(x) for x in loc], [list(q) for q in quat], center, DT, end, burn_in=burn_in,
                                                trajectory_length=length)
    finally:
      gau.calc_total_msd_from_matrix_and_center = pair
    assert calls["pair"] % length == 0
    # the restatement of the tests must already agree (same arithmetic, another order)
    kept = [k for k in range(N_FRAMES) if k > burn_in and k % (int(end / DT / length) + 1) == 0]
    S, n = mnp.sums(frames[kept[1:]][:, None, :], length, offsets=offset, origins="window")
    div = N_FRAMES / (int(end / DT / length) + 1) - length - burn_in / (int(end / DT / length) + 1)
    print("%-9s kept %3d origins %3d  max |restatement - reference| = %.3e of %.3e" %
          (name, calls["center"], calls["pair"] // length, np.abs(S / div - msd).max(), np.abs(msd).max()))
    data.update({name + "_locations": loc, name + "_orientations": quat, name + "_dt": DT, name + "_end": end, name + "_burn_in": burn_in,
                 name + "_trajectory_length": length, name + "_offset": p, name + "_has_offset": offset is not None,
                 name + "_msd": np.asarray(msd), name + "_n_kept": calls["center"], name + "_n_origins": calls["pair"] // length})
  target = os.path.join(args.out, "g18_msd_reference.npz")
  np.savez_compressed(target, **data)
  print("%s: %d bytes" % (target, os.path.getsize(target)))


if __name__ == "__main__":
  main()
