#!/usr/bin/env python
"""Worst element-wise error of every pair block per (kernel family, kind, boundary), from the GPU test itself.

Runs tests/test_gpu_pair_blocks.py in this process (the same code, no launch beyond the test's own) and writes the ratios
the test recorded: |got - EXT| / (C eps s) maximised over the designed clouds, the blob pairs and the nine elements, with the
extended-precision reference, the scale s and the yardstick C of tests/_mobility_numpy.py (C = C_ORACLE, eps = 2^-53; for the
`f32_*` families C_ORACLE32 and 2^-24).  The test's bound is MARGIN = 4 in these units.

  python tools/pair_blocks_report.py [--out profiles/FILE.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  import pytest
  rc = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_pair_blocks.py")])
  import torch
  import _mobility_numpy as mn
  import _pair_blocks_gpu as pb
  lines = ["# tools/pair_blocks_report.py on %s; pytest exit status %d; %d (family, kind, boundary) rows" %
           (torch.cuda.get_device_name(0), int(rc), len(pb.RESULTS)),
           "# worst |got - EXT| / (C eps s) over clouds, pairs and elements; the test's bound is %g" % mn.MARGIN,
           "# C: C_ORACLE (open / in a box) in units of 2^-53 s, C_ORACLE32 in units of 2^-24 s for the f32_* families",
           "%-32s %-4s %-5s %9s %9s %7s" % ("family", "kind", "bound", "C open", "C box", "worst")]
  for (family, kind, boundary), ratio in sorted(pb.RESULTS.items()):
    f32 = family.startswith("f32_")
    c_open = mn.C_ORACLE32[kind, boundary] if f32 else mn.C_ORACLE[kind, boundary, False]
    c_box = "-" if f32 else "%.0f" % mn.C_ORACLE[kind, boundary, True]
    lines.append("%-32s %-4s %-5s %9.0f %9s %7.3f" % (family, kind, boundary, c_open, c_box, ratio))
  lines.append("# largest: %.3f" % max(pb.RESULTS.values()))
  text = "\n".join(lines) + "\n"
  if args.out:
    with open(args.out, "w") as fh:
      fh.write(text)
  print(text)
  return int(rc)


if __name__ == "__main__":
  sys.exit(main())
