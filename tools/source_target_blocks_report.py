#!/usr/bin/env python
"""Worst element-wise error of the source -> target operators per kernel family, from the GPU test itself.

Runs tests/test_gpu_source_target_blocks.py in this process (the same code, no launch beyond the test's own) and writes
the ratios the test recorded: |got - EXT| / (C eps s) maximised over the designed clouds, the pairs and the elements, with
the extended-precision reference, the scales and the yardsticks of tests/_source_target_numpy.py (C_ST / C_P / C_DL and
eps = 2^-53; C_ST32 and 2^-24 for radii_f32; C_*_SUM per target for edge_products).  The test's bound is MARGIN = 4 in
these units; the tracer_no_slip rows are |u_t| in units of C eps sum_s s_ts |f_s| against a bound of 1.

  python tools/source_target_blocks_report.py [--out profiles/FILE.txt] [-k EXPR]
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
  ap.add_argument("-k", default=None, help="pytest -k expression")
  args = ap.parse_args()
  import pytest
  argv = ["-m", "gpu", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_source_target_blocks.py")]
  if args.k:
    argv += ["-k", args.k]
  rc = pytest.main(argv)
  import torch
  import _source_target_blocks_gpu as sb
  import _source_target_numpy as sn
  lines = ["# tools/source_target_blocks_report.py on %s; pytest exit status %d; %d (family, operator) rows" %
           (torch.cuda.get_device_name(0), int(rc), len(sb.RESULTS)),
           "# worst |got - EXT| / (C eps s) over clouds, pairs and elements; the test's bound is %g" % sn.MARGIN,
           "# operators: st0 / st1 / st2 radii mobility unbounded / wall / free surface, p_0 / p_1 pressure without / with the wall,",
           "# dl_free / dl_wall / dl_rpy double layer",
           "%-44s %-10s %7s" % ("family", "operator", "worst")]
  for (family, op), ratio in sorted(sb.RESULTS.items()):
    lines.append("%-44s %-10s %7.3f" % (family, op, ratio))
  if sb.RESULTS:
    lines.append("# largest: %.3f" % max(sb.RESULTS.values()))
  text = "\n".join(lines) + "\n"
  if args.out:
    with open(args.out, "w") as fh:
      fh.write(text)
  print(text)
  return int(rc)


if __name__ == "__main__":
  sys.exit(main())
