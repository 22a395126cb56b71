#!/usr/bin/env python
"""Worst rounding error of the per-body rigid kernels and of the block product per quantity, from the GPU tests themselves.

Runs tests/test_gpu_rigid_kernels.py and tests/test_gpu_block_apply.py in this process (the same code, no launch beyond the
tests' own) and writes, per key of the yardstick table C of tests/_rigid_kernels_numpy.py: C (the fp64 numpy restatement's
worst fraction of the derived bound against long double, measured on the CPU; `nres` and the end-to-end keys in units of
2^-53 times their scale), the asserted bound (min(MARGIN C, 1) with a derived bound, MARGIN C without) and the worst
measured value on the device as a fraction of that bound; then the worst fraction per kernel.

  python tools/rigid_kernels_report.py [--out profiles/FILE.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kernel_of(key):
  if key[0] == "block":
    return "block_apply_kernel"
  if key[0].startswith("config"):
    return "rigid_config_kernel"
  if key[0].startswith("advance"):
    return "rigid_advance_kernel"
  return "rigid_pc_large_kernel" if key[-1] == "large" else "rigid_pc_kernel"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  import pytest
  rc = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_rigid_kernels.py"),
                    os.path.join(ROOT, "tests", "test_gpu_block_apply.py")])
  import torch
  import _rigid_kernels_numpy as rk
  lines = ["# tools/rigid_kernels_report.py on %s; pytest exit status %d; %d of %d keys measured" %
           (torch.cuda.get_device_name(0), int(rc), len(rk.RESULTS), len(rk.C)),
           "# C: worst fraction of the fp64 numpy restatement (CPU, against long double) of the derived bound; nres and e2e_* in",
           "#    units of 2^-53 scale (no derived bound).  bound: min(%g C, 1) resp. %g C.  device: worst measured / bound." % (rk.MARGIN, rk.MARGIN),
           "# advance: device sin / cos / sqrt accuracy ASSUMED %g u, %g u, %g u in the derived bound (no documented figure);" % (rk.E_TRIG, rk.E_TRIG, rk.E_SQRT),
           "#    the restatement's own error is C['advance_quat'] = %g of that bound" % rk.C[("advance_quat",)],
           "%-38s %10s %10s %8s" % ("key", "C", "bound", "device")]
  worst = {}
  for key in sorted(rk.C):
    got = rk.RESULTS.get(key)
    lines.append("%-38s %10.4g %10.4g %8s" % (" ".join(key), rk.C[key], rk.bound(key), "-" if got is None else "%.3f" % got))
    if got is not None:
      k = kernel_of(key)
      if got > worst.get(k, (-1.0, None))[0]:
        worst[k] = (got, key)
  lines.append("# worst fraction of its bound per kernel")
  for k in sorted(worst):
    lines.append("%-24s %.3f   (%s)" % (k, worst[k][0], " ".join(worst[k][1])))
  text = "\n".join(lines) + "\n"
  if args.out:
    with open(args.out, "w") as fh:
      fh.write(text)
  print(text)
  return int(rc)


if __name__ == "__main__":
  sys.exit(main())
