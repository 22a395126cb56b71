#!/usr/bin/env python
"""Worst per-blob error of the pair laws per (family, law, boundary), from the GPU test itself.

Runs tests/test_gpu_pair_forces.py in this process (the same code, no launch beyond the test's own) and writes the ratios the
test recorded: (|got - EXT| - floor)+ / (C eps S) maximised over the designed clouds, the blobs and the three components (the
energies: over the slab-pair bands and the ladder), with the extended-precision reference, the per-blob scale S, the floor
and the yardstick C of tests/_pair_forces_numpy.py (eps = 2^-53; for the `f32_*` families C32 and 2^-24).  The test's bound is
MARGIN = 4 in these units.  The C values it prints are the stored ones; tests/test_pair_forces_host.py measures them.

  python tools/pair_forces_report.py [--out profiles/FILE.txt]
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
  rc = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_pair_forces.py")])
  import torch
  import _pair_forces_gpu as pg
  import _pair_forces_numpy as pf
  lines = ["# tools/pair_forces_report.py on %s; pytest exit status %d; %d (family, law, boundary) rows" %
           (torch.cuda.get_device_name(0), int(rc), len(pg.RESULTS)),
           "# worst (|got - EXT| - floor)+ / (C eps S) over clouds, blobs and components; the test's bound is %g" % pf.MARGIN,
           "# C (CPU-measured, tests/test_pair_forces_host.py; units of 2^-53 S, open / in a box): " +
           ", ".join("%s %g / %g" % (k, pf.C[k, False], pf.C[k, True]) for k in sorted(set(k for k, _ in pf.C))),
           "# C32 (units of 2^-24 S, open): " + ", ".join("%s %g" % kv for kv in sorted(pf.C32.items())),
           "# as measured on the CPU (fp64 oracle / float32 restatement against EXT): " +
           ", ".join("%s %s %.3f" % (k[0], {False: "open", True: "box", 32: "fp32"}[k[1]], v) for k, v in sorted(pf.C_MEASURED.items(), key=str)),
           "%-30s %-8s %-5s %6s %9s" % ("family", "law", "bound", "C", "worst")]
  for (family, law, boundary), ratio in sorted(pg.RESULTS.items()):
    fam = pg.BY_NAME.get(family)
    if fam is not None and fam.bound_precision == 32:
      c = pf.C32[law]
    else:
      c = pf.C["yukawa_energy" if (fam is None and law == "yukawa" and not family.startswith("host_wrapper")) else law, boundary == "box"]
    lines.append("%-30s %-8s %-5s %6g %9.3f" % (family, law, boundary, c, ratio))
  if pg.RESULTS:
    lines.append("# largest: %.3f" % max(pg.RESULTS.values()))
  text = "\n".join(lines) + "\n"
  if args.out:
    with open(args.out, "w") as fh:
      fh.write(text)
  print(text)
  return int(rc)


if __name__ == "__main__":
  sys.exit(main())
