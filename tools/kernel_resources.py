#!/usr/bin/env python
"""Per-kernel resources of the one-sided translation units, read off the gfx950 assembly of a source tree: VGPRs, SGPRs,
scratch, static LDS, code bytes, and for the sweep kernels the pair-loop instruction mix of isa_stats.kernel_loop_stats
(VALU / fp64 VALU / flops per lane / LDS instructions per pair).  The chunk plan of a one-sided sweep follows from its
residency, so a change that moves an instance across a register or LDS boundary changes results in the last bits.

  python tools/kernel_resources.py                  this tree
  python tools/kernel_resources.py OTHER_TREE       OTHER_TREE | this tree, side by side, differing rows marked
"""
import os
import re
import subprocess
import sys

import isa_stats

UNITS = ("rmb_sweep.hip", "rmb_laplace.hip")
INFO = re.compile(r"^(_Z\w+):.*?; codeLenInByte = (\d+).*?; TotalNumSgprs: (\d+)\n; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?"
                  r"; LDSByteSize: (\d+)", re.S | re.M)


def resident(vgpr, lds):
  """Workgroups of 4 waves per CU: 512 VGPRs per SIMD lane in blocks of 8, 160 KiB LDS, the launchers' cap of 8."""
  return min(8, 512 // (8 * ((vgpr + 7) // 8)), (160 * 1024) // lds if lds else 8)


def table(root):
  rows = {}
  for unit in UNITS:
    asm = subprocess.run([isa_stats.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-S",
                          "--cuda-device-only", "-o", "-", os.path.join(root, "rigidmultiblobswall_amd", "csrc", unit)],
                         check=True, capture_output=True, text=True).stdout
    for m in INFO.finditer(asm):
      name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
      name = re.sub(r"\(.*", "", name).replace("void ", "")
      code, sgpr, vgpr, scratch, lds = (int(g) for g in m.groups()[1:])
      row = "vgpr %3d sgpr %3d scratch %d lds %5d res %d code %4d" % (vgpr, sgpr, scratch, lds, resident(vgpr, lds), code)
      if "sweep_kernel" in name:
        st = isa_stats.kernel_loop_stats(asm, m.group(1))
        row += "  pair loop %3d / %3d / %3d / %d" % (st["valu_per_step"], st["f64_valu_per_step"], st["flops_per_lane_step"],
                                                    st["lds_per_step"])
      rows[name] = row
  return rows


if __name__ == "__main__":
  here = table(isa_stats.ROOT)
  other = table(sys.argv[1]) if len(sys.argv) > 1 else None
  for name in sorted(here):
    if other is None:
      print("%-44s %s" % (name, here[name]))
    else:
      print("%-44s %-88s | %s%s" % (name, other.get(name, "-"), here[name], "" if other.get(name) == here[name] else "   *"))
