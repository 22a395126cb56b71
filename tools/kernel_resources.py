#!/usr/bin/env python
"""Per-kernel resources of the one-sided translation units, read off the gfx950 assembly of a source tree: VGPRs, SGPRs,
scratch, static LDS, code bytes, and for the sweep kernels the pair-loop instruction mix of isa_stats.kernel_loop_stats
(VALU / fp64 VALU / flops per lane / LDS instructions per pair).  The chunk plan of a one-sided sweep follows from its
residency, so a change that moves an instance across a register or LDS boundary changes results in the last bits.

  python tools/kernel_resources.py                  this tree
  python tools/kernel_resources.py OTHER_TREE       OTHER_TREE | this tree, side by side, differing rows marked
  python tools/kernel_resources.py --potential      potential_kernel next to sym_force_kernel, every pair loop of each
  python tools/kernel_resources.py --moves          body_delta_kernel / move_finish_kernel (rmb_mcmc_moves.hip), every pair loop
  python tools/kernel_resources.py --pair-hist      pair_hist_kernel (rmb_pair_hist.hip) next to potential_kernel; `lds` is the static part
                                                    (the staging slabs), the counters add 4 n_bins bytes of dynamic LDS
  python tools/kernel_resources.py --msd             msd_record_kernel / msd_sweep_kernel / msd_finish_kernel (rmb_msd.hip); the sweep's LDS is
                                                    dynamic: 56 (origin_chunk + 63) bytes, at least 10 752
  python tools/kernel_resources.py --scattering      scat_modes_kernel / scat_record_kernel / scat_sweep_kernel and their finishing launches
                                                    (rmb_scattering.hip); the lag sweep's LDS is dynamic: 16 NC (256 + 63) bytes at most
  python tools/kernel_resources.py --van-hove        van_hove_distinct_kernel / van_hove_self_kernel / van_hove_moments_finish_kernel
                                                    (rmb_van_hove.hip) next to pair_hist_kernel; `lds` is the static part, the counters add
                                                    4 n_bins (distinct) or 4 lags_per_tile n_bins <= 32 768 (self) bytes of dynamic LDS
  python tools/kernel_resources.py --bond-order      bond_order_kernel / bond_order_finalize_kernel / pair_field_kernel (rmb_bond_order.hip) next to
                                                    pair_hist_kernel; `lds` is the static part, pair_field_kernel's accumulators add 12 n_bins
                                                    <= 49 152 bytes of dynamic LDS
  python tools/kernel_resources.py --hydro-function  hydro_coef_kernel / hydro_self_kernel / hydro_function_kernel / hydro_finish_kernel (rmb_hydro_function.hip)
  python tools/kernel_resources.py --clusters        cluster_init_kernel / cluster_kernel / cluster_finish_kernel (rmb_clusters.hip) next to
                                                    pair_hist_kernel; no dynamic LDS; scratch must be 0 (a spill in the union-find's loops
                                                    would be the first thing to look at)
  python tools/kernel_resources.py --sym OTHER_TREE every kernel of the units that see pair_blocks.h / sym_kernels.h (symmetric families, fp32
                                                    twins, one-sided sweeps): OTHER_TREE | this tree, resources and every pair loop, differing
                                                    rows marked and counted -- what a change to the shared pair arithmetic touched
  python tools/kernel_resources.py --rigid [TREE]   the dense per-body blocks and the finishing launches of the rigid-body
                                                    operator / Lanczos step (rmb_rigid.hip), every boundary instance
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


RIGID_UNITS = ("rmb_sweep.hip", "rmb_rigid.hip")
RIGID_KERNELS = ("body_dense_tt_kernel", "rigid_operator_finish_kernel", "lanczos_finish_kernel", "plain_finish_kernel")


def table(root, units=UNITS, only=None):
  rows = {}
  for unit in units:
    asm = subprocess.run([isa_stats.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-S",
                          "--cuda-device-only", "-o", "-", os.path.join(root, "rigidmultiblobswall_amd", "csrc", unit)],
                         check=True, capture_output=True, text=True).stdout
    for m in INFO.finditer(asm):
      if only is not None and not any(k in m.group(1) for k in only):
        continue
      name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
      name = name.replace("(anonymous namespace)::", "")
      name = re.sub(r"\(.*", "", name).replace("void ", "")
      code, sgpr, vgpr, scratch, lds = (int(g) for g in m.groups()[1:])
      row = "vgpr %3d sgpr %3d scratch %d lds %5d res %d code %4d" % (vgpr, sgpr, scratch, lds, resident(vgpr, lds), code)
      if "sweep_kernel" in name:
        st = isa_stats.kernel_loop_stats(asm, m.group(1))
        row += "  pair loop %3d / %3d / %3d / %d" % (st["valu_per_step"], st["f64_valu_per_step"], st["flops_per_lane_step"],
                                                    st["lds_per_step"])
      rows[name] = row
  return rows


def pair_loops(asm, mangled, floor=30):
  """(header, VALU, fp64 VALU, LDS instructions) of EVERY inner loop of a kernel with at least `floor` VALU instructions:
  a kernel with a plain and a guarded pair loop (potential_kernel) has two, isa_stats.kernel_loop_stats reports the larger."""
  lines = asm.split("\n")
  start = next(i for i, l in enumerate(lines) if l.startswith(mangled) and ":" in l)
  end = start
  while "s_endpgm" not in lines[end]:
    end += 1
  blocks, cur = [], None
  for l in lines[start:end]:
    m = re.match(r"^\.(LBB\d+_\d+):(.*)$", l)
    if m:
      cur = [m.group(1), m.group(2), []]
      blocks.append(cur)
    elif cur is not None and re.match(r"^\s+;", l):
      cur[1] += " " + l.strip()
    elif cur is not None:
      m = re.match(r"^\s+([a-z_0-9]+)", l)
      if m:
        cur[2].append(m.group(1))
  out = []
  for label, ann, _ in blocks:
    if "Inner Loop Header" not in ann:
      continue
    ops = [o for b in blocks if b[0] == label or re.search(r"in Loop: Header=%s\b" % label[1:], b[1]) for o in b[2]]
    valu = [o for o in ops if o.startswith("v_")]
    if len(valu) >= floor:
      out.append((label, len(valu), sum("f64" in o for o in valu), sum(o.startswith("ds_") for o in ops)))
  return out


POTENTIAL_KERNELS = (("rmb_potential.hip", "potential_kernel"), ("rmb_sym.hip", "sym_force_kernel"))
PAIR_HIST_KERNELS = (("rmb_pair_hist.hip", "pair_hist_kernel"), ("rmb_potential.hip", "potential_kernel"))
MSD_KERNELS = (("rmb_msd.hip", "msd_"),)
SCATTERING_KERNELS = (("rmb_scattering.hip", "scat_"),)
VAN_HOVE_KERNELS = (("rmb_van_hove.hip", "van_hove_"), ("rmb_pair_hist.hip", "pair_hist_kernel"))
BOND_ORDER_KERNELS = (("rmb_bond_order.hip", "bond_order_"), ("rmb_bond_order.hip", "pair_field_kernel"), ("rmb_pair_hist.hip", "pair_hist_kernel"))
CLUSTER_KERNELS = (("rmb_clusters.hip", "cluster_"), ("rmb_pair_hist.hip", "pair_hist_kernel"))
HYDRO_FUNCTION_KERNELS = (("rmb_hydro_function.hip", "hydro_"),)
MOVE_KERNELS = (("rmb_mcmc_moves.hip", "body_delta_kernel"), ("rmb_mcmc_moves.hip", "move_finish_kernel"))


def potential_table(root, kernels=POTENTIAL_KERNELS):
  """potential_kernel (rmb_potential.hip) next to sym_force_kernel (rmb_sym.hip), or the kernels of the single-body moves:
  resources and every pair loop."""
  for unit, pattern in kernels:
    asm = subprocess.run([isa_stats.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-S",
                          "--cuda-device-only", "-o", "-", os.path.join(root, "rigidmultiblobswall_amd", "csrc", unit)],
                         check=True, capture_output=True, text=True).stdout
    for m in INFO.finditer(asm):
      if pattern not in m.group(1):
        continue
      name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
      name = re.sub(r"\(.*", "", name).replace("void ", "")
      code, sgpr, vgpr, scratch, lds = (int(g) for g in m.groups()[1:])
      loops = "  ".join("loop %d VALU / %d fp64 / %d LDS" % l[1:] for l in pair_loops(asm, m.group(1)))
      print("%-44s vgpr %3d sgpr %3d scratch %d lds %5d res %d code %4d  %s" % (name, vgpr, sgpr, scratch, lds, resident(vgpr, lds), code, loops))


SYM_UNITS = ("rmb_sym.hip", "rmb_symx2t.hip", "rmb_symx2t_per.hip", "rmb_symx_coop.hip", "rmb_sym32.hip", "rmb_sweep.hip")


def sym_table(root):
  """name -> resources + every pair loop, for every kernel of SYM_UNITS (units compiled in parallel)."""
  from concurrent.futures import ThreadPoolExecutor

  def one(unit):
    return subprocess.run([isa_stats.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-S",
                           "--cuda-device-only", "-o", "-", os.path.join(root, "rigidmultiblobswall_amd", "csrc", unit)],
                          check=True, capture_output=True, text=True).stdout
  with ThreadPoolExecutor(max_workers=len(SYM_UNITS)) as pool:
    asms = list(pool.map(one, SYM_UNITS))
  rows = {}
  for asm in asms:
    found = list(INFO.finditer(asm))
    names = subprocess.run(["c++filt"], input="\n".join(m.group(1) for m in found), capture_output=True, text=True).stdout.split("\n")
    for m, name in zip(found, names):
      name = re.sub(r"\)$", "", re.sub(r"\((rmb::)?\w+( const)?\)$", "", name.strip().replace("(anonymous namespace)::", "").replace("void ", "")))
      code, sgpr, vgpr, scratch, lds = (int(g) for g in m.groups()[1:])
      loops = " ".join("%d/%d/%d" % l[1:] for l in pair_loops(asm, m.group(1)))
      rows[name] = "vgpr %3d sgpr %3d scratch %3d lds %5d code %5d  loops %s" % (vgpr, sgpr, scratch, lds, code, loops)
  return rows


if __name__ == "__main__":
  if "--sym" in sys.argv:
    other, here = sym_table(sys.argv[sys.argv.index("--sym") + 1]), sym_table(isa_stats.ROOT)
    changed = [n for n in sorted(set(here) | set(other)) if here.get(n) != other.get(n)]
    for name in sorted(here):
      print("%-70s %-72s | %s%s" % (name[:70], other.get(name, "-"), here[name], "   *" if name in changed else ""))
    print("# %d kernels, %d differ (loops: VALU / fp64 VALU / LDS instructions of every inner loop with >= 30 VALU instructions)" %
          (len(here), len(changed)))
    for name in changed:
      print("#   differs: %s" % name)
    sys.exit(0)
  if "--potential" in sys.argv:
    potential_table(isa_stats.ROOT)
    sys.exit(0)
  if "--moves" in sys.argv:
    potential_table(isa_stats.ROOT, MOVE_KERNELS)
    sys.exit(0)
  if "--msd" in sys.argv:
    potential_table(isa_stats.ROOT, MSD_KERNELS)
    sys.exit(0)
  if "--scattering" in sys.argv:
    potential_table(isa_stats.ROOT, SCATTERING_KERNELS)
    sys.exit(0)
  if "--van-hove" in sys.argv:
    potential_table(isa_stats.ROOT, VAN_HOVE_KERNELS)
    sys.exit(0)
  if "--bond-order" in sys.argv:
    potential_table(isa_stats.ROOT, BOND_ORDER_KERNELS)
    sys.exit(0)
  if "--clusters" in sys.argv:
    potential_table(isa_stats.ROOT, CLUSTER_KERNELS)
    sys.exit(0)
  if "--hydro-function" in sys.argv:
    potential_table(isa_stats.ROOT, HYDRO_FUNCTION_KERNELS)
    sys.exit(0)
  if "--pair-hist" in sys.argv:
    potential_table(isa_stats.ROOT, PAIR_HIST_KERNELS)
    sys.exit(0)
  if "--rigid" in sys.argv:
    root = sys.argv[sys.argv.index("--rigid") + 1] if len(sys.argv) > sys.argv.index("--rigid") + 1 else isa_stats.ROOT
    for name, row in sorted(table(root, RIGID_UNITS, RIGID_KERNELS).items()):
      print("%-72s %s" % (name.replace("rmbi::", "").replace("rmb::", ""), row))
    sys.exit(0)
  here = table(isa_stats.ROOT)
  other = table(sys.argv[1]) if len(sys.argv) > 1 else None
  for name in sorted(here):
    if other is None:
      print("%-44s %s" % (name, here[name]))
    else:
      print("%-44s %-88s | %s%s" % (name, other.get(name, "-"), here[name], "" if other.get(name) == here[name] else "   *"))
