"""Block extraction from the HIP kernel families and the element-wise comparison with the extended-precision restatement
(tests/_mobility_numpy.py) -- shared by tests/test_gpu_pair_blocks.py and tools/pair_blocks_report.py.

A family is a set of context options that pins one kernel (its `last_path` code is asserted after every launch) plus an
extraction mode: which entry point is fed the 3N unit vectors.  Every other column contributes exact zeros to a product,
so the column a unit vector extracts IS the kernel's block, with the kernel's own roundings and nothing else.

`last_path` codes: 0 one-sided sweep ("symmetric" = 0, "deterministic" = 1, a target sub-range or N < 128), 1 symmetric per
wave, 2 the ordered symmetric reduction ("deterministic" = 2), 3 workgroup-cooperative, 4 two target blobs per lane."""
import numpy as np

import _mobility_numpy as mn
from _mobility_numpy import A, ETA

EPS = {64: 2.0 ** -53, 32: 2.0 ** -24}
RESULTS = {}        # (family, kind, boundary) -> worst ratio seen, in units of C (tools/pair_blocks_report.py prints it)


class Family(object):
  def __init__(self, name, mode, options, path, boundaries=("none", "wall"), clouds=("open", "offset", "odd", "pow2"), kinds=mn.KINDS,
               precision=64, in_plane=False, target_range=None, chunks=None):
    self.name, self.mode, self.options, self.path = name, mode, dict(options), path
    self.boundaries, self.clouds, self.kinds = tuple(boundaries), tuple(clouds), tuple(kinds)
    self.precision, self.in_plane, self.target_range, self.chunks = precision, in_plane, target_range, chunks

  def cases(self):
    return [(self.name, b, c) for c in self.clouds for b in self.boundaries]


WAVE = {"sym_coop": 0, "sym_two_targets": 0}
COOP = {"sym_coop": 2}
TWO = {"sym_two_targets": 2}
ALL_B = ("none", "wall", "free")
OPEN = ("open", "offset")

FAMILIES = [
    # --- one-sided sweep (path 0) ---------------------------------------------------------------------------------------
    Family("sweep", "single", {"symmetric": 0}, 0, ALL_B),
    Family("sweep_deterministic1", "single", {"deterministic": 1}, 0, clouds=("open", "odd")),
    Family("sweep_chunks2", "single", {"symmetric": 0, "chunks": 2}, 0, clouds=("open", "pow2"), chunks=2),      # four tiles: two source chunks
    Family("sweep_target_range", "single", {}, 0, ALL_B, clouds=("open", "odd"), target_range=(61, 137)),
    Family("sweep_fused", "fused_kind", {"symmetric": 0}, 0, ALL_B, kinds=("tt", "tr")),
    Family("sweep_in_plane", "single", {"symmetric": 0}, 0, ("wall",), kinds=("tt", "tr"), in_plane=True),
    # --- sym_kernel and its variants ------------------------------------------------------------------------------------
    Family("sym_wave", "single", WAVE, 1),
    Family("sym_deterministic2", "single", {"deterministic": 2}, 2, ALL_B),
    Family("sym_coop", "single", COOP, 3),
    Family("sym_two_targets", "single", TWO, 4),          # sym2t_kernel; in a box symx2t_kernel<OpSingle, periodic>
    # --- the generic skeleton -------------------------------------------------------------------------------------------
    Family("symx_single_wave", "single", dict(WAVE, symx_single=1), 1),
    Family("symx_single_coop", "single", dict(COOP, symx_single=1), 3),
    Family("symx_in_plane_wave", "single", WAVE, 1, ("wall",), kinds=("tt", "tr"), in_plane=True),
    Family("symx_in_plane_coop", "single", COOP, 3, ("wall",), kinds=("tt", "tr"), in_plane=True),
    Family("symx_fused_kind_wave", "fused_kind", WAVE, 1, ALL_B, kinds=("tt", "tr")),
    Family("symx_fused_kind_two_targets", "fused_kind", TWO, 4, kinds=("tt", "tr")),
    Family("symx_fused_op_wave", "op_fused", WAVE, 1, ALL_B, kinds=("tt", "tr")),
    Family("symx_fused_op_coop", "op_fused", COOP, 3, kinds=("tt", "tr")),
    Family("symx_grand_wave", "op_grand", WAVE, 1, ALL_B),
    Family("symx_grand_coop", "op_grand", COOP, 3),
    Family("symx_grand_two_targets", "op_grand", TWO, 4),
    Family("symx_force_column_wave", "op_colf", WAVE, 1, ALL_B, kinds=("tt", "rt")),
    Family("symx_force_column_coop", "op_colf", COOP, 3, kinds=("tt", "rt")),
    Family("symx_force_column_two_targets", "op_colf", TWO, 4, kinds=("tt", "rt")),
    Family("symx_multi4_wave", "multi4", WAVE, 1),
    Family("symx_multi4_coop", "multi4", COOP, 3),
    Family("symx_multi2_two_targets", "multi2", TWO, 4),
    Family("sym2_two_vectors", "matvec2", WAVE, 1, kinds=("tt",)),
    Family("symx_two_vectors_wave", "matvec2", dict(WAVE, symx_single=1), 1, kinds=("tt",)),
    Family("symx_two_vectors_coop", "matvec2", dict(COOP, symx_single=1), 3, kinds=("tt",)),
    Family("symx_two_vectors_two_targets", "matvec2", dict(TWO, symx_single=1), 4, kinds=("tt",)),
    # --- free surface: tt has a cooperative instance, the rotational kinds the per-wave kernel only -------------------------
    Family("free_wave", "single", WAVE, 1, ("free",)),
    Family("free_tt_coop", "single", COOP, 3, ("free",), kinds=("tt",)),
    # --- dense builders ---------------------------------------------------------------------------------------------------
    Family("dense_builder", "dense", {}, None, ALL_B, clouds=OPEN, kinds=("tt",)),
    # --- precision 32: per-wave fp32 twins, open boundaries -----------------------------------------------------------------
    Family("f32_single", "single", {"precision": 32}, 1, clouds=OPEN, precision=32),
    Family("f32_free_tt", "single", {"precision": 32}, 1, ("free",), clouds=OPEN, kinds=("tt",), precision=32),
    Family("f32_in_plane", "single", {"precision": 32}, 1, ("wall",), clouds=OPEN, kinds=("tt", "tr"), precision=32, in_plane=True),
    Family("f32_fused_op", "op_fused", {"precision": 32}, 1, clouds=OPEN, kinds=("tt", "tr"), precision=32),
    Family("f32_grand", "op_grand", {"precision": 32}, 1, clouds=OPEN, precision=32),
    Family("f32_force_column", "op_colf", {"precision": 32}, 1, clouds=OPEN, kinds=("tt", "rt"), precision=32),
    Family("f32_multi4", "multi4", {"precision": 32}, 1, clouds=OPEN, precision=32),
    Family("f32_two_vectors", "matvec2", {"precision": 32}, 1, clouds=OPEN, kinds=("tt",), precision=32),
]
BY_NAME = {f.name: f for f in FAMILIES}
assert len(BY_NAME) == len(FAMILIES)


def all_cases():
  return [c for f in FAMILIES for c in f.cases()]


def bound(kind, boundary, periodic, precision):
  """MARGIN C eps, per unit of scale."""
  c = mn.C_ORACLE[kind, boundary, bool(periodic)] if precision == 64 else mn.C_ORACLE32[kind, boundary]
  return mn.MARGIN * c * EPS[precision]


def open_context(Ctx, fam, boundary, r, L):
  import torch
  ctx = Ctx(0)
  for key, val in fam.options.items():
    ctx.set_option(key, val)
  if boundary == "free":
    ctx.set_option("free_surface_rotation", 1)
  wall = {"none": False, "wall": True, "free": "free_surface"}[boundary]
  ctx.set_positions(torch.as_tensor(np.ascontiguousarray(r).reshape(-1), device="cuda"), A, L, wall)
  if fam.target_range:
    ctx.set_target_range(*fam.target_range)
  return ctx


def extract(ctx, fam, n, eye):
  """{kind: (3 n_targets, 3N) numpy array} of the family's kernel, column by column."""
  import torch
  n3 = 3 * n
  nt3 = 3 * ctx.n_targets
  zero = torch.zeros(n3, dtype=torch.float64, device="cuda")

  def launched():
    path = ctx.get_option("last_path")
    assert path == fam.path, "%s: last_path %d, expected %d" % (fam.name, path, fam.path)
    if fam.chunks is not None:
      assert ctx.last_launch()["chunks"] == fam.chunks, ctx.last_launch()

  out = {k: torch.empty((n3, nt3), dtype=torch.float64, device="cuda") for k in fam.kinds}
  mode = fam.mode
  if mode == "single":
    for kind in fam.kinds:
      for k in range(n3):
        ctx.matvec_device(kind, eye[k], ETA, in_plane=fam.in_plane, out=out[kind][k])
        launched()
  elif mode == "fused_kind":      # M_tt f + M_tr tau in one pass: a unit force reads off tt, a unit torque tr
    for k in range(n3):
      ctx.matvec_device("tt_tr", eye[k], ETA, vec2=zero, out=out["tt"][k]); launched()
      ctx.matvec_device("tt_tr", zero, ETA, vec2=eye[k], out=out["tr"][k]); launched()
  elif mode == "op_fused":
    for k in range(n3):
      ctx.matvec_op_device("velocity_from_force_torque", (eye[k], zero), ETA, outs=(out["tt"][k],)); launched()
      ctx.matvec_op_device("velocity_from_force_torque", (zero, eye[k]), ETA, outs=(out["tr"][k],)); launched()
  elif mode == "op_grand":
    for k in range(n3):
      ctx.matvec_op_device("grand", (eye[k], zero), ETA, outs=(out["tt"][k], out["rt"][k])); launched()
      ctx.matvec_op_device("grand", (zero, eye[k]), ETA, outs=(out["tr"][k], out["rr"][k])); launched()
  elif mode == "op_colf":
    for k in range(n3):
      ctx.matvec_op_device("force_column", (eye[k],), ETA, outs=(out["tt"][k], out["rt"][k])); launched()
  elif mode in ("multi4", "multi2"):
    w = int(mode[-1])
    assert n3 % w == 0
    for kind in fam.kinds:
      for k in range(0, n3, w):
        ctx.matvec_op_device(kind + "_multi", [eye[k + q] for q in range(w)], ETA, outs=[out[kind][k + q] for q in range(w)]); launched()
  elif mode == "matvec2":
    for k in range(0, n3, 2):
      ctx.matvec2_device("tt", eye[k], eye[k + 1], ETA, out_a=out["tt"][k], out_b=out["tt"][k + 1]); launched()
  elif mode == "dense":
    first = torch.zeros(1, dtype=torch.int64, device="cuda")
    out["tt"] = ctx.body_mobility_dense_device(first, n, ETA)[0].t().contiguous()
  else:
    raise ValueError(mode)
  torch.cuda.synchronize()
  return {k: v.t().cpu().numpy() for k, v in out.items()}


def compare(label, kind, boundary, cloud_name, got_dense, precision=64, in_plane=False, rows=None):
  """Assert |got - EXT| <= MARGIN C eps s element by element; returns the worst ratio in units of C eps s."""
  r, L = mn.cloud(cloud_name)
  E, s = mn.reference(cloud_name, kind, boundary, in_plane)
  got = mn.from_dense(np.asarray(got_dense))
  if rows is not None:
    E, s = E[rows[0]:rows[1]], s[rows[0]:rows[1]]
  assert got.shape == E.shape, (got.shape, E.shape)
  assert np.all(np.isfinite(got)), "%s %s %s %s: non-finite block" % (label, kind, boundary, cloud_name)
  c = bound(kind, boundary, L is not None, precision) / mn.MARGIN
  ratio, i, j, p, q = mn.worst_ratio(got, E, s, c)
  i_abs = i + (rows[0] if rows is not None else 0)
  key = (label, kind, boundary)
  RESULTS[key] = max(RESULTS.get(key, 0.0), ratio)
  print("%-30s %s %-4s %-6s worst %.3f C at pair (%d, %d) element (%d, %d)" % (label, kind, boundary, cloud_name, ratio, i_abs, j, p, q))
  assert ratio <= mn.MARGIN, (
      "family %s kind %s boundary %s cloud %s: block (%d, %d) element (%d, %d) is off by %.1f C = %.1f units of %s s (bound %g C); "
      "got %.17g, extended precision %s; regime: %s" % (label, kind, boundary, cloud_name, i_abs, j, p, q, ratio, ratio * c / EPS[precision],
                                                            "2^-53" if precision == 64 else "2^-24", mn.MARGIN, got[i, j, p, q],
                                                            np.format_float_scientific(E[i, j, p, q], precision=20), mn.regime_of(r, A, i_abs, j, L)))
  return ratio


def run_case(Ctx, name, boundary, cloud_name, eye):
  fam = BY_NAME[name]
  r, L = mn.cloud(cloud_name)
  ctx = open_context(Ctx, fam, boundary, r, L)
  try:
    blocks = extract(ctx, fam, len(r), eye)
  finally:
    ctx.close()
  for kind in fam.kinds:
    compare(name, kind, boundary, cloud_name, blocks[kind], fam.precision, fam.in_plane, fam.target_range)
