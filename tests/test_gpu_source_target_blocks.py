"""Every block of the source -> target operators -- the translation mobility with per-blob radii (pair_st, st_coeffs /
st_apply / OpRadiiTT, OpRadiiTT32), the Stokeslet pressure, the Stokes double layer and its RPY form (aux_pair) --
element by element against the extended-precision restatement of tests/_source_target_numpy.py:

    |got - EXT| <= MARGIN * C * eps * s_ts          (MARGIN = 4)

with the scales and the yardsticks C_ST / C_ST32 / C_P / C_DL of that module (the fp64 oracle's own worst error in the same
units, measured on the CPU by tests/test_source_target_blocks_host.py), on the designed clouds whose regime counts are
asserted there: pairs exactly on and 4e-12 a off the switches r = a_t + a_s and r = |a_t - a_s|, concentric blobs, radius
ratios 1e-3 and 1e3, tracer targets, a 64-target tile with one / every / no lane overlapping a source, clamped and damped
blobs on either side, overlapping images below a free surface, two boxes; for the aux operators the 1e-14 skip, z -> 0 and
the coincident pair of the pressure (non-finite exactly where the oracle is).  Whole products at the edge shapes of the
512-record tile, the 64-target workgroup and forced chunk edges are held per target to

    |Delta_t| <= MARGIN * C_SUM * eps * sum_s s_ts |f_s|_max

repeated calls bit for bit, different chunk counts within the same bound, one-hot sources on every record slot and chunk
edge.  The families and the kernel each one pins are listed in tests/_source_target_blocks_gpu.py;
tools/source_target_blocks_report.py runs this file and writes the worst ratio per family."""
import numpy as np
import pytest

import _source_target_blocks_gpu as sb
import _source_target_numpy as sn
from _source_target_numpy import ETA, EXT, MARGIN

pytestmark = pytest.mark.gpu

AUX_OPS = [("p", 0), ("p", 1), ("dl", "free"), ("dl", "wall"), ("dl", "rpy")]
OPS = [("st", m) for m in sn.MODES] + AUX_OPS
FORCED = (0, 1, 2, 64)          # "chunks" of the block extraction: automatic, 1, 2, and a count at the number of sources
_id = lambda v: "_".join(str(x) for x in v) if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.fixture(scope="module")
def Ctx():
  from rigidmultiblobswall_amd import MobilityContext
  return MobilityContext


def _c_aux(op):
  return sn.C_P[op[1]] if op[0] == "p" else sn.C_DL[op[1]]


def _c_sum(op):
  return {"st": sn.C_ST_SUM, "p": sn.C_P_SUM, "dl": sn.C_DL_SUM}[op[0]][op[1]]


def test_the_reference_is_extended_precision_and_the_clouds_hold_every_class():
  assert sn.mn.LONG_DOUBLE, "np.longdouble has no 64-bit mantissa here: fp64 would be compared with fp64"
  for name in sn.ST_CLOUDS:
    c = sn.cloud(name)                 # asserts the classes of every mode and the absence of ties
    assert len(c[0]) == 64 and len(c[2]) % 64 and len(c[2]) > 3 * 64
  for name in ("open", "odd", "pow2"):
    assert len(sn.same_cloud(name)[0]) == 200
  for name in sn.AUX_CLOUDS:
    sn.aux(name)


# ---------------------------------------------------------------------------------------------------------------------
# one-sided sweep of the radii mobility (pair_st), sources != targets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sn.MODES)
@pytest.mark.parametrize("name", sorted(sn.ST_CLOUDS))
def test_st_blocks_host_wrappers(name, mode):
  src, rs, tgt, rt, L = sn.cloud(name)
  E, s = sn.st_reference(name, mode)
  sb.compare("st_host_wrapper", "st%d" % mode, sb.extract_st_host(mode, src, rs, tgt, rt, L), E, s, sn.C_ST[mode, L is not None], note=name)


@pytest.mark.parametrize("forced", FORCED)
@pytest.mark.parametrize("mode", sn.MODES)
@pytest.mark.parametrize("name", sorted(sn.ST_CLOUDS))
def test_st_blocks_device_entry(Ctx, name, mode, forced):
  src, rs, tgt, rt, L = sn.cloud(name)
  E, s = sn.st_reference(name, mode)
  d = sb.Device(Ctx, {"chunks": forced})
  try:
    # 64 sources: one chunk whatever is forced (a chunk holds at least 128 sources)
    got = sb.extract_st_device(d, mode, src, rs, tgt, rt, L, path=0, chunks=1)
  finally:
    d.close()
  sb.compare("st_sweep_chunks%d" % forced, "st%d" % mode, got, E, s, sn.C_ST[mode, L is not None], note=name)


# ---------------------------------------------------------------------------------------------------------------------
# sources == targets, N = 200: st_coeffs / st_apply / OpRadiiTT, OpRadiiTT32, and what falls back to pair_st
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name,mode", sb.same_cases(), ids=_id)
def test_same_blocks_device_entry(Ctx, family, name, mode):
  """The full (N, N) block matrix: the reversed block [s, t] (gamma <-> delta, the flipped sign) next to [t, s]."""
  options, path, precision, _, _ = sb.SAME_FAMILIES[family]
  r, rad, L = sn.same_cloud(name)
  E, s = sn.same_reference(name, mode)
  d = sb.Device(Ctx, options)
  try:
    got = sb.extract_st_device(d, mode, r, rad, r, rad, L, path=path, chunks=(None if path == 0 else 0), same=True)
  finally:
    d.close()
  c = sn.C_ST[mode, L is not None] if precision == 64 else sn.C_ST32[mode]
  sb.compare(family, "st%d" % mode, got, E, s, c, precision, note=name)


@pytest.mark.parametrize("mode", (0, 1))
def test_same_blocks_host_wrapper(mode):
  r, rad, L = sn.same_cloud("open")
  E, s = sn.same_reference("open", mode)
  sb.compare("radii_host_wrapper", "st%d" % mode, sb.extract_st_host(mode, r, rad, r, rad, None, same=True), E, s, sn.C_ST[mode, False], note="open")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("n", (127, 128, 129))
def test_same_blocks_at_the_symmetric_threshold(Ctx, n, mode):
  """N = 127 takes the one-sided sweep, 128 and 129 must not."""
  r, rad, _ = sn.same_cloud("open")
  r, rad = r[:n], rad[:n]
  E, s = sn.st_blocks(mode, r, r, rad, rad, ETA), sn.st_scale(mode, r, r, rad, rad, ETA)
  d = sb.Device(Ctx)
  try:
    d.st(mode, sb.dev(r), sb.dev(rad), sb.dev(r), sb.dev(rad), sb.dev(np.zeros(3 * n)), None, sb.dev(np.zeros(3 * n)))     # distinct pointers: the sweep
    d.launched(0)
    import torch
    sd, rd, out = sb.dev(r), sb.dev(rad), torch.empty(3 * n, dtype=torch.float64, device="cuda")
    d.st(mode, sd, rd, sd, rd, sb.dev(np.zeros(3 * n)), None, out)
    path = d.ctx.get_option("last_path")
    assert (path == 0) == (n < 128), (n, path)
    got = sb.extract_st_device(d, mode, r, rad, r, rad, None, path=path, same=True)
  finally:
    d.close()
  sb.compare("radii_threshold_n%d" % n, "st%d" % mode, got, E, s, sn.C_ST[mode, False], note="path %d" % path)


# ---------------------------------------------------------------------------------------------------------------------
# pressure, double layer, RPY double layer (aux_pair)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", AUX_OPS, ids=_id)
@pytest.mark.parametrize("name", sorted(sn.AUX_CLOUDS))
def test_aux_blocks_host_wrappers(name, op):
  src, nrm, w, tgt = sn.aux(name)
  E, s = sn.pressure_reference(name, op[1]) if op[0] == "p" else sn.dl_reference(name, op[1])
  with np.errstate(all="ignore"):
    got = sb.extract_aux_host(op, src, nrm, w, tgt)
  sb.compare("aux_host_wrapper", _id(op), got, E, s, _c_aux(op), one_hot_rows=op[0] == "p", note=name)


@pytest.mark.parametrize("forced", FORCED)
@pytest.mark.parametrize("op", AUX_OPS, ids=_id)
@pytest.mark.parametrize("name", sorted(sn.AUX_CLOUDS))
def test_aux_blocks_device_entry(Ctx, name, op, forced):
  src, nrm, w, tgt = sn.aux(name)
  E, s = sn.pressure_reference(name, op[1]) if op[0] == "p" else sn.dl_reference(name, op[1])
  d = sb.Device(Ctx, {"chunks": forced})
  try:
    got = sb.extract_aux_device(d, op, src, nrm, w, tgt, chunks=1)
  finally:
    d.close()
  sb.compare("aux_sweep_chunks%d" % forced, _id(op), got, E, s, _c_aux(op), one_hot_rows=op[0] == "p", note=name)


# ---------------------------------------------------------------------------------------------------------------------
# whole products at the edge shapes
# ---------------------------------------------------------------------------------------------------------------------
def _product(d, op, e, vec, out):
  if op[0] == "st":
    d.st(op[1], e["src_d"], e["rs_d"], e["tgt_d"], e["rt_d"], vec, None, out)
  elif op[0] == "p":
    d.pressure(op[1], e["src_d"], e["tgt_d"], vec, out)
  else:
    d.dl(op[1], e["src_d"], e["tgt_d"], e["nrm_d"], vec, e["w_d"], out)


@pytest.mark.parametrize("op", OPS, ids=_id)
@pytest.mark.parametrize("ns,nt", sn.EDGE_SHAPES)
def test_whole_products_at_edge_shapes(Ctx, ns, nt, op):
  import torch
  e = dict(sn.edge_problem(ns, nt))
  for k in ("src", "rs", "tgt", "rt", "nrm", "w"):
    e[k + "_d"] = sb.dev(e[k])
  vec = e["v"] if op[0] == "dl" else e["f"]
  u, row = sn.edge_reference(op, ns, nt)
  width = 1 if op[0] == "p" else 3
  u, eps = u.reshape(nt, width), sb.EPS[64]
  bound = (MARGIN * _c_sum(op) * eps * row)[:, None]
  # one source alone: the product is a block applied to a vector, |Delta_t| <= MARGIN C eps s_tj |f_j|_1
  B, s = sn.edge_blocks(op, ns, nt)
  if op[0] == "p":
    B = B[:, :, None, :]
  c1 = sn.C_ST[op[1], False] if op[0] == "st" else _c_aux(op)
  d = sb.Device(Ctx)
  results, worst, worst1 = {}, 0.0, 0.0
  try:
    for forced in sn.EDGE_CHUNKS:
      d.ctx.set_option("chunks", forced)
      chunks, length = sb.chunk_plan(ns, forced)
      runs = []
      for rep in range(2):
        out = torch.full((nt * width,), 7.0, dtype=torch.float64, device="cuda")
        _product(d, op, e, sb.dev(vec), out)
        d.launched(0, chunks)
        runs.append(out.cpu().numpy().reshape(nt, width))
      assert np.array_equal(runs[0], runs[1]), "not bit-identical run to run (chunks %d)" % forced
      err = np.abs(runs[0].astype(EXT) - u)
      worst = max(worst, float((err / bound * MARGIN).max()))
      assert np.all(np.isfinite(runs[0])) and np.all(err <= bound), (forced, float((err / bound * MARGIN).max()))
      results[forced] = runs[0]
      # one-hot sources: every record slot of interest and the first and last index of each chunk
      hot = {0, 511, 512, ns - 1} | {c * length for c in range(chunks)} | {min((c + 1) * length, ns) - 1 for c in range(chunks)}
      for j in sorted(k for k in hot if 0 <= k < ns):
        one = np.zeros_like(vec)
        one[j] = vec[j]
        out = torch.full((nt * width,), 7.0, dtype=torch.float64, device="cuda")
        _product(d, op, e, sb.dev(one), out)
        got = out.cpu().numpy().reshape(nt, width)
        ref = np.einsum("tpq,q->tp", B[:, j], vec[j].astype(EXT))
        b1 = (MARGIN * c1 * eps * s[:, j] * EXT(np.abs(vec[j]).sum()))[:, None]
        e1 = np.abs(got.astype(EXT) - ref)
        worst1 = max(worst1, float((e1 / b1 * MARGIN).max()))
        assert np.all(e1 <= b1), ("one-hot source %d, chunks %d" % (j, forced), float((e1 / b1 * MARGIN).max()))
    for forced in sn.EDGE_CHUNKS[1:]:
      assert np.all(np.abs(results[forced].astype(EXT) - results[1]) <= bound), "chunks %d against 1" % forced
  finally:
    d.close()
  sb.RESULTS["edge_products", _id(op)] = max(sb.RESULTS.get(("edge_products", _id(op)), 0.0), worst)
  sb.RESULTS["edge_one_hot", _id(op)] = max(sb.RESULTS.get(("edge_one_hot", _id(op)), 0.0), worst1)
  print("%-44s %-14s %-8s worst %.3f C_SUM, one-hot %.3f C" % ("edge_products", _id(op), "%dx%d" % (ns, nt), worst, worst1))


# ---------------------------------------------------------------------------------------------------------------------
# the no-slip property at tracers on the wall
# ---------------------------------------------------------------------------------------------------------------------
def test_no_slip_velocity_vanishes_at_tracers_on_the_wall(Ctx):
  """radius_target = 0, z_t = 0: the wall product is pure rounding, |u_t| <= C eps sum_s s_ts |f_s|_max (see the host test)."""
  import torch
  from rigidmultiblobswall_amd import mobility as mob
  src, rs, tgt, rt, f = sn.tracer_problem()
  s = sn.st_scale(1, src, tgt, rs, rt, ETA)
  row = (s * np.abs(f).max(axis=1).astype(EXT)[None, :]).sum(axis=1)[:, None]
  d = sb.Device(Ctx)
  try:
    out = torch.empty(3 * len(tgt), dtype=torch.float64, device="cuda")
    d.st(1, sb.dev(src), sb.dev(rs), sb.dev(tgt), sb.dev(rt), sb.dev(f), None, out)
    d.launched(0)
    u_dev = out.cpu().numpy().reshape(-1, 3)
  finally:
    d.close()
  u_host = mob.single_wall_mobility_trans_times_force_source_target_hip(src, tgt, f, rs, rt, ETA).reshape(-1, 3)
  for label, u in (("device", u_dev), ("host", u_host)):
    ratio = float((np.abs(u) / (sb.EPS[64] * row)).max())
    sb.RESULTS["tracer_no_slip_" + label, "st1"] = ratio / sn.C_ST[1, False]
    print("tracer no-slip, %s: worst |u_t| = %.2f units of 2^-53 sum_s s_ts |f_s| (C = %g)" % (label, ratio, sn.C_ST[1, False]))
    assert ratio <= sn.C_ST[1, False], (label, ratio)
  free = mob.no_wall_mobility_trans_times_force_source_target_hip(src, tgt, f, rs, rt, ETA)
  assert np.abs(free).max() > 1e-3
