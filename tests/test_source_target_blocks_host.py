"""The extended-precision restatement of the source -> target operators (tests/_source_target_numpy.py) against everything
that pins it on the CPU -- the fp64 oracle block by block (one source at a time) and product by product, the reference's
golden vectors g4 / g11 -- the coverage counts of the designed clouds, and the yardsticks C_ST / C_ST32 / C_P / C_DL /
C_*_SUM that tests/test_gpu_source_target_blocks.py holds the HIP kernels to, measured here from the reference side alone.

Units: one rounding unit of a block element is 2^-53 s_ts (2^-24 s_ts in single precision) with the scales of
_source_target_numpy.  Two fp64 evaluations of the same formulas that are each within C of the exact value are within 2 C
of each other: that is the bound of the oracle comparisons."""
import os

import numpy as np
import pytest

import _source_target_numpy as sn
from _source_target_numpy import ETA, EXT
from conftest import GOLDEN, golden_files, load_golden, rel_err

EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24
ST_CASES = [(name, mode) for name in sorted(sn.ST_CLOUDS) for mode in sn.MODES]
AUX_OPS = [("p", 0), ("p", 1), ("dl", "free"), ("dl", "wall"), ("dl", "rpy")]
TOL_GOLDEN = 2e-14         # tests/test_oracle_golden.py TOL, tests/test_aux_operators.py TOL_ORACLE


def test_long_double_is_the_extended_format():
  assert sn.mn.LONG_DOUBLE and EXT is np.longdouble and np.finfo(np.longdouble).nmant >= 63


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", ST_CASES)
def test_st_cloud_holds_every_class(name, mode):
  c = sn.st_cloud(*sn.ST_CLOUDS[name])
  src, rs, tgt, rt, L = c
  assert len(src) == sn.N_SOURCES <= 64 and len(tgt) == sn.N_TARGETS and len(tgt) % 64 and len(tgt) > 3 * 64
  cov = sn.assert_st_coverage(mode, name, c)
  assert all(cov[k] >= 1 for k in sn.st_classes(mode, name)) and cov["ties"] == 0
  assert cov["tile_one_lane"] >= 1 and cov["tile_no_lane"] >= 1 and cov["tile_all_lanes"] >= 1
  if L is not None:
    assert (L[0] == 2.0 ** round(np.log2(L[0]))) == (name == "pow2") and (L[1] > 0) == (name == "pow2")


@pytest.mark.parametrize("name", ["open", "odd", "pow2"])
def test_same_cloud_holds_every_class(name):
  r, rad, L = sn.same_cloud(name)          # asserts the classes of both modes and the absence of ties
  assert r.shape == (200, 3) and np.all(rad > 0)
  assert (L is None) == (name == "open")


@pytest.mark.parametrize("name", sorted(sn.AUX_CLOUDS))
def test_aux_cloud_holds_every_class(name):
  c = sn.aux_cloud(sn.AUX_CLOUDS[name][0])
  assert len(c[0]) <= 64 and len(c[3]) == 200
  cov = sn.assert_aux_coverage(name, c)
  assert all(cov[k] >= 1 for k in sn.AUX_CLOUDS[name][1])


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 oracle in block form, once per process
# ---------------------------------------------------------------------------------------------------------------------
_oracle_cache = {}


def _oracle_st(oracle, name, mode):
  if ("st", name, mode) not in _oracle_cache:
    src, rs, tgt, rt, L = sn.cloud(name)
    _oracle_cache["st", name, mode] = sn.oracle_st_blocks(oracle, mode, src, tgt, rs, rt, ETA, L)
  return _oracle_cache["st", name, mode]


def _oracle_aux(oracle, name, op):
  if (name, op) not in _oracle_cache:
    src, nrm, w, tgt = sn.aux(name)
    _oracle_cache[name, op] = (sn.oracle_pressure_rows(oracle, op[1], src, tgt) if op[0] == "p" else
                               sn.oracle_dl_blocks(oracle, op[1], src, tgt, nrm, w))
  return _oracle_cache[name, op]


def _aux_restatement(name, op, dtype):
  src, nrm, w, tgt = sn.aux(name)
  return sn.pressure_rows(op[1], src, tgt, dtype) if op[0] == "p" else sn.dl_blocks(op[1], src, tgt, nrm, w, dtype=dtype)


def _aux_reference(name, op):
  return sn.pressure_reference(name, op[1]) if op[0] == "p" else sn.dl_reference(name, op[1])


def _c_aux(op):
  return sn.C_P[op[1]] if op[0] == "p" else sn.C_DL[op[1]]


# ---------------------------------------------------------------------------------------------------------------------
# 1. float64 restatement == the oracle, block by block and product by product
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", ST_CASES)
def test_float64_st_restatement_matches_oracle_blocks(oracle, name, mode):
  src, rs, tgt, rt, L = sn.cloud(name)
  got = sn.st_blocks(mode, src, tgt, rs, rt, ETA, L, dtype=np.float64)
  ref = _oracle_st(oracle, name, mode)
  E, s = sn.st_reference(name, mode)
  assert np.all(np.isfinite(E)) and np.all(np.isfinite(ref)) and np.all((s > 0) | (mode == 1))      # b = 0: scale and block vanish
  ratio, where = sn.worst(got, ref.astype(EXT), s, EPS64)
  print("%s mode %d: restatement fp64 vs oracle %.2f units at %s" % (name, mode, ratio, where))
  assert ratio <= 2 * sn.C_ST[mode, L is not None], (ratio, where)
  if mode == 1:          # z = 0 with a > 0: b = 0, the block is exactly zero on either side
    z0s, z0t = (src[:, 2] == 0) & (rs > 0), (tgt[:, 2] == 0) & (rt > 0)
    assert z0s.any() and z0t.any()
    for B in (got, ref, E):
      assert np.all(B[:, z0s] == 0) and np.all(B[z0t] == 0)


@pytest.mark.parametrize("name,mode", ST_CASES)
def test_float64_st_restatement_matches_oracle_products(oracle, name, mode):
  """Multi-source products, random forces.  Both sides sum 3 ns (x boxes) terms in different orders: a coarse bound
  (2 C + 12 ns boxes) units of sum_s s_ts |f_s|_1 that still sees a wrong image, sign or box (those are O(1))."""
  src, rs, tgt, rt, L = sn.cloud(name)
  f = np.random.RandomState(11).randn(len(src), 3)
  got = np.einsum("tspq,sq->tp", sn.st_blocks(mode, src, tgt, rs, rt, ETA, L, dtype=np.float64), f)
  u = sn.oracle_st_product(oracle, mode, src, tgt, f, rs, rt, ETA, L)
  s = sn.st_reference(name, mode)[1]
  row = (s * np.abs(f).sum(axis=1).astype(EXT)[None, :]).sum(axis=1)
  boxes = len(sn._boxes(sn._period(L)))
  ratio, where = sn.worst(got, u.astype(EXT), row, EPS64)
  assert ratio <= 2 * sn.C_ST[mode, L is not None] + 12 * len(src) * boxes, (ratio, where)
  # sources == targets, N = 200
  if name != "offset":
    r, rad, Ls = sn.same_cloud(name)
    f = np.random.RandomState(12).randn(len(r), 3)
    E, s = sn.same_reference(name, mode)
    u = sn.oracle_st_product(oracle, mode, r, r, f, rad, rad, ETA, Ls)
    row = (s * np.abs(f).sum(axis=1).astype(EXT)[None, :]).sum(axis=1)
    ratio, where = sn.worst(np.einsum("tspq,sq->tp", E, f.astype(EXT)), u.astype(EXT), row, EPS64)
    assert ratio <= 2 * sn.C_ST[mode, Ls is not None] + 12 * len(r) * boxes, (ratio, where)


@pytest.mark.parametrize("name", sorted(sn.AUX_CLOUDS))
@pytest.mark.parametrize("op", AUX_OPS, ids=lambda o: "%s_%s" % o)
def test_float64_aux_restatement_matches_oracle_blocks(oracle, name, op):
  got = _aux_restatement(name, op, np.float64)
  ref = _oracle_aux(oracle, name, op)
  E, s = _aux_reference(name, op)
  # the NaN policy: non-finite exactly where the oracle is (the coincident pairs of the pressure), nowhere else
  assert np.array_equal(np.isfinite(E), np.isfinite(ref)) and np.array_equal(np.isfinite(got), np.isfinite(ref))
  assert np.all(np.isfinite(E)) == (op[0] != "p")
  ratio, where = sn.worst(got, ref.astype(EXT), s, EPS64)
  print("%s %s: restatement fp64 vs oracle %.2f units at %s" % (name, op, ratio, where))
  assert ratio <= 2 * _c_aux(op), (ratio, where)
  # where the scale is zero (a skipped pair without image) the block is exactly zero
  zero = np.broadcast_to((np.asarray(s) == 0).reshape(s.shape + (1,) * (E.ndim - 2)), E.shape)
  assert np.all(E[zero] == 0) and np.all(ref[zero] == 0)
  # multi-source product on the finite targets
  src, nrm, w, tgt = sn.aux(name)
  v = np.random.RandomState(13).randn(len(src), 3)
  u = sn.oracle_pressure_product(oracle, op[1], src, tgt, v) if op[0] == "p" else sn.oracle_dl_product(oracle, op[1], src, tgt, nrm, v, w)
  mine = np.einsum("tsq,sq->t" if op[0] == "p" else "tspq,sq->tp", got, v)
  ok = np.isfinite(np.asarray(E, dtype=np.float64)).reshape(len(tgt), -1).all(axis=1)
  assert np.array_equal(np.isfinite(u).reshape(len(tgt), -1).all(axis=1), ok)
  row = (s * np.abs(v).sum(axis=1).astype(EXT)[None, :])[ok].sum(axis=1)
  ratio, where = sn.worst(mine[ok], u[ok].astype(EXT), row, EPS64)
  assert ratio <= 2 * _c_aux(op) + 12 * len(src), (ratio, where)


# ---------------------------------------------------------------------------------------------------------------------
# 2. EXT restatement == the reference's golden vectors
# ---------------------------------------------------------------------------------------------------------------------
def test_ext_restatement_reproduces_g4_source_target():
  g = np.load(os.path.join(GOLDEN, "g4_source_target.npz"))
  for name in ("small", "mixed", "periodic"):
    src, tgt, f, rs, rt = [g[name + "_" + k] for k in ("source", "target", "force", "radius_source", "radius_target")]
    L = g[name + "_L"] if np.any(g[name + "_L"] > 0) else None
    for wall, mode in ((1, 1), (0, 0), (2, 2)):
      B = sn.st_blocks(mode, src, tgt, rs, rt, float(g[name + "_eta"]), L)
      u = np.einsum("tspq,sq->tp", B, np.asarray(f, dtype=np.float64).reshape(-1, 3).astype(EXT)).astype(np.float64)
      assert rel_err(u, g["%s_wall%d" % (name, wall)]) < TOL_GOLDEN, (name, wall, rel_err(u, g["%s_wall%d" % (name, wall)]))
  c = "mixed"
  B = sn.st_blocks(1, g[c + "_source"], g[c + "_source"], g[c + "_radius_source"], g[c + "_radius_source"], float(g[c + "_eta"]))
  u = np.einsum("tspq,sq->tp", B, np.asarray(g[c + "_force"], dtype=np.float64).reshape(-1, 3).astype(EXT)).astype(np.float64)
  assert rel_err(u, g["mixed_radii_self_wall1"]) < TOL_GOLDEN


def test_ext_restatement_reproduces_g11_aux_operators():
  g = load_golden(golden_files("g11_aux_operators.npz")[0])
  src, tgt, f = g["source"], g["target"], np.asarray(g["force"], dtype=np.float64).reshape(-1, 3)
  prod = lambda B, v, sub: np.einsum(sub, B, v.astype(EXT)).astype(np.float64)        # noqa: E731
  assert rel_err(prod(sn.pressure_rows(0, src, tgt), f, "tsq,sq->t"), g["p_no_wall"]) < TOL_GOLDEN
  for k in (0, 7, len(src) - 1):
    assert rel_err(prod(sn.pressure_rows(1, src[k:k + 1], tgt), f[k:k + 1], "tsq,sq->t"), g["p_wall_single_%d" % k]) < TOL_GOLDEN
  assert rel_err(prod(sn.pressure_rows(1, src, tgt), f, "tsq,sq->t"), g["p_wall_superposed"]) < TOL_GOLDEN
  a = float(g["blob_radius"])
  v = np.asarray(g["vector"], dtype=np.float64).reshape(-1, 3)
  for t, sfx in ((tgt, ""), (src, "_self")):
    for variant, key in (("free", "dl_no_wall"), ("wall", "dl_wall"), ("rpy", "dl_rpy")):
      u = prod(sn.dl_blocks(variant, src, t, g["normals"], g["weights"], a), v, "tspq,sq->tp")
      assert rel_err(u, g[key + sfx]) < TOL_GOLDEN, (key + sfx, rel_err(u, g[key + sfx]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the yardsticks
# ---------------------------------------------------------------------------------------------------------------------
def measure_c_st(oracle):
  out = {}
  for mode in sn.MODES:
    for periodic, names in ((False, ("open", "offset")), (True, ("odd", "pow2"))):
      out[mode, periodic] = max(sn.worst(_oracle_st(oracle, n, mode), *sn.st_reference(n, mode), EPS64)[0] for n in names)
  return out


def measure_c_st32():
  out = {}
  for mode in (0, 1):
    worst = 0.0
    for name in ("open", "offset"):
      src, rs, tgt, rt, L = sn.cloud(name)
      worst = max(worst, sn.worst(sn.st_blocks(mode, src, tgt, rs, rt, ETA, dtype=np.float32), *sn.st_reference(name, mode), EPS32)[0])
    r, rad, L = sn.same_cloud("open")
    worst = max(worst, sn.worst(sn.st_blocks(mode, r, r, rad, rad, ETA, dtype=np.float32), *sn.same_reference("open", mode), EPS32)[0])
    out[mode] = worst
  return out


def measure_c_aux(oracle):
  p, dl = {}, {}
  for op in AUX_OPS:
    (p if op[0] == "p" else dl)[op[1]] = max(sn.worst(_oracle_aux(oracle, n, op), *_aux_reference(n, op), EPS64)[0] for n in sn.AUX_CLOUDS)
  return p, dl


def oracle_edge_product(oracle, op, ns, nt):
  e = sn.edge_problem(ns, nt)
  if op[0] == "st":
    return sn.oracle_st_product(oracle, op[1], e["src"], e["tgt"], e["f"], e["rs"], e["rt"], ETA)
  if op[0] == "p":
    return sn.oracle_pressure_product(oracle, op[1], e["src"], e["tgt"], e["f"])
  return sn.oracle_dl_product(oracle, op[1], e["src"], e["tgt"], e["nrm"], e["v"], e["w"])


def measure_c_sum(oracle):
  st, p, dl = {}, {}, {}
  for op in [("st", m) for m in sn.MODES] + AUX_OPS:
    worst = 0.0
    for ns, nt in sn.EDGE_SHAPES:
      u, row = sn.edge_reference(op, ns, nt)
      assert np.all(np.isfinite(u)) and np.all(row > 0)
      worst = max(worst, sn.worst(oracle_edge_product(oracle, op, ns, nt), u, row, EPS64)[0])
    {"st": st, "p": p, "dl": dl}[op[0]][op[1]] = worst
  return st, p, dl


def _print_table(title, table):
  print("\n%s = {" % title)
  for key in sorted(table, key=str):
    print("    %r: %.0f.0,      # measured %.2f" % (key, np.ceil(table[key]), table[key]))
  print("}")


def _check(title, got, committed):
  _print_table(title, got)
  assert set(got) == set(committed)
  for key, val in got.items():
    assert np.isfinite(val) and val <= committed[key], (title, key, val, committed[key])
    assert committed[key] <= 2 * val + 2, (title, key, "the committed value is stale: far above what is measured", val)


def test_yardstick_blocks_do_not_exceed_the_committed_tables(oracle):
  """C = max over elements of |oracle_fp64 - EXT| / (2^-53 s), recomputed: the committed numbers are what the GPU test
  multiplies by MARGIN, so they may only be too large, never too small (and not stale either)."""
  _check("C_ST", measure_c_st(oracle), sn.C_ST)
  _check("C_ST32", measure_c_st32(), sn.C_ST32)
  p, dl = measure_c_aux(oracle)
  _check("C_P", p, sn.C_P)
  _check("C_DL", dl, sn.C_DL)


def test_yardstick_products_do_not_exceed_the_committed_tables(oracle):
  st, p, dl = measure_c_sum(oracle)
  _check("C_ST_SUM", st, sn.C_ST_SUM)
  _check("C_P_SUM", p, sn.C_P_SUM)
  _check("C_DL_SUM", dl, sn.C_DL_SUM)


# ---------------------------------------------------------------------------------------------------------------------
# 4. a physical property of the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_no_slip_velocity_vanishes_at_tracers_on_the_wall():
  """u(z = 0) = 0 above a no-slip wall: with radius_target = 0 and z_t = 0 the image system cancels the free part
  identically (R = r, and every term with x3 or a_t^2 is absent), so the wall product is pure rounding:
  |u_t| <= C eps sum_s s_ts |f_s|.  In EXT eps = 2^-64 (C_ST[1] is an fp64 count; the term count is the same)."""
  src, rs, tgt, rt, f = sn.tracer_problem()
  assert np.all(rt == 0) and np.all(tgt[:, 2] == 0)
  s = sn.st_scale(1, src, tgt, rs, rt, ETA)
  row = (s * np.abs(f).max(axis=1).astype(EXT)[None, :]).sum(axis=1)
  for dtype, eps in ((EXT, 2.0 ** -64), (np.float64, EPS64)):
    u = np.einsum("tspq,sq->tp", sn.st_blocks(1, src, tgt, rs, rt, ETA, dtype=dtype), f.astype(dtype))
    assert np.all(np.abs(u) <= sn.C_ST[1, False] * eps * row[:, None]), float((np.abs(u) / (eps * row[:, None])).max())
  free = np.einsum("tspq,sq->tp", sn.st_blocks(0, src, tgt, rs, rt, ETA), f.astype(EXT))
  assert np.abs(free).max() > 1e-3          # the free part alone is O(1): the cancellation is the image system's doing
