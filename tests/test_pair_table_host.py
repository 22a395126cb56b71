"""Tabulated pair law, host side (no GPU): the PairTable class, the yardstick of tests/_pair_table_numpy.py and its constants
C, the C ABI's argument refusals through a null context, and the callers' refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pair_table_numpy as pt      # noqa: E402
from _pair_table_numpy import EXT, PairTable      # noqa: E402
from rigidmultiblobswall_amd import _lib      # noqa: E402
from rigidmultiblobswall_amd import pair_table as ptm      # noqa: E402

needs_ext = pytest.mark.skipif(not pt.LONG_DOUBLE, reason="np.longdouble has no 64-bit mantissa on this platform")


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick's constants
# ---------------------------------------------------------------------------------------------------------------------
def _measure():
  """Worst ratio of the float64 restatement against EXT per (family, periodic): the ladders and a radial scan for every K,
  the clouds of 65 and 129 blobs for every K."""
  worst = {k: 0.0 for k in pt.C}
  for K in pt.K_LIST:
    T = pt.lj_table(K)
    # radial scan: U against S_U, U' against S_F (one pair along x: the force component is U' itself)
    rng = np.random.RandomState(K)
    r = np.concatenate([rng.uniform(0.01, T.r_cut, 4000), [pt.ladder_distance(T, g) for g in pt.RUNGS]])
    U, dU, S_U, S_F = pt.radial(T, r.astype(EXT))
    u64, du64, _, _ = pt.radial(T, r, np.float64)
    for per in (False, True):      # the law of one pair knows no box
      worst["energy", per] = max(worst["energy", per], pt.worst(u64, U, S_U, 1.0))
      worst["force", per] = max(worst["force", per], pt.worst(du64, dU, S_F, 1.0))
    for size in (65, 129):
      for variant in ("open", "box", "box3"):
        r, L = pt.cloud(size, variant)
        per = L is not None
        F, S = pt.forces(T, r, L)
        worst["force", per] = max(worst["force", per], pt.worst(pt.forces(T, r, L, np.float64)[0], F, S, 1.0))
        if variant != "box3":
          U, S = pt.energy(T, r, L)
          worst["energy", per] = max(worst["energy", per], pt.worst(pt.energy(T, r, L, np.float64)[0], U, S, 1.0))
  return worst


@needs_ext
def test_yardstick_constants():
  worst = _measure()
  for key in sorted(worst):
    print("C[%r]: measured %.3f, stored %.1f (recorded %.3f)" % (key, worst[key], pt.C[key], pt.C_MEASURED[key]))
  for key, m in worst.items():
    assert m <= pt.C[key] <= 2.0 * m + 1.0, (key, m, pt.C[key])
    assert abs(pt.C_MEASURED[key] - m) <= 0.05 * m + 0.01, (key, m, pt.C_MEASURED[key])


# ---------------------------------------------------------------------------------------------------------------------
# PairTable
# ---------------------------------------------------------------------------------------------------------------------
def _hermite_ext(r0, h, u, d, r):
  """Cubic Hermite interpolant of the knots in EXT, in the basis form (not the table's coefficients)."""
  u, d, r = np.asarray(u, dtype=EXT), np.asarray(d, dtype=EXT), np.asarray(r, dtype=EXT)
  K = len(u) - 1
  x = (r - EXT(r0)) / EXT(h)
  k = np.minimum(np.floor(x), K - 1).astype(int)
  t = x - k
  h00, h10, h01, h11 = 2 * t ** 3 - 3 * t ** 2 + 1, t ** 3 - 2 * t ** 2 + t, -2 * t ** 3 + 3 * t ** 2, t ** 3 - t ** 2
  p = h00 * u[k] + h10 * EXT(h) * d[k] + h01 * u[k + 1] + h11 * EXT(h) * d[k + 1]
  dh00, dh10, dh01, dh11 = 6 * t ** 2 - 6 * t, 3 * t ** 2 - 4 * t + 1, -6 * t ** 2 + 6 * t, 3 * t ** 2 - 2 * t
  dp = (dh00 * u[k] + dh10 * EXT(h) * d[k] + dh01 * u[k + 1] + dh11 * EXT(h) * d[k + 1]) / EXT(h)
  return p, dp


@needs_ext
@pytest.mark.parametrize("K", pt.K_LIST)
def test_from_knots_is_the_hermite_interpolant(K):
  U, dU = ptm.lennard_jones()
  r0, rc = pt.LJ["r0"], pt.LJ["r_cut"]
  h = (rc - r0) / K
  rk = EXT(r0) + np.arange(K + 1, dtype=EXT) * EXT(h)
  u, d = U(rk), dU(rk)
  T = PairTable.from_knots(r0, h, u, d)
  assert T.K == K and T.r0 == r0 and T.h == h and T.r_cut == r0 + K * h
  # knots (from the left interval and the right one) and midpoints, against the basis form in EXT; the bound is the
  # rounding of the four coefficients (2^-53 each, amplified by nothing: |basis| <= 1) plus the fp64 evaluation (C)
  r = np.concatenate([rk[:-1], rk[:-1] + EXT(0.5) * EXT(h), np.nextafter(rk[1:].astype(np.float64), 0.0).astype(EXT)])
  p, dp = _hermite_ext(r0, h, u, d, r)
  Ue, dUe, S_U, S_F = pt.radial(T, r)
  assert pt.worst(Ue, p, S_U, 2.0) <= 1.0 and pt.worst(dUe, dp, S_F, 4.0) <= 1.0
  r64 = r.astype(np.float64)
  assert pt.worst(T.U(r64), p, S_U, pt.MARGIN * pt.C["energy", False]) <= 1.0
  assert pt.worst(T.dU(r64), dp, S_F, pt.MARGIN * pt.C["force", False]) <= 1.0
  # the class's own evaluation IS the restatement in float64
  u64, du64, _, _ = pt.radial(T, r64, np.float64)
  assert np.array_equal(T.U(r64), u64) and np.array_equal(T.dU(r64), du64)


def test_definition_outside_the_intervals():
  T = pt.lj_table(16, "none")
  c, h, r0 = T.coeff, T.h, T.r0
  r = np.array([0.0, 0.25 * r0, np.nextafter(r0, 0.0)])
  assert np.allclose(T.U(r), c[0, 0] + (c[0, 1] / h) * (r - r0), rtol=1e-15, atol=0)
  assert np.allclose(T.dU(r), c[0, 1] / h, rtol=1e-15, atol=0)
  assert T.U(0.0) == c[0, 0] + (0.0 - r0) * (1.0 / h) * c[0, 1]
  beyond = np.array([T.r_cut, np.nextafter(T.r_cut, np.inf), 1.5 * T.r_cut, 2e100])
  assert pt.is_positive_zero(T.U(beyond)) and pt.is_positive_zero(T.dU(beyond))
  assert T.U(np.nextafter(T.r_cut, 0.0)) != 0.0          # shift="none": the law jumps at r_cut
  assert T.U(np.nan) == 0.0 and T.dU(np.nan) == 0.0      # a NaN distance fails r < r_cut (and reads interval 0, never beyond the table)


@needs_ext
def test_shift_modes():
  U, dU = ptm.lennard_jones()
  r0, rc, K = pt.LJ["r0"], pt.LJ["r_cut"], 16
  none, en, fo = (PairTable.from_function(U, dU, r0, rc, K, shift=s) for s in ("none", "energy", "force"))
  uc, dc = float(U(EXT(rc))), float(dU(EXT(rc)))
  rn, un, dn = none.knots()
  _, ue, de = en.knots()
  _, uf, df = fo.knots()
  tol = 8 * np.finfo(float).eps * np.abs(un).max()
  assert abs(un[-1] - uc) <= tol and abs(dn[-1] - dc) <= tol / none.h
  assert abs(ue[-1]) <= tol and np.allclose(ue, un - uc, rtol=0, atol=tol) and np.allclose(de, dn, rtol=0, atol=tol / none.h)
  assert abs(uf[-1]) <= tol and abs(df[-1]) <= tol / none.h
  assert np.allclose(uf, un - (uc + (rn - rc) * dc), rtol=0, atol=tol) and np.allclose(df, dn - dc, rtol=0, atol=tol / none.h)
  with pytest.raises(ValueError, match="shift"):
    PairTable.from_function(U, dU, r0, rc, K, shift="both")


def test_constructor_refusals():
  ok = np.zeros((3, 4))
  for kw, match in ((dict(r0=-0.1, h=1.0, coeff=ok), "r0"), (dict(r0=np.inf, h=1.0, coeff=ok), "r0"), (dict(r0=0.0, h=0.0, coeff=ok), "h must"),
                    (dict(r0=0.0, h=np.nan, coeff=ok), "h must"), (dict(r0=0.0, h=1.0, coeff=np.zeros((0, 4))), "1..1024"),
                    (dict(r0=0.0, h=1.0, coeff=np.zeros((1025, 4))), "1..1024"), (dict(r0=0.0, h=1.0, coeff=np.zeros((3, 3))), "shape"),
                    (dict(r0=0.0, h=1.0, coeff=np.full((3, 4), np.nan)), "finite")):
    with pytest.raises(ValueError, match=match):
      PairTable(**kw)
  assert PairTable(0.0, 1.0, np.zeros((1024, 4))).K == 1024
  with pytest.raises(ValueError, match="K must be"):
    PairTable.from_function(*ptm.lennard_jones(), 0.9, 2.5, 1025)


def test_file_round_trip_and_refusals(tmp_path):
  T = pt.lj_table(16)
  path = str(tmp_path / "lj.table")
  T.save(path)
  with open(path) as fh:
    text = fh.read()
  assert text.startswith("#") and len([ln for ln in text.splitlines() if not ln.startswith("#")]) == 17
  T2 = PairTable.load(path)
  assert T2.K == T.K and T2.r0 == T.r0 and abs(T2.h - T.h) <= 2 * np.finfo(float).eps * T.h
  # the file carries knots and slopes in 17 digits: the reloaded coefficients are the Hermite table of those numbers
  scale = np.abs(T.coeff).max(axis=1, keepdims=True)
  assert np.all(np.abs(T2.coeff - T.coeff) <= 64 * np.finfo(float).eps * scale)
  # comments and blank lines
  with open(path, "w") as fh:
    fh.write("# a harmonic bond 0.5 (r - 1)^2\n\n0.5 0.125 -0.5   # first knot\n1.0 0.0 0.0\n1.5 0.125 0.5\n")
  H = PairTable.load(path)
  assert H.K == 2 and H.r0 == 0.5 and H.h == 0.5 and abs(H.U(1.25) - 0.03125) < 1e-16 and abs(H.dU(0.75) + 0.25) < 1e-16
  for body, match in (("0.5 1 0\n1.0 0 0\n1.6 1 0\n", "not uniformly spaced"), ("0.5 1 0\n", "2 to 1025 rows"), ("0.5 1\n1.0 0\n", "columns"),
                      ("1.0 1 0\n0.5 0 0\n", "must increase"), ("0.5 x 0\n1.0 0 0\n", "not a number"),
                      ("".join("%r 0 0\n" % (0.5 + 0.001 * k,) for k in range(1027)), "2 to 1025 rows")):
    with open(path, "w") as fh:
      fh.write(body)
    with pytest.raises(ValueError, match=match):
      PairTable.load(path)


@needs_ext
def test_yukawa_table_interpolates_within_the_derived_bounds():
  """Cubic Hermite interpolation of a C^4 function on a uniform grid: |U - p| <= h^4/384 max|U''''| and
  |U' - p'| <= sqrt(3)/216 h^3 max|U''''|; the Yukawa law eps = 1, b = 0.5 on [0.5, 8], K = 1024."""
  T = pt.yukawa_table("none")
  U, dU = ptm.yukawa(pt.YUK["eps"], pt.YUK["b"])
  m4, h = pt.yukawa_d4_max(), EXT(T.h)
  r = (EXT(T.r0) + (np.arange(20 * T.K, dtype=EXT) + EXT(0.5)) * h / 20).astype(np.float64)
  p, dp, S_U, S_F = pt.radial(T, r.astype(EXT))
  eU, edU = np.abs(U(r.astype(EXT)) - p), np.abs(dU(r.astype(EXT)) - dp)
  bU, bdU = h ** 4 / 384 * m4, np.sqrt(EXT(3)) / 216 * h ** 3 * m4
  round_U, round_dU = 4 * EXT(pt.EPS64) * S_U, 4 * EXT(pt.EPS64) * S_F          # the coefficients' own rounding
  print("worst |U - p| / bound %.3f, worst |U' - p'| / bound %.3f" % (float((eU / bU).max()), float((edU / bdU).max())))
  assert np.all(eU <= bU + round_U) and np.all(edU <= bdU + round_dU)
  assert (eU / bU).max() > 0.5 and (edU / bdU).max() > 0.5          # the bounds are sharp where U'''' is largest


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
EXPORTS = ("rmb_ctx_set_pair_table", "rmb_pair_table_force", "rmb_pair_table_force_device", "rmb_blob_potential_table",
           "rmb_blob_potential_table_device")


def test_exports_and_header():
  lib = _lib.load()
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rmb_mobility.h")).read()
  for name in EXPORTS:
    assert name in _lib.SYMBOLS and hasattr(lib, name) and ("int %s(" % name) in header, name


def test_set_pair_table_refuses_bad_arguments_without_a_device():
  lib = _lib.load()
  good = np.ascontiguousarray(pt.lj_table(16).coeff)
  big = np.zeros((1025, 4))
  bad = good.copy()
  bad[3, 2] = np.inf
  p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
  cases = [((0.5, 0.1, 1025, p(big)), "1..1024"), ((0.5, 0.1, -1, p(good)), "1..1024"), ((0.5, 0.0, 16, p(good)), "width h"),
           ((0.5, -0.1, 16, p(good)), "width h"), ((0.5, float("nan"), 16, p(good)), "width h"), ((0.5, float("inf"), 16, p(good)), "width h"),
           ((-0.5, 0.1, 16, p(good)), "r0"), ((float("nan"), 0.1, 16, p(good)), "r0"), ((float("inf"), 0.1, 16, p(good)), "r0"),
           ((0.5, 0.1, 16, p(bad)), "coefficient 14 is not finite"), ((0.5, 0.1, 16, None), "null coefficient"),
           ((0.5, 0.1, 16, p(good)), "null context"), ((0.0, 1.0, 0, None), "null context")]
  for args, match in cases:
    rc = lib.rmb_ctx_set_pair_table(None, *args)
    assert rc != 0 and match in lib.rmb_last_error().decode(), (args[:3], lib.rmb_last_error())
  out = np.zeros(6)
  for fn, args in ((lib.rmb_pair_table_force, ()), (lib.rmb_pair_table_force_device, ()),
                   (lib.rmb_blob_potential_table, (0.0, 1.0, 0.0, 0.5, 0)), (lib.rmb_blob_potential_table_device, (0.0, 1.0, 0.0, 0.5, 0))):
    assert fn(None, *args, p(out)) != 0 and "null context" in lib.rmb_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------
# callers: deck keywords and refusals
# ---------------------------------------------------------------------------------------------------------------------
def _deck(tmp_path, extra):
  (tmp_path / "blob.vertex").write_text("1\n0 0 0\n")
  (tmp_path / "blob.clones").write_text("2\n0 0 1 1 0 0 0\n1.5 0 1 1 0 0 0\n")
  path = tmp_path / "inputfile.dat"
  path.write_text("scheme deterministic_adams_bashforth_rollers\nmobility_vector_prod_implementation hip\nmobility_blobs_implementation hip\n"
                  "domain single_wall\nblob_radius 0.4\n" + extra + "structure blob.vertex blob.clones\n")
  return str(path)


def test_deck_keywords_and_refusals(tmp_path):
  from rigidmultiblobswall_amd import deck_modes, dispatch
  from rigidmultiblobswall_amd.read_input import ReadInput
  pt.lj_table(16).save(str(tmp_path / "lj.table"))
  read = ReadInput(_deck(tmp_path, "blob_blob_force_implementation table_hip\nblob_blob_pair_table lj.table\n"))
  assert read.blob_blob_force_implementation == "table_hip" and read.blob_blob_pair_table == "lj.table"
  for dense in (False, True):
    assert deck_modes.validate(read, uses_dense_blocks=dense, body_body_forces=True) == "single_wall"
    assert deck_modes.validate(read, uses_dense_blocks=dense, pair_tables=True) == "single_wall"
  T = deck_modes.pair_table(read)          # the path is relative to the deck
  assert T.K == 16 and T.r0 == pt.LJ["r0"]
  # a context without the sweep (the multi-device engine): refused, as body-body forces are
  with pytest.raises(ValueError, match="single-GPU MobilityContext"):
    deck_modes.validate(read, uses_dense_blocks=False, body_body_forces=False)
  with pytest.raises(ValueError, match="single-GPU MobilityContext"):
    deck_modes.validate(read, uses_dense_blocks=True, body_body_forces=True, pair_tables=False)
  # the file is missing / the keyword is missing / the keyword without the implementation
  with pytest.raises(ValueError, match="no such file"):
    deck_modes.validate(ReadInput(_deck(tmp_path, "blob_blob_force_implementation table_hip\nblob_blob_pair_table nowhere.table\n")), False, True)
  with pytest.raises(ValueError, match="needs `blob_blob_pair_table FILE`"):
    deck_modes.validate(ReadInput(_deck(tmp_path, "blob_blob_force_implementation table_hip\n")), False, True)
  with pytest.raises(ValueError, match="table_hip` only"):
    deck_modes.validate(ReadInput(_deck(tmp_path, "blob_blob_force_implementation hip\nblob_blob_pair_table lj.table\n")), False, True)
  # decks without the new keywords are what they were
  plain = ReadInput(_deck(tmp_path, "blob_blob_force_implementation hip\n"))
  assert plain.blob_blob_pair_table is None and deck_modes.pair_table(plain) is None
  assert deck_modes.validate(plain, uses_dense_blocks=False) == "single_wall"
  # dispatch
  f = dispatch.set_blob_blob_forces("table_hip", pair_table=T)
  assert f.func.__name__ == "calc_blob_blob_forces_table_hip" and f.keywords["pair_table"] is T
  assert dispatch.set_blob_blob_forces("table_hip", pair_table_file=str(tmp_path / "lj.table")).keywords["pair_table"].K == 16
  with pytest.raises(ValueError, match="does not exist"):
    dispatch.set_blob_blob_forces("table_hip", pair_table_file=str(tmp_path / "nowhere.table"))
  with pytest.raises(ValueError, match="needs pair_table="):
    dispatch.set_blob_blob_forces("table_hip")
  with pytest.raises(ValueError, match="must be a PairTable"):
    dispatch.set_blob_blob_forces("table_hip", pair_table=np.zeros((4, 4)))
  with pytest.raises(ValueError, match="not served"):
    dispatch.set_blob_blob_forces("table_cuda")


def test_out_of_scope_requests_are_refused(tmp_path, monkeypatch):
  from rigidmultiblobswall_amd import forces, potential
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  T = pt.lj_table(16)
  r = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0]])
  with pytest.raises(ValueError, match="PairTable"):
    forces.calc_blob_blob_forces_table_hip(r, pair_table=None)
  with pytest.raises(ValueError, match="per-blob radii"):
    forces.calc_blob_blob_forces_table_hip(r, pair_table=T, radius_blobs=np.ones(2))
  with pytest.raises(ValueError, match="single-body"):
    potential.body_energy_difference_hip(r, 0, r[:1], pair_table=T, potential="soft")
  # the sampler: single-body moves, a caller's energy function, a wrong type -- all before a device is touched
  (tmp_path / "blob.vertex").write_text("1\n0 0 0\n")
  (tmp_path / "blob.clones").write_text("2\n0 0 1 1 0 0 0\n1.5 0 1 1 0 0 0\n")
  (tmp_path / "data.main").write_text("n_steps 2\nblob_radius 0.4\nseed 1\nstructure blob.vertex blob.clones\n")
  monkeypatch.chdir(tmp_path)
  with pytest.raises(ValueError, match="moves='single' does not serve a pair table"):
    MCMCSampler("data.main", pair_table=T, moves="single", write_files=False)
  with pytest.raises(ValueError, match="energy= function"):
    MCMCSampler("data.main", pair_table=T, energy=lambda x: 0.0, write_files=False)
  with pytest.raises(ValueError, match="PairTable or the path"):
    MCMCSampler("data.main", pair_table=3.0, write_files=False)
  with pytest.raises(ValueError, match="not uniformly spaced"):
    (tmp_path / "bad.table").write_text("0.5 1 0\n1.0 0 0\n1.6 1 0\n")
    MCMCSampler("data.main", pair_table="bad.table", write_files=False)
