"""The yardstick of tests/test_gpu_rigid_kernels.py and tests/test_gpu_block_apply.py, checked on the CPU: the fp64 numpy
restatement of the per-body kernels (tests/_rigid_kernels_numpy.py) meets every bound on every case of the GPU tests, the
committed table C of its worst fractions is current, and five mutants of the restatement -- each of which passes the
assertions of tests/test_gpu_krylov.py, restated here at their tolerances on their inputs -- exceed the new bounds."""
import numpy as np
import pytest

import _rigid_kernels_numpy as rk

EXT = rk.EXT
_measured = {}


def _note(key, value, where=None):
  if value > _measured.get(key, (-1.0, None))[0]:
    _measured[key] = (value, where)


def _measure_pc():
  if "pc" in _measured:
    return
  _measured["pc"] = (0.0, None)
  def one(M, K, fam, n_b, where, large=None, ref=None):
    kern = "large" if (3 * n_b > rk.SMALL_MAX_N if large is None else large) else "small"
    o = rk.preconditioner(M, K, np.float64, large)
    ref = rk.preconditioner(M, K, EXT, large) if ref is None else ref
    full = rk.expected_info(fam, n_b) == 0
    assert o["info"] == ref["info"] == rk.expected_info(fam, n_b), where
    assert rk.exact_structure(o) == [], (where, rk.exact_structure(o))
    for q, v in rk.factor_fractions(o, M, K, large, full=full).items():
      _note((q, kern), v, where)
    for q, v in rk.e2e_fractions(o, ref, rk.E2E if full else ("Minv", "Lchol")).items():
      _note((q, fam, kern), v, where)
  for fam, n_b, bnd in rk.pc_launches():
    for v in range(3):
      M, K = rk.body(fam, n_b, bnd, v)
      one(M, K, fam, n_b, (fam, n_b, bnd, v), ref=rk.ext_reference(fam, n_b, bnd, v))
  for fam, n_b, bnd in rk.SKEW_CASES:
    for v in range(3):
      M, K = rk.body(fam, n_b, bnd, v)
      one(rk.skewed(M, v), K, fam, n_b, ("skew", fam, n_b, bnd, v), ref=rk.ext_reference(fam, n_b, bnd, v, skew_seed=v))


def _measure_rest():
  if "rest" in _measured:
    return
  _measured["rest"] = (0.0, None)
  for n_b, nb in rk.CONFIG_SHAPES:
    ref, loc, quat = rk.config_case(n_b, nb)
    r, rel, _ = rk.configuration(ref, loc, quat, np.float64)
    for q, v in rk.config_fractions(r, rel, ref, loc, quat).items():
      _note((q,), v, (n_b, nb))
  for nb in rk.ADVANCE_BODIES:
    for per_body in (False, True):
      loc, quat, Uv, dt, ang = rk.advance_case(nb, per_body)
      l2, q2, _, _ = rk.advance(loc, quat, Uv, dt, np.float64)
      for q, v in rk.advance_fractions(l2, q2, loc, quat, Uv, dt).items():
        _note((q,), v, (nb, per_body))
  for case in rk.block_cases():
    nb, r1, c1, r2, c2, al, be, seed = case
    d = rk.block_case(nb, r1, c1, r2, c2, seed)
    for A, B, y0 in ((d["A11"], d["A12"], d["y1"]), (d["A21"], d["A22"], d["y2"])):
      y, _ = rk.block_apply(A, B, d["x1"], d["x2"], y0, al, be, np.float64)
      _note(("block",), rk.block_fraction(y, A, B, d["x1"], d["x2"], y0, al, be), case)
  for label, _, d, al, be, blocks in rk.block_extra_cases():
    for A, B, y0 in ((blocks[0], blocks[1], d["y1"]), (blocks[2], blocks[3], d["y2"])):
      y, _ = rk.block_apply(A, B, d["x1"], d["x2"], y0, al, be, np.float64)
      _note(("block",), rk.block_fraction(y, A, B, d["x1"], d["x2"], y0, al, be), label)


def _keys():
  return sorted(k for k in _measured if k not in ("pc", "rest"))


def test_long_double_is_extended():
  assert rk.LONG_DOUBLE and np.finfo(EXT).nmant >= 63


def test_cw_ratio_demands_exact_zeros():
  assert rk.cw_ratio(np.array([0.0, rk.U]), np.array([0.0, 1.0])) == 1.0
  assert rk.cw_ratio(np.array([1e-300, 0.0]), np.array([0.0, 1.0])) == float("inf")
  assert rk.cw_ratio(np.array([np.nan]), np.array([1.0])) == float("inf")
  assert rk.cw_ratio(np.zeros(3), np.zeros(3)) == 0.0


def test_families_have_exact_zeros_and_a_range_of_conditioning():
  M, _ = rk.body("bent", 12, "none", 0)
  assert (M == 0.0).sum() > 0                     # a planar body in an unbounded fluid: exact zeros off the diagonal
  conds = [np.linalg.cond(rk.body(f, 42, "wall", 1)[0]) for f in ("shell", "bent", "overlap", "loose", "dense")]
  assert min(conds) < 50 and max(conds) > 150, conds


def test_table_is_current_and_the_restatement_meets_every_bound(capsys):
  _measure_pc()
  _measure_rest()
  with capsys.disabled():
    print()
    for k in _keys():
      print("    %-34s %8.6g,   # measured %.4f at %s" % (repr(k) + ":", _round_up(_measured[k][0]), _measured[k][0], (_measured[k][1],)))
  assert set(_keys()) == set(rk.C), (set(_keys()) ^ set(rk.C))
  for k in _keys():
    m = _measured[k][0]
    assert m <= rk.C[k], (k, m, rk.C[k])                       # the table covers the restatement ...
    assert rk.C[k] <= _round_up(m) * 1.0000001, (k, m, rk.C[k])      # ... and is not padded
    assert m <= rk.bound(k), (k, m, rk.bound(k))
    derived = not (k[0] == "nres" or k[0].startswith("e2e_"))
    if derived:
      assert m < 1.0, (k, m)


def _round_up(x):
  """three significant digits, upwards"""
  if x <= 0:
    return 0.0
  e = 10.0 ** (np.floor(np.log10(x)) - 2)
  return float(np.ceil(x / e) * e)


def test_every_derived_bound_holds_with_the_margin_where_the_table_says_so():
  """MARGIN C <= 1 (the derived bound) is what the asserted bound min(MARGIN C, 1) relies on to be a tightening; where
  MARGIN C exceeds 1 the derived bound itself is asserted.  Listed, so that a change of either is seen."""
  over = sorted(k for k in rk.C if not (k[0] == "nres" or k[0].startswith("e2e_")) and rk.MARGIN * rk.C[k] > 1.0)
  assert over == sorted(rk.DERIVED_BOUND_APPLIES), over


# ---------------------------------------------------------------------------------------------------------------------
# the assertions of tests/test_gpu_krylov.py, restated
# ---------------------------------------------------------------------------------------------------------------------
PRESENT_PC = ((1, 3), (5, 12), (9, 16), (6, 4), (3, 17), (7, 30), (2, 42))          # its (nb, n_b) below 300 bodies
PRESENT_N_B = (3, 4, 12, 16, 17, 30, 42)


def _present_pc_inputs(nb, n_b):
  rng = np.random.RandomState(nb * 7 + n_b)
  n = 3 * n_b
  G = rng.randn(nb, n, n)
  Mb = G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
  K = np.stack([rk.build_K(rel) for rel in rng.randn(nb, n_b, 3)])
  skew = 1e-13 * rng.randn(nb, n, n)
  return Mb, K, Mb + skew - skew.transpose(0, 2, 1)


def _present_pc_assertions(o, Mb, K):
  nb, n = Mb.shape[0], Mb.shape[1]
  assert o["info"] == 0
  L = np.linalg.cholesky(Mb)
  assert np.abs(o["Lchol"] - L).max() < 1e-12 and np.abs(np.triu(o["Lchol"], 1)).max() == 0.0
  eye = np.eye(n)
  assert np.abs(o["Linv"] @ L - eye).max() < 1e-11
  assert np.abs(o["Minv"] @ Mb - eye).max() < 1e-10 and np.abs(o["Minv"] - o["Minv"].transpose(0, 2, 1)).max() == 0.0
  Rres = K.transpose(0, 2, 1) @ np.linalg.solve(Mb, K)
  assert np.abs(o["Nbody"] @ Rres - np.eye(6)).max() < 1e-9 and np.abs(o["Nbody"] - o["Nbody"].transpose(0, 2, 1)).max() == 0.0
  S = np.zeros((nb, n + 6, n + 6))
  S[:, :n, :n] = Mb; S[:, :n, n:] = -K; S[:, n:, :n] = -K.transpose(0, 2, 1)
  P = np.zeros_like(S)
  P[:, :n, :n] = o["A11"]; P[:, :n, n:] = o["A12"]; P[:, n:, :n] = o["A21"]; P[:, n:, n:] = o["A22"]
  assert np.abs(P @ S - np.eye(n + 6)).max() < 1e-8
  assert np.abs(o["A21"] - o["A12"].transpose(0, 2, 1)).max() == 0.0


def _neighbour_mutant(Ms, Ks, n_b):
  """mutant (e): at a body size the older test does not run, body 1's A12 (and with it A11) is formed with body 0's N"""
  o = rk.preconditioner_batch(Ms, Ks)
  if n_b not in PRESENT_N_B and len(Ms) > 1:
    m = rk.preconditioner(Ms[1], Ks[1], N_other=o["Nbody"][0])
    for name in ("A11", "A12", "A21"):
      o[name][1] = m[name]
  return o


def _exceeds(label, fraction, key):
  factor = fraction / rk.bound(key)
  print("  mutant %s: %s at %.3g of its bound" % (label, key, factor))
  return factor


def test_mutant_a_no_symmetrisation_on_load(capsys):
  for nb, n_b in PRESENT_PC:
    Mb, K, Min = _present_pc_inputs(nb, n_b)
    _present_pc_assertions(rk.preconditioner_batch(Min, K, symmetrise=False), Mb, K)
  with capsys.disabled():
    for fam, n_b, bnd in rk.SKEW_CASES:
      M, K = rk.body(fam, n_b, bnd, 0)
      Ms = rk.skewed(M, 0)
      f = rk.factor_fractions(rk.preconditioner(Ms, K, symmetrise=False), Ms, K, full=False)
      assert _exceeds("a", f["chol"], ("chol", rk.kernel_of(n_b))) > 1.0


def test_mutant_b_fp32_seeded_root(capsys):
  for nb, n_b in PRESENT_PC:
    Mb, K, Min = _present_pc_inputs(nb, n_b)
    _present_pc_assertions(rk.preconditioner_batch(Min, K, root=rk.root_fp32_seed), Mb, K)
  with capsys.disabled():
    for fam, n_b, bnd in (("shell", 12, "wall"), ("dense", 16, "wall"), ("bent", 22, "wall"), ("overlap", 17, "none")):
      M, K = rk.body(fam, n_b, bnd, 1)
      f = rk.factor_fractions(rk.preconditioner(M, K, root=rk.root_fp32_seed), M, K, full=False)
      assert _exceeds("b", f["chol"], ("chol", rk.kernel_of(n_b))) > 1.0


def test_mutant_c_half_for_small_angles(capsys):
  import torch
  g = torch.Generator().manual_seed(4)
  nb = 777
  loc = torch.randn(nb, 3, generator=g, dtype=torch.float64).numpy()
  quat = torch.randn(nb, 4, generator=g, dtype=torch.float64)
  quat = (quat / quat.norm(dim=1, keepdim=True)).numpy()
  Uv = torch.randn(nb, 6, generator=g, dtype=torch.float64).numpy()
  Uv[5, 3:] = 0.0
  for dt in (0.013, torch.rand(nb, 1, generator=g, dtype=torch.float64).numpy().reshape(-1)):
    l_ref, q_ref, _, _ = rk.advance(loc, quat, Uv, dt)
    l2, q2, _, _ = rk.advance(loc, quat, Uv, dt, half_below=1e-4)
    assert np.abs(l2 - l_ref).max() < 1e-14 and np.abs(q2 - q_ref).max() < 1e-14
    assert np.array_equal(q2[5], quat[5]) and np.abs(np.linalg.norm(q2, axis=1) - 1).max() < 1e-14
  loc, quat, Uv, dt, ang = rk.advance_case(257, False)
  l2, q2, _, _ = rk.advance(loc, quat, Uv, dt, half_below=1e-4)
  with capsys.disabled():
    assert _exceeds("c", rk.advance_fractions(l2, q2, loc, quat, Uv, dt)["advance_quat"], ("advance_quat",)) > 1.0


def test_mutant_d_last_entry_of_a_small_row_dropped(capsys):
  """the older assertion is a norm over the whole output (rel_err < 1e-13) with every row on one scale, where a dropped entry
  is seen.  Its input cannot hold the mutant's row, so the older assertion is applied to its shape (5, 36, 36, 6) with the rows
  scaled by 1e-8 ... 1e8 as the new test scales them: the dropped entry of a row at 1e-8 is 1e-18 of the norm."""
  from conftest import rel_err
  nb, r = 5, 36
  d = rk.block_case(nb, r, 36, 6, 6, seed=5 + 36)
  A1, A2, x1, x2 = d["A11"], d["A12"], d["x1"], d["x2"]
  row = int(np.argmin(np.abs(A1[2]).max(axis=1)))
  assert np.abs(A1[2, row]).max() < 1e-7 * np.abs(A1[2]).max()
  y0 = np.zeros((nb, r))
  want = np.einsum("bij,bj->bi", A1, x1) + np.einsum("bij,bj->bi", A2, x2)
  y, _ = rk.block_apply(A1, A2, x1, x2, y0, 1.0, 0.0, drop=(2, row))
  assert rel_err(y, want) < 1e-13
  with capsys.disabled():
    assert _exceeds("d", rk.block_fraction(y, A1, A2, x1, x2, y0, 1.0, 0.0), ("block",)) > 1.0


def test_mutant_e_neighbours_resistance(capsys):
  for nb, n_b in PRESENT_PC:
    Mb, K, Min = _present_pc_inputs(nb, n_b)
    _present_pc_assertions(_neighbour_mutant(Min, K, n_b), Mb, K)
  with capsys.disabled():
    for fam, n_b, bnd in (("bent", 22, "wall"), ("dense", 10, "none")):
      Ms, Ks = rk.launch(fam, n_b, bnd)
      o = _neighbour_mutant(Ms, Ks, n_b)
      one = {k: v[1] for k, v in o.items() if k != "info"}
      f = rk.factor_fractions(one, Ms[1], Ks[1])
      assert _exceeds("e", f["a12"], ("a12", rk.kernel_of(n_b))) > 1.0


def test_advance_keeps_the_rotation_when_the_squares_underflow():
  """|omega dt| = 1e-200: p.p underflows to 0; the rotation quaternion is (1, p / 2), not (1, 0)"""
  loc, quat, Uv, dt = np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0, 0.0]]), np.array([[0, 0, 0, 6e-201, 0.0, 8e-201]]), 1.0
  _, q, _, _ = rk.advance(loc, quat, Uv, dt)
  assert np.array_equal(q[0], [1.0, 3e-201, 0.0, 4e-201])
  Uv[0, 3:] = 0.0
  quat = rk.unit_quaternions(np.random.RandomState(0), 1)
  assert np.array_equal(rk.advance(loc, quat, Uv, dt)[1], quat)
