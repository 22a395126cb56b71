"""The yardstick of the Krylov step kernels on the CPU (tests/_krylov_numpy.py): the table C is current, the fp64
restatement is exact on the exact basis, and the mutant table -- three defects of the fused Gram-Schmidt step pass every
assertion the orthonormal-basis test makes, all five exceed the new bounds more than tenfold on the designed basis."""
import os
import re

import numpy as np
import pytest

import _krylov_numpy as kn
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not kn.LONG_DOUBLE, reason="needs an 80-bit long double")

NEW_ENTRIES = ("rmb_krylov_orthogonalize3_device", "rmb_rigid_arnoldi_step2_device", "rmb_rigid_lanczos_step_device", "rmb_lanczos_step_device",
               "rmb_krylov_lincomb_device", "rmb_krylov_norm_device")


def _merge(worst, f, where):
  for k, x in f.items():
    if x > worst.get(k, (-1.0, None))[0]:
      worst[k] = (x, where)


def _measure():
  worst = {}
  for n, rows, kind in kn.ortho_cases():
    V, w0 = kn.ortho_case(n, rows, kind)
    ref = kn.reference(V[:rows], w0)
    for ls in (False, True):
      _merge(worst, kn.model_fractions(V[:rows], w0, ls, kind == "a", ref=ref)[0], ("ortho", n, rows, kind, ls))
  for nb, r1, r2 in kn.PC_SHAPES:
    n = nb * (r1 + r2)
    for rows in kn.PC_ROWS[(nb, r1, r2)]:
      for kind in ("a", "b", "d"):
        if kind == "d" and rows == 1:
          continue
        V, w0 = kn.ortho_case(n, rows, kind)
        ref = kn.reference(V[:rows], w0)
        for ls in (False, True):
          _merge(worst, kn.model_fractions(V[:rows], w0, ls, kind == "a", ref=ref)[0], ("pc", nb, r1, r2, rows, kind, ls))
  for delta in kn.LADDER_DELTAS:
    V, w0 = kn.ladder_case(delta)
    ref = kn.reference(V[:kn.LADDER_ROWS], w0)
    for ls in (False, True):
      _merge(worst, kn.model_fractions(V[:kn.LADDER_ROWS], w0, ls, True, ref=ref)[0], ("ladder", delta, ls))
  # the step entries' shapes on random vectors, first-pass partials per body / per tile (the low-synchronisation ending)
  for (n_b, nb), j in (((1, 132), 0), ((1, 132), 16), ((2, 66), 3), ((12, 33), 59), ((22, 18), 4), ((33, 12), 16), ((42, 10), 59), ((12, 256), 16)):
    for r2 in (6, 0):
      n, rows = nb * (3 * n_b + r2), j + 1
      for kind in ("a", "b", "d"):
        V, w0 = kn.ortho_case(n, rows, kind)
        f = kn.model_fractions(V[:rows], w0, True, kind == "a", parts1=kn.body_parts(nb, 3 * n_b, r2))[0]
        _merge(worst, f, ("step", n_b, nb, r2, j, kind))
  for N, j in ((129, 0), (193, 16), (16448, 4)):
    for kind in ("a", "b", "d"):
      V, w0 = kn.ortho_case(3 * N, j + 1, kind)
      _merge(worst, kn.model_fractions(V[:j + 1], w0, True, kind == "a", parts1=kn.tile_parts(N))[0], ("plain", N, j, kind))
  for k in kn.LINCOMB_K:
    for n in kn.LINCOMB_N:
      V, coef, y0 = kn.lincomb_case(k, n)
      _merge(worst, {"lincomb": kn.lincomb_fraction(kn.lincomb(y0, V, coef)[0], y0, V, coef)}, ("lincomb", k, n))
  for n in kn.VNORM_N:
    for flat in (False, True):
      v = kn.vnorm_case(n, flat)
      _merge(worst, {"vnorm": kn.vnorm_fraction(kn.vnorm_model(v), v)}, ("vnorm", n, flat))
  return worst


def test_table_is_current():
  """C is what the fp64 restatement reaches over the cases of the GPU tests: not exceeded, and not stale by more than 2 %
  (the table rounds up)."""
  worst = _measure()
  print()
  for k in sorted(worst):
    print("    %-13s %-8.3g # measured %.4f at %s" % ('"%s":' % k, kn.C[k], worst[k][0], worst[k][1]))
  assert sorted(worst) == sorted(kn.C)
  for k, (x, where) in worst.items():
    assert x <= kn.C[k] and kn.C[k] <= 1.02 * x + 1e-3, (k, x, kn.C[k], where)
    assert 0.0 < kn.bound(k) <= 1.0


def _existing_assertions(V, w0, rows, m):
  """every assertion tests/test_gpu_krylov.py::test_fused_gram_schmidt_matches_two_classical_passes makes, on a model run m"""
  Vj = V[:rows]
  h = Vj @ w0
  w1 = w0 - Vj.T @ h
  h2 = Vj @ w1
  w2 = w1 - Vj.T @ h2
  nrm = float(np.linalg.norm(w2))
  return (rel_err(m["col"], h + h2) < 1e-12 and abs(float(m["nrm"]) - nrm) <= 1e-12 * max(nrm, 1.0) and rel_err(m["w"], w2) < 1e-9 and
          rel_err(m["v"], w2 / nrm) < 1e-9 and float(np.abs(Vj @ m["v"]).max()) < 1e-12 and abs(float(np.linalg.norm(m["v"])) - 1.0) < 1e-13)


@pytest.mark.parametrize("n,rows", [(2688, 17), (4608, 60), (1025, 7)])
def test_three_defects_pass_every_assertion_of_the_orthonormal_test(n, rows):
  """The gap: on a QR-orthonormal basis each classical pass repairs the other.  A dropped first-pass partial (what a wrong
  n_part1, a stale per-body partial or a wrong tile index causes), no second pass at all, and the norm taken from w1 all pass
  the existing assertions; a dropped SECOND-pass partial does not (the control)."""
  rng = np.random.RandomState(n + rows)
  V = kn.basis("a", rows, n, rng)
  w0 = rng.randn(n)
  n_chunks = kn.layout(n)[1]
  assert _existing_assertions(V, w0, rows, kn.gram_schmidt(V[:rows], w0))
  for mutant in (("drop1", n_chunks // 2), "no_pass2", "norm_w1"):
    for ls in (False, True):
      assert _existing_assertions(V, w0, rows, kn.gram_schmidt(V[:rows], w0, low_sync=ls, mutant=mutant)), (mutant, ls)
  bodies = kn.body_parts(n // 42, 36, 6) if n % 42 == 0 else None
  if bodies:
    assert _existing_assertions(V, w0, rows, kn.gram_schmidt(V[:rows], w0, low_sync=True, parts1=bodies, mutant=("drop1", 3)))
  # control: pass 2 has nobody behind it
  Vj = V[:rows]
  w1 = w0 - Vj.T @ (Vj @ w0)
  m = kn.gram_schmidt(Vj, w0)
  chunk = kn.chunk_parts(n)[n_chunks // 2]
  m["col"] = m["col"] - Vj[:, chunk] @ w1[chunk]
  assert not _existing_assertions(V, w0, rows, m)


def _parity_excess(f):
  return max(f[k] / kn.bound(k) for k in f)


def test_all_five_defects_exceed_the_new_bounds_tenfold_on_the_designed_basis():
  """Basis (b), rows (q_r + 0.3 q_{r+1}) normalised: every defect is off by many orders of magnitude of the bound, in both
  forms, at every shape on which the defect changes anything ("clamp" needs a last row group of two or three rows).  The
  norm of the low-synchronisation ending is pinned on basis (d), coupling 0.01: its bound carries the basis's own defect
  |V V^T - I|_2 |h2|^2, which on (b) is of the size of the term the mutant leaves out.  Basis (d) catches the others too."""
  seen = set()
  for n, rows, kind in kn.ortho_cases():
    if kind == "a" or n > 65537 or rows == 1:      # (one normalised row is an orthonormal basis: nothing designed about it)
      continue
    V, w0 = kn.ortho_case(n, rows, kind)
    ref = kn.reference(V[:rows], w0)
    n_parts = kn.layout(n)[1]
    mutants = [("drop1", n_parts // 2), "no_pass2", "norm_w1", "skip"] + (["clamp"] if rows % 4 in (2, 3) else [])
    for ls in (False, True):
      clean, _ = kn.model_fractions(V[:rows], w0, ls, False, ref=ref)
      assert _parity_excess(clean) <= 1.0
      for mutant in mutants:
        if mutant == "norm_w1" and ls and kind == "b":
          continue
        f, _ = kn.model_fractions(V[:rows], w0, ls, False, mutant=mutant, ref=ref)
        assert _parity_excess(f) > 10.0, (n, rows, kind, ls, mutant, f)
        seen.add((mutant if isinstance(mutant, str) else mutant[0], ls))
  assert seen == {(m, ls) for m in ("drop1", "no_pass2", "norm_w1", "skip", "clamp") for ls in (False, True)}
  # per-body and per-tile first-pass partials (the step entries)
  for parts, n in ((kn.body_parts(12, 63, 6), 12 * 69), (kn.body_parts(33, 36, 0), 33 * 36), (kn.tile_parts(193), 579)):
    V, w0 = kn.ortho_case(n, 17, "b")
    ref = kn.reference(V[:17], w0)
    for k in (0, len(parts) - 1):
      f, _ = kn.model_fractions(V[:17], w0, True, False, parts1=parts, mutant=("drop1", k), ref=ref)
      assert _parity_excess(f) > 10.0, (n, k, f)
  # the linear combination: a coefficient skipped at the unroll boundary
  for k in kn.LINCOMB_K:
    V, coef, y0 = kn.lincomb_case(k, 257)
    assert kn.lincomb_fraction(kn.lincomb(y0, V, coef)[0], y0, V, coef) <= kn.bound("lincomb")
    assert kn.lincomb_fraction(kn.lincomb(y0, V, coef, skip=kn.unroll_edge(k) if k >= 8 else k - 1)[0], y0, V, coef) > 10.0 * kn.bound("lincomb")


def test_a_dropped_element_shows_in_the_norm_of_a_flat_vector():
  """vec_norm_kernel's yardstick: on standard normals leaving out one element (the last, the first of the second round of
  1024 threads) exceeds the bound tenfold; on the 300-decade vectors one or two entries carry the norm and it need not."""
  for n in kn.VNORM_N:
    if n < 255:
      continue
    v = kn.vnorm_case(n, flat=True)
    assert kn.vnorm_fraction(kn.vnorm_model(v), v) <= kn.bound("vnorm")
    for drop in (n - 1, min(1024, n - 2)):
      assert kn.vnorm_fraction(kn.vnorm_model(np.delete(v, drop)), v) > 10.0 * kn.bound("vnorm"), (n, drop)


@pytest.mark.parametrize("n,rows", kn.EXACT_SHAPES)
def test_the_restatement_is_exact_on_the_exact_basis(n, rows):
  """Basis (c): what the GPU test compares bitwise is what the algorithm gives in fp64, in both forms."""
  chunk, n_chunks = kn.layout(n)
  for last_free in (False, True):
    V, pos, free = kn.exact_basis(n, rows, last_free)
    assert len(set(pos)) == rows and not set(free) & set(pos) and V[:rows].sum() == rows and free[0] // chunk == 0
    assert ((n - 1) in set(pos)) != last_free and (not last_free or free[1] // chunk == n_chunks - 1)
    hots = kn.edge_one_hots(n, pos)
    assert {p // chunk for p, _ in hots} == set(range(n_chunks)) and len(hots) == 2 * n_chunks - (chunk * (n_chunks - 1) == n - 1)
    if n > 65537:
      continue        # the positions are checked; the fp64 run of a million columns adds nothing the smaller shapes do not show
    for name, w0, col, w_out, in_span in kn.exact_vectors(n, rows, pos, free):
      for ls in (False, True):
        m = kn.gram_schmidt(V[:rows], w0, low_sync=ls)
        assert np.array_equal(m["col"], col[:rows]) and m["nrm"] == col[rows] and np.array_equal(m["w"], w_out), (name, ls)
        if in_span:
          assert not np.isfinite(m["v"]).any()
        else:
          assert np.array_equal(m["v"], w_out / 5.0)
    if last_free:
      continue
    for p, r in hots:
      w0 = np.zeros(n)
      w0[p] = 7.0
      for ls in (False, True):
        m = kn.gram_schmidt(V[:rows], w0, low_sync=ls)
        col = np.zeros(rows)
        if r is not None:
          col[r] = 7.0
        assert np.array_equal(m["col"], col) and m["nrm"] == (0.0 if r is not None else 7.0), (p, r, ls)
        assert np.array_equal(m["w"], w0 if r is None else np.zeros(n)), (p, r, ls)
        assert np.array_equal(m["v"], w0 / 7.0) if r is None else not np.isfinite(m["v"]).any(), (p, r, ls)


def test_the_step_entries_are_declared_bound_and_exported():
  from rigidmultiblobswall_amd import _lib
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rmb_mobility.h")).read(), flags=re.S)
  lib = _lib.load()
  for name in NEW_ENTRIES:
    assert re.search(r"\bint %s\(" % name, src) and name in _lib.SYMBOLS and hasattr(lib, name), name
