"""The extended-precision restatement of the pair blocks (tests/_mobility_numpy.py) against everything that pins it on the
CPU: the fp64 oracle block by block, the oracle's pseudo-periodic and free-surface products, the reference's golden
vectors -- and the yardsticks C_ORACLE / C_ORACLE32 that tests/test_gpu_pair_blocks.py holds the HIP kernels to, measured
here from the reference side alone.

Units: one rounding unit of a block element is 2^-53 s_ij (2^-24 s_ij in single precision) with the scale s_ij of
_mobility_numpy.scale.  Two fp64 evaluations of the same formulas that are each within C of the exact value are within 2 C
of each other: that is the bound of the oracle comparisons ("a few rounding units": C is 7 to 25)."""
import os

import numpy as np
import pytest

import _mobility_numpy as mn
from _mobility_numpy import A, ETA, EXT
from conftest import KERNEL_KEYS, golden_files, load_golden, rel_err

EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24
BOUNDARIES = ("none", "wall", "free")
# source blobs whose columns the pseudo-periodic oracle comparisons extract (a product per column: 5 ms each)
N_COLS_PERIODIC, N_COLS_PERIODIC_FREE = 40, 16


def test_long_double_is_the_extended_format():
  """No skip and no fallback: with a 53-bit long double the GPU test would compare fp64 with fp64 unnoticed."""
  import platform
  if platform.machine() in ("x86_64", "AMD64"):
    assert mn.LONG_DOUBLE and mn.EXT is np.longdouble and np.finfo(np.longdouble).nmant >= 63
  assert mn.LONG_DOUBLE, "np.longdouble has no 64-bit mantissa here: the element-wise block tests have no yardstick"


@pytest.mark.parametrize("name", sorted(mn.CLOUDS))
def test_regime_cloud_holds_every_class(name):
  periodic, offset, classes = mn.CLOUDS[name]
  r, L = mn.regime_cloud(A, periodic, offset)
  assert r.shape == (mn.N_CLOUD, 3) and mn.N_CLOUD % 64 != 0 and mn.N_CLOUD > 3 * 64
  c = mn.assert_coverage(r, A, L, classes)
  assert all(c[k] >= 1 for k in classes)
  # the wall clamp must not create coincident blobs either
  x = r.copy(); x[:, 2] = mn.wall_heights(r, A)[0]
  assert mn.coverage(x, A, L)["exactly_coincident"] == 0
  if periodic:
    assert (L[0] == 2.0 ** round(np.log2(L[0]))) == (periodic == "pow2")


def test_tie_check_rebuilds_a_tied_input():
  L = np.array([8.0, 6.0, 0.0])
  r = np.array([[0.25, 0.5, 1.0], [4.25, 0.7, 2.0], [1.0, 3.5, 1.0], [7.0, 1.0, 1.5]])      # 0-1 tie in x, 0-2 in y
  assert mn.ties(r, L) == 2
  with pytest.raises(AssertionError):
    mn.assert_coverage(r, A, L, ())
  fixed = mn.untie(r, L)
  assert mn.ties(fixed, L) == 0 and np.abs(fixed - r).max() <= 4e-8 * L.max()
  assert mn.ties(r + [0.0, 0.0, 0.0], None) == 0            # no periodic direction, no tie


# ---------------------------------------------------------------------------------------------------------------------
# 1. float64 restatement == the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _c(kind, boundary, periodic):
  return mn.C_ORACLE[kind, boundary, bool(periodic)]


@pytest.mark.parametrize("name", ["open", "offset"])
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("kind", mn.KINDS)
def test_float64_restatement_matches_oracle_dense(oracle, kind, boundary, name):
  r, L = mn.cloud(name)
  got = mn.blocks(kind, boundary, r, A, ETA, dtype=np.float64)
  ref = _oracle_blocks(oracle, name, kind, boundary)[0]
  ratio, i, j, c, d = mn.worst_ratio(got, ref.astype(EXT), mn.reference(name, kind, boundary)[1], EPS64)
  print("%s %s %s: restatement fp64 vs oracle %.2f units at pair (%d, %d) element (%d, %d)" % (name, kind, boundary, ratio, i, j, c, d))
  assert ratio <= 2 * _c(kind, boundary, False), (ratio, i, j, c, d, mn.regime_of(r, A, i, j))


def _periodic_cols(r, n_cols, L=None):
  """Source blobs of the column comparisons.  In a box: first the blobs whose separations are worst conditioned -- largest
  (one unit in the last place of the unwrapped difference) / (wrapped distance), where the fp64 wrap of the oracle loses
  most -- then seeded ones; open: seeded."""
  n = len(r)
  rng = np.random.RandomState(5)
  picks = []
  if L is not None:
    d = r[:, None, :] - r[None, :, :]
    w = d.copy()
    for k in range(3):
      if L[k] > 0:
        w[..., k] = d[..., k] - np.trunc(d[..., k] / L[k] + 0.5 * np.sign(d[..., k])) * L[k]
    dist = np.sqrt((w ** 2).sum(axis=2)) + np.eye(n)
    cond = (np.spacing(np.abs(d[..., :2]).max(axis=2)) * (np.abs(w - d).sum(axis=2) > 0)) / np.minimum(dist, A)
    picks = list(np.argsort(-cond.max(axis=0))[:n_cols // 2])
  rest = [j for j in rng.permutation(n) if j not in picks]
  return np.sort(np.array(picks + rest[:n_cols - len(picks)], dtype=np.int64))


_oracle_cache = {}


def _oracle_blocks(oracle, name, kind, boundary):
  """(oracle blocks, columns or None) of a cloud, once per process."""
  key = (name, kind, boundary)
  if key not in _oracle_cache:
    r, L = mn.cloud(name)
    cols = None if L is None else _periodic_cols(r, N_COLS_PERIODIC_FREE if boundary == "free" else N_COLS_PERIODIC, L)
    _oracle_cache[key] = (mn.oracle_blocks(oracle, kind, boundary, r, A, ETA, L, cols=cols), cols)
  return _oracle_cache[key]


@pytest.mark.parametrize("name", ["odd", "pow2"])
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("kind", mn.KINDS)
def test_float64_restatement_matches_oracle_products_periodic(oracle, kind, boundary, name):
  """Pseudo-periodic: the oracle has no dense builder, so its products on unit vectors (columns, exact extraction) and on
  one random vector.  For the random vector both sides sum 3N terms in different orders: each sum is off by at most
  3N 2^-53 sum |terms|, |term| <= 2 s_ij |v_j| -- (2 C + 12 N) units of sum_j s_ij |v_j|_1, a coarse bound that still
  sees a wrong image, sign or box (those are O(1))."""
  r, L = mn.cloud(name)
  n = len(r)
  got = mn.blocks(kind, boundary, r, A, ETA, L, dtype=np.float64)
  ref, cols = _oracle_blocks(oracle, name, kind, boundary)
  s = mn.reference(name, kind, boundary)[1]
  ratio, i, j, c, d = mn.worst_ratio(got[:, cols], ref.astype(EXT), s[:, cols], EPS64)
  assert ratio <= 2 * _c(kind, boundary, True), (ratio, i, cols[j], c, d, mn.regime_of(r, A, i, cols[j], L))
  v = np.random.RandomState(11).randn(3 * n)
  if boundary == "free":
    import _free_surface_mirror as mirror
    u = mirror.product(oracle, kind, r, v, ETA, A, L)
    if kind == "tt":
      assert rel_err(oracle.free_surface_mobility_trans_times_force_oracle(r, v, ETA, A, periodic_length=L), u) < 1e-13
  else:
    u = oracle._wrapped(kind, 1 if boundary == "wall" else 0, r, v, ETA, A, periodic_length=L)
  row = (s * np.abs(v.reshape(n, 3)).sum(axis=1)[None, :]).sum(axis=1)
  err = np.abs((mn.dense(got) @ v).reshape(n, 3).astype(EXT) - u.reshape(n, 3)) / (EPS64 * row[:, None])
  assert err.max() <= 2 * _c(kind, boundary, True) + 12 * n, err.max()


@pytest.mark.parametrize("kind", ["tt", "tr"])
def test_float64_restatement_matches_oracle_in_plane(oracle, kind):
  r, L = mn.cloud("open")
  cols = _periodic_cols(r, N_COLS_PERIODIC)
  got = mn.blocks(kind, "wall", r, A, ETA, dtype=np.float64, in_plane=True)
  ref = mn.oracle_blocks(oracle, kind, "wall", r, A, ETA, cols=cols, in_plane=True)
  ratio = mn.worst_ratio(got[:, cols], ref.astype(EXT), mn.reference("open", kind, "wall")[1][:, cols], EPS64)
  assert ratio[0] <= 2 * _c(kind, "wall", False), ratio
  full = mn.blocks(kind, "wall", r, A, ETA, dtype=np.float64)
  mask = mn._TT_MASK if kind == "tt" else mn._TR_MASK
  assert np.array_equal(got, np.where(mask, full, 0.0))           # the in-plane variant is the masked block, bit for bit


def test_free_surface_tt_columns_match_its_own_oracle_product(oracle):
  """The doubled-system form of oracle_blocks against the oracle's free-surface product (the reference's kernel), open box."""
  r, L = mn.cloud("open")
  n = len(r)
  D = mn.dense(mn.oracle_blocks(oracle, "tt", "free", r, A, ETA))
  s = mn.reference("open", "tt", "free")[1]
  e = np.zeros(3 * n)
  for k in (0, 17, 3 * n - 1, 301):
    e[k] = 1.0
    u = oracle.free_surface_mobility_trans_times_force_oracle(r, e, ETA, A)
    e[k] = 0.0
    # (B + I) v norm there, B norm + I norm here: both within C of the exact block
    assert np.all(np.abs(u - D[:, k]).reshape(n, 3) <= 2 * _c("tt", "free", False) * EPS64 * np.asarray(s[:, k // 3], dtype=np.float64)[:, None])


# ---------------------------------------------------------------------------------------------------------------------
# 2. EXT restatement == the reference's golden vectors
# ---------------------------------------------------------------------------------------------------------------------
_GOLDEN_KEYS = {"no_wall_tt": ("tt", "none", False), "wall_tt": ("tt", "wall", False), "in_plane_tt": ("tt", "wall", True),
                "no_wall_tr": ("tr", "none", False), "wall_tr": ("tr", "wall", False), "in_plane_tr": ("tr", "wall", True),
                "no_wall_rt": ("rt", "none", False), "wall_rt": ("rt", "wall", False), "no_wall_rr": ("rr", "none", False),
                "wall_rr": ("rr", "wall", False), "free_surface_tt": ("tt", "free", False)}
assert set(_GOLDEN_KEYS) == set(KERNEL_KEYS)


@pytest.mark.parametrize("path", golden_files("g[123]_*.npz"), ids=lambda p: os.path.basename(p)[:-4])
def test_ext_restatement_reproduces_the_reference_goldens(path):
  """The tolerance of test_gpu_parity.test_golden_vectors: 1e-12 on the well-separated wall cloud, 1e-10 on the dense and
  contact clouds (relative L2 of the product)."""
  g = load_golden(path)
  r, v, eta, a, L = g["r_vectors"], np.asarray(g["vector"], dtype=np.float64).reshape(-1), float(g["eta"]), float(g["a"]), g["periodic_length"]
  n = len(r)
  tol = 1e-12 if "wall_cloud" in path else 1e-10
  seen = 0
  for key, (kind, boundary, in_plane) in _GOLDEN_KEYS.items():
    if key not in g:
      continue
    u = np.empty(3 * n)
    for i0 in range(0, n, 250):          # rows in slabs: the N = 1000 fixture would need gigabytes at once
      rows = np.arange(i0, min(n, i0 + 250))
      M = mn.dense(mn.blocks(kind, boundary, r, a, eta, L, in_plane=in_plane, rows=rows))
      u[3 * i0:3 * rows[-1] + 3] = (M @ v.astype(EXT)).astype(np.float64)
    assert rel_err(u, g[key]) < tol, (key, rel_err(u, g[key]))
    seen += 1
  assert seen >= 2


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. the yardsticks
# ---------------------------------------------------------------------------------------------------------------------
def measure_c_oracle(oracle):
  out = {}
  for kind in mn.KINDS:
    for boundary in BOUNDARIES:
      for periodic, names in ((False, ("open", "offset")), (True, ("odd", "pow2"))):
        worst = 0.0
        for name in names:
          r, L = mn.cloud(name)
          E, s = mn.reference(name, kind, boundary)
          O, cols = _oracle_blocks(oracle, name, kind, boundary)
          if cols is not None:
            E, s = E[:, cols], s[:, cols]
          worst = max(worst, mn.worst_ratio(O, E, s, EPS64)[0])
        out[kind, boundary, periodic] = worst
  return out


def measure_c_oracle32():
  out = {}
  for kind in mn.KINDS:
    for boundary in BOUNDARIES:
      worst = 0.0
      for name in ("open", "offset"):
        r, L = mn.cloud(name)
        E, s = mn.reference(name, kind, boundary)
        worst = max(worst, mn.worst_ratio(mn.blocks(kind, boundary, r, A, ETA, dtype=np.float32), E, s, EPS32)[0])
      out[kind, boundary] = worst
  return out


def _print_table(title, table):
  print("\n%s = {" % title)
  for key in sorted(table):
    print("    %r: %.0f.0,      # measured %.2f" % (key, np.ceil(table[key]), table[key]))
  print("}")


def test_yardstick_c_oracle_does_not_exceed_the_committed_table(oracle):
  """C_oracle = max over elements of |oracle_fp64 - EXT| / (2^-53 s) per (kind, boundary, periodic), recomputed: the
  committed numbers are what the GPU test multiplies by MARGIN, so they may only be too large, never too small."""
  got = measure_c_oracle(oracle)
  _print_table("C_ORACLE", got)
  assert set(got) == set(mn.C_ORACLE)
  for key, val in got.items():
    assert np.isfinite(val) and val <= mn.C_ORACLE[key], (key, val, mn.C_ORACLE[key])
    assert mn.C_ORACLE[key] <= 2 * val + 2, (key, "the committed value is stale: far above what is measured", val)


def test_yardstick_c_oracle32_does_not_exceed_the_committed_table():
  """The same for the reference's `precision = 'single'` arithmetic (float32 on separations taken exactly from the float64
  positions), in units of 2^-24 s."""
  got = measure_c_oracle32()
  _print_table("C_ORACLE32", got)
  assert set(got) == set(mn.C_ORACLE32)
  for key, val in got.items():
    assert np.isfinite(val) and val <= mn.C_ORACLE32[key], (key, val, mn.C_ORACLE32[key])
    assert mn.C_ORACLE32[key] <= 2 * val + 2, (key, "the committed value is stale", val)


def test_ext_blocks_are_exact_where_the_value_is_known():
  """Closed forms: the self blocks, and the pair at r = 2a exactly along x (a = 1/2, d = (1, 0, 0)), no boundary:
  tt = (1/(8 pi eta a)) diag(7/12 + 1/8 ... ) -> far and near branch agree there, so either is the value."""
  r = np.array([[0.0, 0.0, 4.0], [1.0, 0.0, 4.0]])
  pref = 1 / (EXT(8) * EXT(mn._PI) * EXT(ETA))
  tt = mn.blocks("tt", "none", r, 0.5, ETA)
  assert abs(tt[0, 0, 0, 0] - pref * EXT(4) / EXT(3) / EXT(0.5)) <= 2.0 ** -62 * float(tt[0, 0, 0, 0])
  # units of a: c1 = 7/12, c2 r_x^2 = (1/16) 4 = 1/4 -> xx = 5/6, yy = 7/12
  assert abs(tt[0, 1, 0, 0] - pref * EXT(5) / EXT(6) / EXT(0.5)) <= 2.0 ** -61 * float(tt[0, 1, 0, 0])
  assert abs(tt[0, 1, 1, 1] - pref * EXT(7) / EXT(12) / EXT(0.5)) <= 2.0 ** -61 * float(tt[0, 1, 1, 1])
  rr = mn.blocks("rr", "none", r, 0.5, ETA)
  assert abs(rr[1, 1, 2, 2] - pref / EXT(0.125)) <= 2.0 ** -62 * float(rr[1, 1, 2, 2])
  # far rr at r = 2: (-1/2 + (3/2) r_x^2/r^2)/r^3 = 1/8 along x, -1/16 across
  assert abs(rr[0, 1, 0, 0] - pref / EXT(8) / EXT(0.125)) <= 2.0 ** -61 * float(rr[0, 1, 0, 0])
  assert abs(rr[0, 1, 1, 1] + pref / EXT(16) / EXT(0.125)) <= 2.0 ** -61 * float(rr[0, 1, 0, 0])
  tr = mn.blocks("tr", "none", r, 0.5, ETA)
  # eps.r / r^3: d = r_0 - r_1 = (-2, 0, 0) in units of a -> M[1, 2] = r_x / r^3 = -1/4
  assert abs(tr[0, 1, 1, 2] + pref / EXT(4) / EXT(0.25)) <= 2.0 ** -61 * float(abs(tr[0, 1, 1, 2]))
