"""Restatement of the tabulated pair law (rigidmultiblobswall_amd/pair_table.py, include/rmb_mobility.h) in a dtype of
choice, the per-pair scales its rounding bounds are stated against, and the designed tables, ladders and clouds -- TEST
infrastructure.  The reference has no table law: this restatement of the definition is the oracle.

  r0 <= r < r_cut:  x = (r - r0)(1/h), k = min(floor(x), K - 1), t = x - k, Horner in t
                    U = c0 + t (c1 + t (c2 + t c3)),   U' = (c1 + t (2 c2 + 3 t c3))/h
  r < r0:           U = c[0][0] + x c[0][1],           U' = c[0][1]/h
  r >= r_cut:       U = U' = 0                         (r_cut: the fp64 number r0 + K h the table carries)
  force on i:       sum_j U'(r) min(1/r, 1e25) d,  d = r_j - r_i, minimal image in every direction with L > 0
  energy:           sum_{i<j, z_i > 0} U(r),  minimal image in x and y only (the blob forms' rule and wall gate)
  minimal image     d - trunc(d/L + sign(d)/2) L, as the kernels and the oracle do it.

The four fp64 coefficients are the law; they enter every dtype exactly.  With dtype = EXT (np.longdouble) the separations of
the fp64 positions are exact.  Scales, per pair, in EXT:

    S_U = |c0| + t (|c1| + t (|c2| + t |c3|)) + r |U'(r)|
    S_F = (|c1| + t (2 |c2| + 3 t |c3|))/h + r |U''(r)|,       U'' = (2 c2 + 6 t c3)/h^2

S_F enters blob i, component k with the weight |d_k| min(1/r, 1e25); the energy's scale is the sum over its pairs.  The last
term of each is the conditioning on r (one rounding of r moves the value by r |dU/dr| units); it also covers an interval
chosen differently at a knot, the interpolant being C^1 there up to one rounding of the coefficients.  Nothing covers a
pair that one side takes for r < r_cut and the other does not when the table does not end at zero: the cloud builder
keeps every pair 1e-9 r_cut away from r_cut and asserts it.

    |got - EXT| <= MARGIN * C[family, periodic] * 2^-53 * S            MARGIN = _mobility_numpy.MARGIN = 4

C: the worst ratio of THIS restatement in float64 against itself in EXT on the designed ladders and clouds, measured on the
CPU by tests/test_pair_table_host.py, which asserts measured <= stored <= 2 measured + 1.  Regenerate with
    python -m pytest tests/test_pair_table_host.py -k yardstick -s
It comes from the restatement only, never from a kernel.

In a box a raw separation x_j - x_i is rounded once in fp64 at the size of the raw separation, which no multiple of the
scales above covers for a close pair many cells apart.  The box clouds and ladders are therefore built so that every raw
separation and every image is exact: coordinates on the grid 2^-20, periods that are powers of two."""
import numpy as np

import _potential_numpy as pn
from _mobility_numpy import EXT, LONG_DOUBLE, MARGIN      # noqa: F401
from rigidmultiblobswall_amd.pair_table import PairTable, lennard_jones, yukawa

EPS64 = 2.0 ** -53
# (family, periodic) -> worst |float64 - EXT| / (2^-53 S), rounded up
C = {("force", False): 3.0, ("force", True): 3.0, ("energy", False): 3.0, ("energy", True): 3.0}
C_MEASURED = {("force", False): 2.331, ("force", True): 2.331, ("energy", False): 2.264, ("energy", True): 2.264}
_cache = {}


# ---------------------------------------------------------------------------------------------------------------------
# the law
# ---------------------------------------------------------------------------------------------------------------------
def radial(T, r, dtype=EXT):
  """(U, dU, S_U, S_F) of the distances r (array of `dtype`); the scales in EXT."""
  r = np.asarray(r, dtype=dtype)
  K = T.K
  inv_h = dtype(1) / dtype(T.h)
  with np.errstate(invalid="ignore", over="ignore"):
    x = (r - dtype(T.r0)) * inv_h
    xc = np.clip(np.where(np.isnan(x), dtype(0), x), dtype(0), dtype(K))
    k = np.minimum(np.floor(xc), K - 1).astype(np.int64)
    t = xc - k.astype(dtype)
    c = T.coeff[k].astype(dtype)
    lead = np.where(x < 0, x, t)
    inside = r < dtype(T.r_cut)
    U = np.where(inside, c[..., 0] + lead * (c[..., 1] + t * (c[..., 2] + t * c[..., 3])), dtype(0))
    dU = np.where(inside, (c[..., 1] + t * (dtype(2) * c[..., 2] + dtype(3) * t * c[..., 3])) * inv_h, dtype(0))
    # scales: always in EXT, from the EXT location of r
    rE = r.astype(EXT)
    hE = EXT(T.h)
    xE = (rE - EXT(T.r0)) / hE
    xcE = np.clip(np.where(np.isnan(xE), EXT(0), xE), EXT(0), EXT(K))
    kE = np.minimum(np.floor(xcE), K - 1).astype(np.int64)
    tE = xcE - kE
    a = np.abs(T.coeff[kE].astype(EXT))
    cE = T.coeff[kE].astype(EXT)
    core = xE < 0
    dUE = (cE[..., 1] + tE * (2 * cE[..., 2] + 3 * tE * cE[..., 3])) / hE
    d2UE = np.where(core, EXT(0), (2 * cE[..., 2] + 6 * tE * cE[..., 3]) / (hE * hE))
    leadE = np.where(core, np.abs(xE), tE)
    insideE = rE < EXT(T.r_cut)
    S_U = np.where(insideE, a[..., 0] + leadE * (a[..., 1] + tE * (a[..., 2] + tE * a[..., 3])) + rE * np.abs(dUE), EXT(0))
    S_F = np.where(insideE, (a[..., 1] + tE * (2 * a[..., 2] + 3 * tE * a[..., 3])) / hE + rE * np.abs(d2UE), EXT(0))
  return U, dU, S_U, S_F


def _period(L):
  return np.zeros(3) if L is None else np.asarray(L, dtype=np.float64).reshape(3)


def _image(d, L, dtype, dims):
  for k in dims:
    if L[k] > 0:
      Lk = dtype(L[k])
      d[..., k] = d[..., k] - np.trunc(d[..., k] / Lk + dtype(0.5) * np.sign(d[..., k])) * Lk
  return d


def _rows(x, L, lo, hi, dtype, dims):
  """d[i, j] = r_j - r_i (minimal image) and r of rows lo..hi; own entries at r = inf."""
  d = _image((x[None, :, :] - x[lo:hi, None, :]).astype(dtype), L, dtype, dims)
  r = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
  r[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
  return d, r


def _near(T, x64, L, lo, hi, dims):
  """(i, j) of the ordered pairs of rows lo..hi within 1.001 r_cut, from a float64 first pass: every other pair is beyond the
  reach in any precision and contributes nothing to a sum or a scale.  Then d and r of those pairs in `dtype`."""
  _, r64 = _rows(x64, L, lo, hi, np.float64, dims)
  ii, jj = np.nonzero(r64 < 1.001 * T.r_cut)
  return ii + lo, jj


def _pairs(x, L, ii, jj, dtype, dims):
  d = _image((x[jj] - x[ii]).astype(dtype), L, dtype, dims)
  return d, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def forces(T, r, L=None, dtype=EXT, block=256):
  """(F, S): (N, 3) forces of the table in `dtype` arithmetic and their scales in EXT."""
  L = _period(L)
  x64 = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  x = x64.astype(dtype)
  n = len(x)
  F = np.zeros((n, 3), dtype=dtype)
  S = np.zeros((n, 3), dtype=EXT)
  for lo in range(0, n, block):
    ii, jj = _near(T, x64, L, lo, min(n, lo + block), (0, 1, 2))
    if not len(ii):
      continue
    d, rr = _pairs(x, L, ii, jj, dtype, (0, 1, 2))
    _, dU, _, S_F = radial(T, rr, dtype)
    with np.errstate(divide="ignore"):
      ir = np.minimum(dtype(1) / rr, dtype(1e25))
    np.add.at(F, ii, (dU * ir)[:, None] * d)
    np.add.at(S, ii, (S_F * ir.astype(EXT))[:, None] * np.abs(d).astype(EXT))
  return F, S


def energy(T, r, L=None, dtype=EXT, block=256):
  """(U_pair, S): sum over i < j with z_i > 0, minimal image in x and y; the scale in EXT."""
  L = _period(L)
  x64 = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  x = x64.astype(dtype)
  n = len(x)
  U, S = dtype(0), EXT(0)
  for lo in range(0, n, block):
    ii, jj = _near(T, x64, L, lo, min(n, lo + block), (0, 1))
    keep = (jj > ii) & (x64[ii, 2] > 0)
    ii, jj = ii[keep], jj[keep]
    if not len(ii):
      continue
    _, rr = _pairs(x, L, ii, jj, dtype, (0, 1))
    u, _, S_U, _ = radial(T, rr, dtype)
    U = U + u.sum(dtype=dtype)
    S = S + S_U.sum(dtype=EXT)
  return U, S


def one_blob(z, eps_w, b_w, weight, a, form):
  """(U_one, S_one) in EXT: tests/_potential_numpy.one_blob_terms (blobs with z <= 0: 1e5 (1 - z))."""
  u1 = pn.one_blob_terms(np.asarray(z, dtype=np.float64), EXT(eps_w), EXT(b_w), EXT(weight), EXT(a), form)
  return u1.sum(dtype=EXT), np.abs(u1).sum(dtype=EXT)


def pair_distances(r, L=None, dims=(0, 1, 2)):
  """(N, N) distances in float64 from EXT; inf on the diagonal."""
  x = np.asarray(r, dtype=np.float64).reshape(-1, 3).astype(EXT)
  n = len(x)
  R = np.empty((n, n))
  for lo in range(0, n, 256):
    hi = min(n, lo + 256)
    R[lo:hi] = _rows(x, _period(L), lo, hi, EXT, dims)[1].astype(np.float64)
  return R


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def ratios(got, ref, S, c):
  """|got - EXT| / (c 2^-53 S) per entry (float64); inf where S = 0 and got differs."""
  err = np.abs(np.asarray(got).astype(EXT) - ref)
  den = EXT(c) * EXT(EPS64) * np.asarray(S, dtype=EXT)
  with np.errstate(divide="ignore", invalid="ignore"):
    q = np.where(err == 0, EXT(0), np.where(den > 0, err / den, EXT(np.inf)))
  return np.asarray(q, dtype=np.float64)


def worst(got, ref, S, c):
  q = np.atleast_1d(ratios(got, ref, S, c))
  return float(q.max())


def is_positive_zero(x):
  return not np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64).any()


# ---------------------------------------------------------------------------------------------------------------------
# designed tables
# ---------------------------------------------------------------------------------------------------------------------
LJ = dict(eps=1.0, sigma=1.0, r0=0.875, r_cut=2.5)     # r0 h and the knots of K = 1, 2, 16 are exact binary numbers
K_LIST = (1, 2, 16, 1024)


def lj_table(K, shift="force"):
  key = ("lj", K, shift)
  if key not in _cache:
    U, dU = lennard_jones(LJ["eps"], LJ["sigma"])
    _cache[key] = PairTable.from_function(U, dU, LJ["r0"], LJ["r_cut"], K, shift=shift)
  return _cache[key]


YUK = dict(eps=1.0, b=0.5, r0=0.5, r_cut=8.0, K=1024)


def yukawa_table(shift="force"):
  key = ("yuk", shift)
  if key not in _cache:
    U, dU = yukawa(YUK["eps"], YUK["b"])
    _cache[key] = PairTable.from_function(U, dU, YUK["r0"], YUK["r_cut"], YUK["K"], shift=shift)
  return _cache[key]


def yukawa_d4_max():
  """max |U''''| of eps exp(-r/b)/r on [r0, r_cut]: at r0 (every term of the derivative decays).
  U'''' = eps e^{-r/b} (1/(b^4 r) + 4/(b^3 r^2) + 12/(b^2 r^3) + 24/(b r^4) + 24/r^5)."""
  e, b, r = EXT(YUK["eps"]), EXT(YUK["b"]), EXT(YUK["r0"])
  return e * np.exp(-r / b) * (1 / (b ** 4 * r) + 4 / (b ** 3 * r ** 2) + 12 / (b ** 2 * r ** 3) + 24 / (b * r ** 4) + 24 / r ** 5)


# ---------------------------------------------------------------------------------------------------------------------
# N = 2 ladder
# ---------------------------------------------------------------------------------------------------------------------
LADDER_BOX = np.array([16.0, 16.0, 0.0])
RUNGS = ("zero", "half_r0", "r0", "in_first", "knot", "knot-ulp", "knot+ulp", "in_last", "below_cut", "cut", "beyond")


def ladder_distance(T, rung):
  K, r0, h, rc = T.K, T.r0, T.h, T.r_cut
  knot = r0 + (K // 2) * h if K > 1 else r0 + h          # K = 1: the only knots are the ends; r_cut is met from below
  return {"zero": 0.0, "half_r0": 0.5 * r0, "r0": r0, "in_first": r0 + 0.37 * h, "knot": knot,
          "knot-ulp": np.nextafter(knot, 0.0), "knot+ulp": np.nextafter(knot, np.inf), "in_last": rc - 0.41 * h,
          "below_cut": np.nextafter(rc, 0.0), "cut": rc, "beyond": 1.5 * rc}[rung]


def ladder_pair(T, rung, box=False):
  """Two blobs along x at the rung's distance, above z = 0; box: LADDER_BOX, the second blob one period back in y (exact)."""
  r = np.array([[0.0, 0.0, 1.0], [ladder_distance(T, rung), 0.0, 1.0]])
  if box:
    r[1, 1] -= LADDER_BOX[1]
  return r, (LADDER_BOX.copy() if box else None)


# ---------------------------------------------------------------------------------------------------------------------
# clouds
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (65, 129, 2113)
N_LONERS = 5
GRID = 2.0 ** -20
VARIANTS = {"open": 0, "box": 2, "box3": 3}      # periodic directions


def _build(size, variant, T):
  """A jittered lattice at the density of the table (spacing ~ 1.05 sigma: pairs inside r0, in every part of the reach and
  beyond it), 3 blobs moved next to others to sit inside r0, N_LONERS blobs beyond r_cut of everything.  2113: a monolayer
  listed at random (33 tiles: the Morton sort and the culling are live)."""
  rng = np.random.RandomState(4100 + size)
  n_core = size - N_LONERS
  rc = T.r_cut
  if size >= 2048:
    m = int(np.ceil(np.sqrt(n_core)))
    shape = (m, m, 1)
  else:
    m = int(np.ceil(n_core ** (1.0 / 3.0)))
    shape = (m, m, m)
  g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3).astype(float)
  core = g[rng.permutation(len(g))[:n_core]] * 1.05 + 0.12 * (2.0 * rng.rand(n_core, 3) - 1.0)
  core -= core.min(axis=0)
  core[:, 2] += 0.75
  for k in range(3):        # pairs inside r0: blob k moved to 0.5 .. 0.9 r0 of blob k + 3
    u = rng.randn(3)
    u[2] = abs(u[2])
    core[k] = core[k + 3] + (0.5 + 0.2 * k) * T.r0 * u / np.linalg.norm(u)
  hi = core.max(axis=0)
  lon = np.zeros((N_LONERS, 3))
  lon[:, 0] = hi[0] + 1.5 * rc + 1.5 * rc * np.arange(N_LONERS)
  lon[:, 1] = 0.3
  lon[:, 2] = 0.75
  r = np.concatenate([core, lon])
  if size >= 2048:
    r = r[rng.permutation(len(r))]
  r = np.round(r / GRID) * GRID
  L = None
  periods = VARIANTS[variant]
  if periods:
    ext = r.max(axis=0) - r.min(axis=0)
    L = 2.0 ** np.ceil(np.log2(ext + 1.5 * rc))      # the loners stay beyond r_cut of every image
    if periods == 2:
      L[2] = 0.0
    shift = np.random.RandomState(77 + size).randint(-2, 3, size=(len(r), 3))
    r = r + shift * L[None, :]                        # exact: grid numbers, power-of-two periods, |r| < 2^12
    assert np.all(np.round(r / GRID) * GRID == r)
  return np.ascontiguousarray(r), L


def coverage(T, r, L, dims=(0, 1, 2)):
  R = pair_distances(r, L, dims)
  cnt = lambda m: int(np.count_nonzero(m))      # noqa: E731
  x = (R - T.r0) / T.h
  c = {"core": cnt(R < T.r0), "beyond": cnt((R >= T.r_cut) & np.isfinite(R)), "inside": cnt((R >= T.r0) & (R < T.r_cut)),
       "intervals": len(np.unique(np.floor(x[(x >= 0) & (x < T.K)]))), "coincident": cnt(R == 0),
       "loners": cnt(R.min(axis=1) >= T.r_cut), "near_cut": cnt(np.abs(R - T.r_cut) < 1e-9 * T.r_cut)}
  return c


def assert_coverage(T, c):
  want = min(T.K, 16)
  assert c["core"] >= 2 and c["beyond"] >= 2 and c["inside"] >= 2 and c["intervals"] >= want, c
  assert c["loners"] >= 4 and c["coincident"] == 0 and c["near_cut"] == 0, c


def cloud(size, variant="open", T=None):
  """(r, L) of a designed cloud, its coverage asserted once (for the force's images and for the energy's)."""
  T = T or lj_table(1024)
  key = ("cloud", size, variant, T.K)
  if key not in _cache:
    r, L = _build(size, variant, T)
    assert_coverage(T, coverage(T, r, L))
    if variant != "box3":
      assert_coverage(T, coverage(T, r, L, (0, 1)))
    _cache[key] = (r, L)
  return _cache[key]


def loners(T, r, L, dims=(0, 1, 2)):
  return np.nonzero(pair_distances(r, L, dims).min(axis=1) >= T.r_cut)[0]


def force_reference(T, size, variant, tag="lj"):
  key = ("fref", tag, T.K, size, variant)
  if key not in _cache:
    r, L = cloud(size, variant)
    _cache[key] = forces(T, r, L)
  return _cache[key]


def energy_reference(T, size, variant, tag="lj"):
  key = ("eref", tag, T.K, size, variant)
  if key not in _cache:
    r, L = cloud(size, variant)
    _cache[key] = energy(T, r, L)
  return _cache[key]
