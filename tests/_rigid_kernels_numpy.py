"""numpy restatement of the per-body kernels of the rigid-body solve (csrc/rmb_rigid.hip: rigid_config_kernel,
rigid_advance_kernel, rigid_pc_kernel for n = 3 n_b <= 48, rigid_pc_large_kernel for n <= 126) and of the batched two-by-two
block product (block_rows.h, rmb_block_apply_device) -- TEST infrastructure, shared by tests/test_rigid_kernels_host.py,
tests/test_gpu_rigid_kernels.py and tests/test_gpu_block_apply.py.

Every function takes dtype = np.float64 (the kernel's arithmetic, operation by operation, in the kernel's order up to the
partition of a dot product over lanes) or EXT (np.longdouble with a 64-bit mantissa: the reference).  Long-double sin / cos
/ sqrt are numpy's own long-double routines.

u = 2^-53, gamma_k = k u / (1 - k u).  Every check below produces a FRACTION: the worst residual over the elements of one
quantity divided by its derived bound (cw_ratio / the derived constant), evaluated in EXT from the kernel's fp64 outputs.

Factor kernels (derived constants; n = 3 n_b)
  chol    |L L^T - sym(M)| <= gamma_{n+1} |L||L^T|.  Right-looking Cholesky: element (i, j), j <= i, receives j subtractions
          of a product (2 roundings each, 1 with fma) and one division or square root: j + 1 <= n operations, each
          contributing at most u |L_ik||L_jk|; the symmetrisation 0.5 (M_ij + M_ji) adds one rounding of |sym M_ij| <=
          (|L||L^T|)_ij: n + 1 in all (Higham, Accuracy and Stability, thm 10.3).
  linv    small kernel: the rows of X = L^-1 come from forward substitution, (L^-1)[i][c] = (delta_ic - sum_{k=c}^{i-1}
          L[i][k] X[k][c]) / L[i][i]: column c of X solves L x = e_c, and substitution guarantees (L + dL_c) x_c = e_c,
          |dL_c| <= gamma_n |L| -- the LEFT residual |L X - I| <= gamma_n |L||X|.
          large kernel: in place from the last column, X[j+1:, j] = -X[j][j] (X[j+1:, j+1:] L[j+1:, j]): row i of the
          statement sum_{k=j}^{i} X[i][k] L[k][j] = delta_ij is an inner product of at most n terms with the finished part
          of ROW i of X -- the RIGHT residual |X L - I| <= gamma_n |X||L| (Higham 14.2.2, method 2 for a lower factor).
          Neither method bounds the other side without a factor cond(L).
  minv    |Minv - X^T X| <= gamma_n |X|^T|X|, X the kernel's own Linv: an inner product of at most n terms.
  a12     A12 = -(M^-1 K) N from the kernel's own Minv, Nbody (and Linv): small kernel M^-1 K is one inner product of n terms
          and the product with N one of 6: gamma_{n+6} |Minv||K||N|; large kernel M^-1 K = X^T (X K), two inner products of
          at most n terms: gamma_{2n+6} |X|^T(|X||K|)|N|.  This is how the unreturned panel M^-1 K is checked.
  a11     A11 - Minv = A12 (M^-1 K)^T from the kernel's own A12, Minv (and Linv): 6 products added to Minv (7 roundings) on
          top of the error of M^-1 K.  The kernel forms the lower triangle and mirrors it (A11 is exactly symmetric), so the
          upper triangle holds (M^-1 K) A12^T: equal to A12 (M^-1 K)^T only as far as A12 = -(M^-1 K) N holds, i.e. to the 6
          roundings of that product on |M^-1 K||N| -- which cancellation can leave far above |A12|.  Hence the scale with
          |M^-1 K||N| in A12's place: gamma_{n+13} (|Minv| + (|Minv||K|)|N|(|Minv||K|)^T), large kernel gamma_{2n+13}
          with |X|^T|X||K| for |Minv||K|.
  nres    R N - I with R = K^T M^-1 K evaluated in EXT from the kernel's Minv (large: Linv): the unreturned R is checked
          through N, its inverse.  The Gauss-Jordan elimination with partial pivoting has no componentwise bound in terms
          of quantities the kernel forms (Higham 14.4 states it in the LU factors), so this quantity has NO derived constant:
          its fraction is in units of u (|K|^T|Minv||K|)|N| and the bound is MARGIN C.
  exact   triu(Lchol, 1) = triu(Linv, 1) = 0; Minv, Nbody, A11 symmetric; A21 = A12^T; A22 = -Nbody: bitwise.
End to end, per body: max|got - EXT| / (u max|EXT|) for Nbody, A11, A12, Minv, Lchol, EXT = this restatement in long double.
The conditioning of the body enters here, so nothing is derived: the bound is MARGIN C per (quantity, family, kernel).

Block product  |y - EXT| <= gamma_{c1+c2+2} (|alpha| (|A11||x1| + |A12||x2|) + |beta y0|) row by row: c1 + c2 products and
  additions in one chain (any partition over lanes has fewer per chain), the product with alpha, beta y0 and the last add.

Configuration  r = 2 ((p0 p0 + d) x + (p0 p1 - s p2) y + (p0 p2 + s p1) z) + loc, d = s s - 1/2.  Per component: a
  coefficient costs at most 3 roundings (s s, the subtraction of 1/2, p p and their sum share the chain: d 2, p p 1, sum 1
  -> the worst term carries 3), its product with the coordinate 1, the two additions of the row 2, the factor 2 none:
  c = 6 for rel, 7 for r (the addition of loc), against T = 2 sum |coefficient terms||coordinate| (+ |loc|), with
  |coefficient terms| = |p p| + |s s| + 1/2 on the diagonal.  Both sides use the same formula, which is a rotation only
  for a unit quaternion: the inputs are asserted to be unit to 8 u (UNIT_QUAT_TOL).

Advance  loc + U dt: 2 roundings on |loc| + |U dt|.  Quaternion: p = omega dt (1 rounding, e_p = 1), nrm = sqrt(p.p): the
  squares 1, the two additions 2, on top of 2 e_p: nrm^2 to 5 u, the root halves it and adds E_SQRT: e_n = 2.5 + E_SQRT.
  qs = cos(nrm / 2): E_TRIG |qs| + (x / 2)|sin(x / 2)| e_n (x = nrm; the argument's error through the derivative).
  f = sin(x / 2) / x: |f| (E_TRIG + 1 + e_n) + |cos(x / 2)| e_n / 2;  q_k = f p_k: |p_k| (that + 2 |f|).
  out = q * r: every component is 4 products in 3 additions, c = 4 on sum |q_a||r_b|, plus sum |dq_a||r_b|.
  E_TRIG = 4 u (2 ulp) and E_SQRT = 2 u (1 ulp) are ASSUMED: no documented accuracy figure for the device's fp64 sin, cos
  and sqrt exists in the toolchain's files.  What carries the check is the fp64 numpy restatement's own worst fraction of this
  expression, C["advance_quat"] = 0.328 (numpy's libm): the asserted bound min(MARGIN C, 1) = 1 is a margin of 3.05 over it,
  inside the MARGIN of every other quantity; both numbers go to the profile file.
  nrm = 0 (omega dt = 0, or p.p underflows: |omega dt| < 1.5e-162) takes f = 1/2, the limit; the result for omega dt = 0
  is the input quaternion bit for bit.

The asserted bound of every fraction is min(MARGIN C, 1) where a derived constant exists and MARGIN C where none does:
MARGIN = _mobility_numpy.MARGIN = 4 covers the kernels' other summation order (four- and eight-lane partial dots,
butterflies, fma).  C is the fp64 restatement's worst fraction against EXT over exactly the cases of the GPU tests, measured
and asserted current by tests/test_rigid_kernels_host.py.  Regenerate with

    python -m pytest tests/test_rigid_kernels_host.py -k table -s        (prints the table)

It comes from the reference side only, never from a kernel."""
import numpy as np

import _mobility_numpy as mn

LONG_DOUBLE = mn.LONG_DOUBLE
EXT = mn.EXT
MARGIN = mn.MARGIN
U = 2.0 ** -53
A_BLOB, ETA = 0.5, 1.3
SMALL_MAX_N = 48                   # kPcMaxN: n above it takes rigid_pc_large_kernel
E_TRIG, E_SQRT = 4.0, 2.0          # assumed, in units of u (see above)
UNIT_QUAT_TOL = 8.0 * U

FAMILIES = ("shell", "bent", "overlap", "loose", "dense", "spd")
RANK_DEFICIENT = ("rod",)
BOUNDARIES = ("wall", "none")
N_B_ALL = tuple(range(1, 43))
E2E = ("Nbody", "A11", "A12", "Minv", "Lchol")

# worst fraction of the fp64 restatement (see the module text): (quantity, kernel) for the factor checks in fractions of
# the derived bound ("nres" in units of u), (quantity, family, kernel) for the end-to-end figures in units of u max|EXT|.
C = {
    ('a11', 'large'):                     0.026,   # measured 0.0259 at (('bent', 22, 'wall', 0),)
    ('a11', 'small'):                    0.0298,   # measured 0.0297 at (('bent', 13, 'wall', 0),)
    ('a12', 'large'):                     0.043,   # measured 0.0430 at (('bent', 22, 'wall', 0),)
    ('a12', 'small'):                     0.189,   # measured 0.1885 at (('bent', 4, 'wall', 0),)
    ('advance_loc',):                     0.723,   # measured 0.7223 at ((256, True),)
    ('advance_quat',):                    0.328,   # measured 0.3278 at ((257, False),)
    ('block',):                           0.282,   # measured 0.2818 at ('c1 = 0',)
    ('chol', 'large'):                    0.192,   # measured 0.1913 at (('bent', 28, 'none', 2),)
    ('chol', 'small'):                    0.421,   # measured 0.4206 at (('bent', 1, 'none', 0),)
    ('config_r',):                        0.444,   # measured 0.4433 at ((42, 7),)
    ('config_rel',):                      0.592,   # measured 0.5914 at ((257, 4),)
    ('e2e_A11', 'bent', 'large'):          31.1,   # measured 31.0675 at (('bent', 40, 'none', 1),)
    ('e2e_A11', 'bent', 'small'):          16.9,   # measured 16.8685 at (('bent', 16, 'wall', 1),)
    ('e2e_A11', 'dense', 'large'):         56.7,   # measured 56.6220 at (('dense', 25, 'wall', 0),)
    ('e2e_A11', 'dense', 'small'):         38.5,   # measured 38.4207 at (('dense', 16, 'none', 0),)
    ('e2e_A11', 'loose', 'large'):         30.6,   # measured 30.5278 at (('loose', 42, 'none', 0),)
    ('e2e_A11', 'loose', 'small'):          699,   # measured 698.1838 at (('loose', 3, 'wall', 1),)
    ('e2e_A11', 'overlap', 'large'):       93.7,   # measured 93.6114 at (('overlap', 38, 'none', 1),)
    ('e2e_A11', 'overlap', 'small'):       27.7,   # measured 27.6169 at (('overlap', 14, 'none', 2),)
    ('e2e_A11', 'shell', 'large'):         18.7,   # measured 18.6856 at (('shell', 42, 'wall', 1),)
    ('e2e_A11', 'shell', 'small'):         12.7,   # measured 12.6777 at (('shell', 15, 'wall', 2),)
    ('e2e_A11', 'spd', 'large'):           17.1,   # measured 17.0641 at (('spd', 38, 'wall', 0),)
    ('e2e_A11', 'spd', 'small'):           8.25,   # measured 8.2441 at (('spd', 14, 'none', 0),)
    ('e2e_A12', 'bent', 'large'):          33.5,   # measured 33.4500 at (('bent', 31, 'none', 2),)
    ('e2e_A12', 'bent', 'small'):            30,   # measured 29.9606 at (('bent', 16, 'none', 2),)
    ('e2e_A12', 'dense', 'large'):         97.2,   # measured 97.1387 at (('dense', 34, 'none', 0),)
    ('e2e_A12', 'dense', 'small'):          110,   # measured 109.7973 at (('dense', 16, 'none', 0),)
    ('e2e_A12', 'loose', 'large'):         38.9,   # measured 38.8936 at (('loose', 39, 'none', 1),)
    ('e2e_A12', 'loose', 'small'):         1010,   # measured 1008.1283 at (('loose', 3, 'wall', 1),)
    ('e2e_A12', 'overlap', 'large'):        404,   # measured 403.6049 at (('overlap', 32, 'wall', 1),)
    ('e2e_A12', 'overlap', 'small'):       45.6,   # measured 45.5991 at (('overlap', 14, 'none', 0),)
    ('e2e_A12', 'shell', 'large'):         21.6,   # measured 21.5461 at (('shell', 36, 'none', 0),)
    ('e2e_A12', 'shell', 'small'):         34.3,   # measured 34.2549 at (('shell', 12, 'none', 2),)
    ('e2e_A12', 'spd', 'large'):           16.3,   # measured 16.2814 at (('spd', 38, 'none', 0),)
    ('e2e_A12', 'spd', 'small'):           13.3,   # measured 13.2236 at (('spd', 8, 'wall', 2),)
    ('e2e_Lchol', 'bent', 'large'):         9.9,   # measured 9.8967 at (('bent', 22, 'wall', 1),)
    ('e2e_Lchol', 'bent', 'small'):        5.98,   # measured 5.9700 at (('bent', 16, 'none', 1),)
    ('e2e_Lchol', 'dense', 'large'):       12.5,   # measured 12.4289 at (('dense', 40, 'none', 1),)
    ('e2e_Lchol', 'dense', 'small'):       6.24,   # measured 6.2330 at (('dense', 16, 'none', 0),)
    ('e2e_Lchol', 'loose', 'large'):       9.28,   # measured 9.2793 at (('loose', 42, 'none', 1),)
    ('e2e_Lchol', 'loose', 'small'):       3.46,   # measured 3.4508 at (('loose', 15, 'none', 0),)
    ('e2e_Lchol', 'overlap', 'large'):     21.6,   # measured 21.5856 at (('overlap', 38, 'none', 1),)
    ('e2e_Lchol', 'overlap', 'small'):     8.19,   # measured 8.1825 at (('overlap', 14, 'wall', 2),)
    ('e2e_Lchol', 'rod', 'large'):         6.97,   # measured 6.9606 at (('rod', 42, 'wall', 2),)
    ('e2e_Lchol', 'rod', 'small'):          2.8,   # measured 2.7993 at (('rod', 16, 'wall', 1),)
    ('e2e_Lchol', 'shell', 'large'):       8.38,   # measured 8.3757 at (('shell', 42, 'wall', 0),)
    ('e2e_Lchol', 'shell', 'small'):       3.51,   # measured 3.5037 at (('shell', 12, 'none', 2),)
    ('e2e_Lchol', 'spd', 'large'):         7.43,   # measured 7.4215 at (('spd', 38, 'wall', 0),)
    ('e2e_Lchol', 'spd', 'small'):         3.77,   # measured 3.7638 at (('spd', 14, 'none', 0),)
    ('e2e_Minv', 'bent', 'large'):         30.4,   # measured 30.3220 at (('bent', 34, 'none', 2),)
    ('e2e_Minv', 'bent', 'small'):         17.7,   # measured 17.6145 at (('bent', 16, 'wall', 1),)
    ('e2e_Minv', 'dense', 'large'):        55.3,   # measured 55.2528 at (('dense', 25, 'wall', 0),)
    ('e2e_Minv', 'dense', 'small'):        39.2,   # measured 39.1025 at (('dense', 16, 'none', 0),)
    ('e2e_Minv', 'loose', 'large'):        30.4,   # measured 30.3981 at (('loose', 42, 'none', 0),)
    ('e2e_Minv', 'loose', 'small'):        12.4,   # measured 12.3688 at (('loose', 12, 'none', 2),)
    ('e2e_Minv', 'overlap', 'large'):        93,   # measured 92.9799 at (('overlap', 38, 'none', 1),)
    ('e2e_Minv', 'overlap', 'small'):      27.5,   # measured 27.4732 at (('overlap', 14, 'none', 2),)
    ('e2e_Minv', 'rod', 'large'):          20.7,   # measured 20.6753 at (('rod', 42, 'wall', 2),)
    ('e2e_Minv', 'rod', 'small'):          8.21,   # measured 8.2047 at (('rod', 16, 'wall', 0),)
    ('e2e_Minv', 'shell', 'large'):        20.3,   # measured 20.2989 at (('shell', 42, 'wall', 1),)
    ('e2e_Minv', 'shell', 'small'):        11.6,   # measured 11.5562 at (('shell', 15, 'wall', 2),)
    ('e2e_Minv', 'spd', 'large'):          17.4,   # measured 17.3044 at (('spd', 38, 'wall', 0),)
    ('e2e_Minv', 'spd', 'small'):          8.54,   # measured 8.5369 at (('spd', 14, 'none', 0),)
    ('e2e_Nbody', 'bent', 'large'):        9.26,   # measured 9.2591 at (('bent', 37, 'wall', 1),)
    ('e2e_Nbody', 'bent', 'small'):        12.7,   # measured 12.6212 at (('bent', 13, 'none', 2),)
    ('e2e_Nbody', 'dense', 'large'):       9.62,   # measured 9.6134 at (('dense', 31, 'wall', 1),)
    ('e2e_Nbody', 'dense', 'small'):       33.8,   # measured 33.7311 at (('dense', 10, 'none', 0),)
    ('e2e_Nbody', 'loose', 'large'):       9.69,   # measured 9.6884 at (('loose', 33, 'wall', 1),)
    ('e2e_Nbody', 'loose', 'small'):       1030,   # measured 1021.4345 at (('loose', 3, 'wall', 1),)
    ('e2e_Nbody', 'overlap', 'large'):      478,   # measured 477.5960 at (('overlap', 32, 'wall', 1),)
    ('e2e_Nbody', 'overlap', 'small'):       36,   # measured 35.9124 at (('overlap', 14, 'none', 1),)
    ('e2e_Nbody', 'shell', 'large'):        9.1,   # measured 9.0907 at (('shell', 27, 'none', 0),)
    ('e2e_Nbody', 'shell', 'small'):       13.5,   # measured 13.4203 at (('shell', 9, 'none', 2),)
    ('e2e_Nbody', 'spd', 'large'):         8.81,   # measured 8.8087 at (('spd', 41, 'none', 1),)
    ('e2e_Nbody', 'spd', 'small'):         4.19,   # measured 4.1819 at (('spd', 11, 'none', 1),)
    ('linv', 'large'):                   0.0717,   # measured 0.0716 at (('loose', 21, 'none', 2),)
    ('linv', 'small'):                     0.25,   # measured 0.2495 at (('bent', 1, 'wall', 2),)
    ('minv', 'large'):                    0.206,   # measured 0.2053 at (('bent', 34, 'none', 2),)
    ('minv', 'small'):                    0.391,   # measured 0.3906 at (('spd', 2, 'wall', 1),)
    ('nres', 'large'):                     2.99,   # measured 2.9835 at (('bent', 34, 'wall', 0),)
    ('nres', 'small'):                     1.57,   # measured 1.5635 at (('spd', 5, 'none', 2),)
}
# where MARGIN C exceeds 1 the derived bound itself is the asserted bound (tests/test_rigid_kernels_host.py lists them)
DERIVED_BOUND_APPLIES = (('advance_loc',), ('advance_quat',), ('block',), ('chol', 'small'), ('config_r',), ('config_rel',), ('minv', 'small'))


# worst fraction per key seen by the GPU tests of this process (tools/rigid_kernels_report.py prints them)
RESULTS = {}


def record(key, fraction):
  RESULTS[key] = max(RESULTS.get(key, 0.0), float(fraction))
  return fraction


def gamma(k):
  k = EXT(k)
  return k * EXT(U) / (EXT(1) - k * EXT(U))


def cw_ratio(residual, scale):
  """worst |residual| / |scale| over the elements in units of 2^-53; where the scale is exactly 0 the residual must be
  exactly 0 (inf otherwise, as for a residual that is not finite)."""
  r = np.abs(np.asarray(residual, dtype=EXT)).reshape(-1)
  s = np.abs(np.broadcast_to(np.asarray(scale, dtype=EXT), np.shape(residual))).reshape(-1)
  if r.size == 0:
    return 0.0
  if not np.all(np.isfinite(r)) or not np.all(np.isfinite(s)):
    return float("inf")
  zero = s == 0
  if np.any(r[zero] != 0):
    return float("inf")
  if np.all(zero):
    return 0.0
  return float((r[~zero] / s[~zero]).max() / EXT(U))


def bound(key):
  """the asserted bound of the fraction `key`"""
  derived = not (key[0] in ("nres",) or key[0].startswith("e2e_"))
  return min(MARGIN * C[key], 1.0) if derived else MARGIN * C[key]


# ---------------------------------------------------------------------------------------------------------------------
# bodies
# ---------------------------------------------------------------------------------------------------------------------
def rotation(q, dtype=EXT):
  """the kernel's matrix of the quaternion (s, p0, p1, p2)"""
  s, p0, p1, p2 = [dtype(v) for v in q]
  d = s * s - dtype(0.5)
  two = dtype(2)
  return two * np.array([[p0 * p0 + d, p0 * p1 - s * p2, p0 * p2 + s * p1], [p1 * p0 + s * p2, p1 * p1 + d, p1 * p2 - s * p0],
                         [p2 * p0 - s * p1, p2 * p1 + s * p0, p2 * p2 + d]], dtype=dtype)


def unit_quaternions(rng, m):
  """(m, 4) float64, normalised in EXT and rounded once per component: unit to ~u"""
  q = rng.randn(m, 4).astype(EXT)
  q /= np.sqrt((q * q).sum(axis=1, keepdims=True))
  return q.astype(np.float64)


def quat_norm_defect(q):
  q = np.asarray(q, dtype=np.float64).astype(EXT)
  return float(np.abs((q * q).sum(axis=-1) - 1).max())


def reference_blobs(family, n_b, seed=0):
  """(n_b, 3) float64 body-frame positions for blob radius A_BLOB"""
  a = A_BLOB
  if family == "shell":          # nested icosahedron shells, nearest neighbours in contact, cut at n_b blobs
    from rigidmultiblobswall_amd.structures import icosahedron_shell
    r0 = 2.0 * a / 1.0514622242382672
    return np.concatenate([icosahedron_shell(k * r0) for k in range(1, 5)])[:n_b].copy()
  l = np.arange(n_b, dtype=np.float64)
  if family == "rod":            # exactly collinear, along axis `seed`
    p = np.zeros((n_b, 3))
    p[:, seed % 3] = 2.0 * a * (l - 0.5 * (n_b - 1))
    return p
  if family == "bent":           # two arms at 60 degrees, blobs in contact
    h = (n_b + 1) // 2
    p = np.zeros((n_b, 3))
    p[:h, 0] = 2.0 * a * l[:h]
    p[h:, 0] = p[h - 1, 0] + 2.0 * a * 0.5 * (l[h:] - h + 1)
    p[h:, 1] = 2.0 * a * np.sqrt(0.75) * (l[h:] - h + 1)
    return p - p.mean(axis=0)
  if family == "overlap":        # a helix of blobs one radius apart along its axis: every blob overlaps its neighbours
    p = np.stack([a * l, 0.6 * a * np.sin(0.7 * l), 0.6 * a * np.cos(0.7 * l)], axis=1)
    return p - p.mean(axis=0)
  if family in ("loose", "dense"):
    fill, dmin = (0.2, 1.0 * a) if family == "loose" else (1.0, 0.3 * a)
    rb = a * (n_b / fill) ** (1.0 / 3.0)
    rng = np.random.RandomState(7919 * n_b + 13 * seed + (0 if family == "loose" else 5))
    pts = []
    while len(pts) < n_b:
      c = (2.0 * rng.rand(3) - 1.0) * rb
      if c @ c <= rb * rb and all(np.linalg.norm(c - q) >= dmin for q in pts):
        pts.append(c)
    return np.array(pts)
  raise ValueError(family)


def build_K(rel):
  """(n_b, 3) -> (3 n_b, 6): rows [I, -(rel x)]"""
  rel = np.asarray(rel, dtype=np.float64)
  K = np.zeros((len(rel), 3, 6))
  K[:, 0, 0] = K[:, 1, 1] = K[:, 2, 2] = 1.0
  K[:, 0, 4] = rel[:, 2];  K[:, 0, 5] = -rel[:, 1]
  K[:, 1, 3] = -rel[:, 2]; K[:, 1, 5] = rel[:, 0]
  K[:, 2, 3] = rel[:, 1];  K[:, 2, 4] = -rel[:, 0]
  return K.reshape(-1, 6)


_bodies = {}


def body(family, n_b, boundary, variant):
  """(M (n, n) float64, K (n, 6) float64): the real blob mobility of one body (the EXT blocks rounded to fp64, so that the
  kernel and the reference read the same bits), or the random SPD matrix G G^T / n + I / 2 of the older test ("spd")."""
  key = (family, n_b, boundary, variant)
  if key in _bodies:
    return _bodies[key]
  n = 3 * n_b
  if family == "spd":
    rng = np.random.RandomState(100 * n_b + 10 * variant + BOUNDARIES.index(boundary))
    G = rng.randn(n, n)
    M = G @ G.T / n + 0.5 * np.eye(n)
    rel = rng.randn(n_b, 3)
  else:
    ref = reference_blobs(family, n_b, variant)
    if family == "rod" or variant == 0:
      rel = ref
    else:
      q = unit_quaternions(np.random.RandomState(31 * n_b + variant), 1)[0]
      rel = (ref.astype(EXT) @ rotation(q).T).astype(np.float64)
    centre = np.array([0.3 * variant, -0.2 * variant, 0.0])
    if boundary == "wall":
      centre[2] = (1.5 + 0.7 * variant) * A_BLOB - rel[:, 2].min()
    r = rel + centre
    rel = r - centre
    M = mn.dense(mn.blocks("tt", boundary, r, A_BLOB, ETA, dtype=EXT)).astype(np.float64)
  _bodies[key] = (M, build_K(rel))
  return _bodies[key]


def families_of(n_b):
  """the two families the GPU test runs at n_b"""
  return FAMILIES[n_b % 6], FAMILIES[(n_b + 3) % 6]


def launch(family, n_b, boundary, bodies=3):
  """(M (bodies, n, n), K (bodies, n, 6)) of one launch"""
  got = [body(family, n_b, boundary, v) for v in range(bodies)]
  return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def skewed(M, seed=0, size=1e-3):
  """M + S - S^T with |S_ij| ~ size |M_ij|: sym(result) differs from sym(M) by roundings only, so the result is compared
  with the symmetrised INPUT as given"""
  rng = np.random.RandomState(seed)
  S = size * rng.randn(*M.shape) * np.abs(M)
  return M + S - np.swapaxes(S, -1, -2)


# ---------------------------------------------------------------------------------------------------------------------
# the factor kernels
# ---------------------------------------------------------------------------------------------------------------------
def _root_exact(piv):
  return np.sqrt(piv)


def root_fp32_seed(piv):
  """mutant (b): the pivot root from an fp32 reciprocal-root seed with one Newton step"""
  T = type(piv)
  y = T(np.float32(1.0) / np.sqrt(np.float32(piv)))
  y = y * (T(1.5) - T(0.5) * piv * y * y)
  return piv * y


def invert_resistance(R, dtype):
  """Gauss-Jordan with partial pivoting on [R | I], symmetrised; -> (N, ok) as the kernel's invert_resistance"""
  T = np.dtype(dtype).type
  ok = True
  w = np.zeros((6, 12), dtype=dtype)
  w[:, :6] = R
  w[:, 6:] = np.eye(6, dtype=dtype)
  for c in range(6):
    piv, best = c, abs(w[c, c])
    for i in range(c + 1, 6):
      if abs(w[i, c]) > best:
        best, piv = abs(w[i, c]), i
    if piv != c:
      w[[c, piv]] = w[[piv, c]]
    d = w[c, c]
    if not abs(d) > 0:
      ok = False
      continue
    w[c] = w[c] * (T(1) / d)
    for i in range(6):
      if i != c:
        f = w[i, c]
        w[i] = w[i] - f * w[c]
  worst = T(0)
  W = w[:, 6:]
  for i in range(6):
    s = np.zeros(6, dtype=dtype)
    for k in range(6):
      s = s + R[i, k] * W[k]
    s[i] = s[i] - T(1)
    for e in np.abs(s):
      if not e <= worst:
        worst = e
  if not worst < 1e-8:
    ok = False
  return T(0.5) * (W + W.T), ok


def preconditioner(M, K, dtype=np.float64, large=None, symmetrise=True, root=_root_exact, N_other=None):
  """One body, the kernel's own algorithm (large: rigid_pc_large_kernel; default by n).  -> dict of Lchol, Linv, Minv, Nbody,
  A11, A12, A21, A22 in `dtype` and info.  symmetrise=False reads the lower triangle only (mutant a); root: the pivot root
  (mutant b); N_other: a 6 x 6 matrix that takes N's place in A12 and A11 (mutant e)."""
  T = np.dtype(dtype).type
  M = np.asarray(M, dtype=np.float64).astype(dtype)
  Kl = np.asarray(K, dtype=np.float64).astype(dtype)
  n = M.shape[0]
  large = n > SMALL_MAX_N if large is None else large
  bad = False
  with np.errstate(all="ignore"):
    A = T(0.5) * (M + M.T) if symmetrise else np.tril(M) + np.tril(M, -1).T
    # right-looking Cholesky, lower: the column divided by the pivot's root, then the trailing triangle
    for k in range(n):
      piv = A[k, k]
      if not piv > 0:
        bad = True
      rt = root(piv)
      A[k + 1:, k] = A[k + 1:, k] / rt
      A[k, k] = rt
      c = A[k + 1:, k]
      A[k + 1:, k + 1:] -= np.tril(c[:, None] * c[None, :])
    L = np.tril(A)
    X = np.zeros((n, n), dtype=dtype)
    if not large:
      # row by row: (L^-1)[i][c] = (delta_ic - sum_{k=c}^{i-1} L[i][k] (L^-1)[k][c]) / L[i][i]
      for i in range(n):
        s = np.zeros(i + 1, dtype=dtype)
        for k in range(i):
          s[:k + 1] += L[i, k] * X[k, :k + 1]
        e = np.zeros(i + 1, dtype=dtype)
        e[i] = T(1)
        X[i, :i + 1] = (e - s) / L[i, i]
    else:
      # in place from the last column: X[j+1:, j] = -X[j][j] (X[j+1:, j+1:] L[j+1:, j])
      X = L.copy()
      for j in range(n - 1, -1, -1):
        dj = T(1) / X[j, j]
        col = X[:, j].copy()
        X[j, j] = dj
        s = np.zeros(n - j - 1, dtype=dtype)
        for k in range(j + 1, n):
          s[k - j - 1:] += X[k:, k] * col[k]
        X[j + 1:, j] = -dj * s
    # M^-1[i][j] = sum_{k >= max(i, j)} X[k][i] X[k][j]: ascending k; the terms below max(i, j) are exact zeros
    Minv = np.zeros((n, n), dtype=dtype)
    for k in range(n):
      Minv[:k + 1, :k + 1] += X[k, :k + 1, None] * X[k, None, :k + 1]
    MK = np.zeros((n, 6), dtype=dtype)
    R = np.zeros((6, 6), dtype=dtype)
    if not large:
      for j in range(n):
        MK += Minv[:, j, None] * Kl[j, None, :]
      for i in range(n):
        R += Kl[i, :, None] * MK[i, None, :]
    else:
      Y = np.zeros((n, 6), dtype=dtype)
      for k in range(n):
        Y[k:] += X[k:, k, None] * Kl[k, None, :]
      for k in range(n):
        MK[:k + 1] += X[k, :k + 1, None] * Y[k, None, :]
      for i in range(n):
        R += Y[i, :, None] * Y[i, None, :]
    N, ok = invert_resistance(R, dtype)
    bad = bad or not ok
    Nu = N if N_other is None else np.asarray(N_other).astype(dtype)
    s = np.zeros((n, 6), dtype=dtype)
    for k in range(6):
      s += MK[:, k, None] * Nu[k, None, :]
    A12 = -s
    # A11 = M^-1 + A12 (M^-1 K)^T: the lower triangle, mirrored (exactly symmetric)
    A11 = Minv.copy()
    for c in range(6):
      A11 += A12[:, c, None] * MK[None, :, c]
    A11 = np.tril(A11) + np.tril(A11, -1).T
  return dict(Lchol=L, Linv=np.tril(X), Minv=Minv, Nbody=N, A11=A11, A12=A12, A21=A12.T.copy(), A22=-N, info=int(bad))


def preconditioner_batch(Ms, Ks, dtype=np.float64, large=None, **kw):
  outs = [preconditioner(M, K, dtype, large, **kw) for M, K in zip(Ms, Ks)]
  o = {k: np.stack([np.asarray(q[k]) for q in outs]) for k in outs[0] if k != "info"}
  o["info"] = int(any(q["info"] for q in outs))
  return o


_ext = {}


def ext_reference(family, n_b, boundary, variant, large=None, skew_seed=None):
  """the EXT restatement of one body of the GPU test, cached per process"""
  key = (family, n_b, boundary, variant, large, skew_seed)
  if key not in _ext:
    M, K = body(family, n_b, boundary, variant)
    if skew_seed is not None:
      M = skewed(M, skew_seed)
    _ext[key] = preconditioner(M, K, EXT, large)
  return _ext[key]


def exact_structure(o):
  """names of the bitwise properties one body's (or a batch's) outputs violate"""
  t = lambda x: np.swapaxes(np.asarray(x), -1, -2)
  bad = []
  for name in ("Lchol", "Linv"):
    if np.any(np.triu(np.asarray(o[name]), 1) != 0):
      bad.append("triu(%s)" % name)
  for name in ("Minv", "Nbody", "A11"):
    if not np.array_equal(np.asarray(o[name]), t(o[name])):
      bad.append("sym(%s)" % name)
  if not np.array_equal(np.asarray(o["A21"]), t(o["A12"])):
    bad.append("A21 = A12^T")
  if not np.array_equal(np.asarray(o["A22"]), -np.asarray(o["Nbody"])):
    bad.append("A22 = -Nbody")
  return bad


def factor_fractions(o, M, K, large=None, full=True):
  """{quantity: fraction} of one body's fp64 outputs `o` (see the module text); full=False: chol, linv, minv only (a body
  whose resistance has no inverse)."""
  M = np.asarray(M, dtype=np.float64).astype(EXT)
  Ke = np.asarray(K, dtype=np.float64).astype(EXT)
  n = M.shape[0]
  large = n > SMALL_MAX_N if large is None else large
  g = lambda k: float(gamma(k) / EXT(U))
  e = lambda name: np.asarray(o[name], dtype=np.float64).astype(EXT)
  L, X, Minv = e("Lchol"), e("Linv"), e("Minv")
  aL, aX = np.abs(L), np.abs(X)
  eye = np.eye(n, dtype=EXT)
  f = {"chol": cw_ratio(L @ L.T - (M + M.T) / 2, aL @ aL.T) / g(n + 1)}
  if large:
    f["linv"] = cw_ratio(X @ L - eye, aX @ aL) / g(n)
  else:
    f["linv"] = cw_ratio(L @ X - eye, aL @ aX) / g(n)
  f["minv"] = cw_ratio(Minv - X.T @ X, aX.T @ aX) / g(n)
  if not full:
    return f
  N, A11, A12 = e("Nbody"), e("A11"), e("A12")
  aK, aN = np.abs(Ke), np.abs(N)
  if large:
    MK, aMK, m = X.T @ (X @ Ke), aX.T @ (aX @ aK), 2 * n
  else:
    MK, aMK, m = Minv @ Ke, np.abs(Minv) @ aK, n
  f["a12"] = cw_ratio(A12 + MK @ N, aMK @ aN) / g(m + 6)
  f["a11"] = cw_ratio(A11 - Minv - A12 @ MK.T, np.abs(Minv) + (aMK @ aN) @ aMK.T) / g(m + 13)
  f["nres"] = cw_ratio((Ke.T @ MK) @ N - np.eye(6, dtype=EXT), (aK.T @ aMK) @ aN)
  return f


def e2e_fractions(o, ref, names=E2E):
  """{e2e_<name>: max|got - EXT| / (u max|EXT|)} of one body"""
  out = {}
  for name in names:
    r = np.asarray(ref[name], dtype=EXT)
    out["e2e_" + name] = cw_ratio(np.abs(np.asarray(o[name], dtype=np.float64).astype(EXT) - r).max(), np.abs(r).max())
  return out


# ---------------------------------------------------------------------------------------------------------------------
# configuration
# ---------------------------------------------------------------------------------------------------------------------
def configuration(ref, loc, quat, dtype=np.float64):
  """-> r (nb n_b, 3), rel (nb, n_b, 3), T_rel (nb, n_b, 3): the sum of |terms| of the bound (K is build_K(rel))"""
  T = np.dtype(dtype).type
  ref = np.asarray(ref, dtype=np.float64).astype(dtype)
  loc = np.asarray(loc, dtype=np.float64).astype(dtype)
  q = np.asarray(quat, dtype=np.float64).astype(dtype)
  s, p0, p1, p2 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
  d = s * s - T(0.5)
  ad = s * s + T(0.5)
  ab = np.abs
  coef = ((p0 * p0 + d, p0 * p1 - s * p2, p0 * p2 + s * p1), (p1 * p0 + s * p2, p1 * p1 + d, p1 * p2 - s * p0),
          (p2 * p0 - s * p1, p2 * p1 + s * p0, p2 * p2 + d))
  size = ((ab(p0 * p0) + ad, ab(p0 * p1) + ab(s * p2), ab(p0 * p2) + ab(s * p1)), (ab(p1 * p0) + ab(s * p2), ab(p1 * p1) + ad, ab(p1 * p2) + ab(s * p0)),
          (ab(p2 * p0) + ab(s * p1), ab(p2 * p1) + ab(s * p0), ab(p2 * p2) + ad))
  x, y, z = ref[:, :, 0], ref[:, :, 1], ref[:, :, 2]
  rel = np.zeros_like(ref)
  terms = np.zeros_like(ref)
  for c in range(3):
    cx, cy, cz = [v[:, None] for v in coef[c]]
    sx, sy, sz = [v[:, None] for v in size[c]]
    rel[:, :, c] = T(2) * (cx * x + cy * y + cz * z)
    terms[:, :, c] = T(2) * (sx * ab(x) + sy * ab(y) + sz * ab(z))
  r = rel + loc[:, None, :]
  return r.reshape(-1, 3), rel, terms


def config_fractions(r, rel, ref, loc, quat):
  """fractions of the derived bounds (6 u T for rel, 7 u (T + |loc|) for r) of a kernel's fp64 outputs"""
  r_e, rel_e, terms = configuration(ref, loc, quat, EXT)
  loc_e = np.abs(np.asarray(loc, dtype=np.float64).astype(EXT))[:, None, :]
  f = {"config_rel": cw_ratio(np.asarray(rel, dtype=np.float64).astype(EXT) - rel_e, terms) / 6.0}
  tr = (terms + loc_e).reshape(-1, 3)
  f["config_r"] = cw_ratio(np.asarray(r, dtype=np.float64).astype(EXT).reshape(-1, 3) - r_e, tr) / 7.0
  return f


# ---------------------------------------------------------------------------------------------------------------------
# advance
# ---------------------------------------------------------------------------------------------------------------------
def advance(loc, quat, Uv, dt, dtype=np.float64, half_below=0.0):
  """x + v dt and quaternion(omega dt) * q.  dt: scalar or (nb,).  half_below: mutant (c), sin(x/2)/x -> 1/2 below it.
  -> loc_out (nb, 3), quat_out (nb, 4), bound (nb, 4): the derived bound of the quaternion in units of u (EXT run only
  meaningful), bound_loc (nb, 3)"""
  T = np.dtype(dtype).type
  loc = np.asarray(loc, dtype=np.float64).astype(dtype)
  q = np.asarray(quat, dtype=np.float64).astype(dtype)
  Uv = np.asarray(Uv, dtype=np.float64).astype(dtype)
  dt = np.broadcast_to(np.asarray(dt, dtype=np.float64).reshape(-1), (len(loc),)).astype(dtype)[:, None]
  with np.errstate(all="ignore"):
    loc_out = loc + Uv[:, :3] * dt
    b_loc = T(2) * (np.abs(loc) + np.abs(Uv[:, :3] * dt))
    p = Uv[:, 3:] * dt
    nrm = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])
    safe = np.where(nrm > 0, nrm, T(1))
    qs = np.cos(T(0.5) * nrm)
    f = np.where(nrm > 0, np.sin(T(0.5) * nrm) / safe, T(0.5))
    if half_below:
      f = np.where(nrm < half_below, T(0.5), f)
    qv = f[:, None] * p
    rs, rv = q[:, 0], q[:, 1:]
    out = np.empty_like(q)
    out[:, 0] = qs * rs - (qv[:, 0] * rv[:, 0] + qv[:, 1] * rv[:, 1] + qv[:, 2] * rv[:, 2])
    out[:, 1] = qs * rv[:, 0] + rs * qv[:, 0] + (qv[:, 1] * rv[:, 2] - qv[:, 2] * rv[:, 1])
    out[:, 2] = qs * rv[:, 1] + rs * qv[:, 1] + (qv[:, 2] * rv[:, 0] - qv[:, 0] * rv[:, 2])
    out[:, 3] = qs * rv[:, 2] + rs * qv[:, 2] + (qv[:, 0] * rv[:, 1] - qv[:, 1] * rv[:, 0])
    # the derived bound
    e_n = T(2.5 + E_SQRT)
    half = T(0.5) * nrm
    dqs = T(E_TRIG) * np.abs(qs) + half * np.abs(np.sin(half)) * e_n
    dqv = np.abs(p) * (np.abs(f) * (T(E_TRIG) + T(3) + e_n) + np.abs(np.cos(half)) * e_n * T(0.5))[:, None]
    aq = np.concatenate([np.abs(qs)[:, None], np.abs(qv)], axis=1)
    dq = np.concatenate([dqs[:, None], dqv], axis=1)
    ar = np.abs(q)
    pair = ((0, 0), (1, 1), (2, 2), (3, 3)), ((0, 1), (1, 0), (2, 3), (3, 2)), ((0, 2), (2, 0), (3, 1), (1, 3)), ((0, 3), (3, 0), (1, 2), (2, 1))
    bnd = np.zeros_like(q)
    for c in range(4):
      for a_, b_ in pair[c]:
        bnd[:, c] += T(4) * aq[:, a_] * ar[:, b_] + dq[:, a_] * ar[:, b_]
  return loc_out, out, bnd, b_loc


def advance_fractions(loc_got, quat_got, loc, quat, Uv, dt):
  l_e, q_e, bnd, b_loc = advance(loc, quat, Uv, dt, EXT)
  x = lambda v: np.asarray(v, dtype=np.float64).astype(EXT)
  return {"advance_quat": cw_ratio(x(quat_got) - q_e, bnd), "advance_loc": cw_ratio(x(loc_got) - l_e, b_loc)}


ANGLES = (0.0, 1e-200, 1e-160, 1e-20, 1e-8, 1e-6, 3e-5, 1e-4, 1e-2, 1.0, np.pi, 2.0 * np.pi, 1e3)


def advance_case(nb, per_body_dt, seed=0):
  """loc, quat, U, dt of one launch: body b takes rung (b // 2) % len(ANGLES) of the ladder of |omega dt|; even b has the
  quaternion (1, 0, 0, 0) exactly, odd b a random unit one.  (1e-6 and 3e-5 are added to the ladder of the issue: below
  1e-4 and far enough above sqrt(u) for the x^2 / 24 of sin(x/2)/x to be visible.)"""
  rng = np.random.RandomState(4000 + 2 * nb + int(per_body_dt) + seed)
  loc = rng.randn(nb, 3) * 3.0
  quat = unit_quaternions(rng, nb)
  quat[0::2] = (1.0, 0.0, 0.0, 0.0)
  dt = rng.rand(nb) + 0.5 if per_body_dt else np.full(nb, 0.37)
  Uv = rng.randn(nb, 6)
  ang = np.array([ANGLES[(b // 2) % len(ANGLES)] for b in range(nb)])
  w = Uv[:, 3:].astype(EXT)
  w = w / np.sqrt((w * w).sum(axis=1, keepdims=True)) * (ang.astype(EXT) / dt.astype(EXT))[:, None]
  Uv[:, 3:] = w.astype(np.float64)
  return loc, quat, Uv, (dt if per_body_dt else 0.37), ang


# ---------------------------------------------------------------------------------------------------------------------
# block product
# ---------------------------------------------------------------------------------------------------------------------
def block_apply(A1, A2, x1, x2, y0, alpha, beta, dtype=np.float64, drop=None):
  """y = beta y0 + alpha (A1 x1 + A2 x2) for a batch: A1 (nb, r, c1) or None, A2 (nb, r, c2) or None, one chain per row in
  ascending column order (row_dot).  beta = 0 does not read y0.  drop = (b, row): mutant (d), that row's last entry is left
  out.  -> y (nb, r), scale (nb, r) = |alpha| (|A1||x1| + |A2||x2|) + |beta y0|"""
  T = np.dtype(dtype).type
  nb, r = np.shape(y0)
  s = np.zeros((nb, r), dtype=dtype)
  sc = np.zeros((nb, r), dtype=dtype)
  blocks = [(A, x) for A, x in ((A1, x1), (A2, x2)) if A is not None and np.shape(A)[2] > 0]
  with np.errstate(all="ignore"):
    for bi, (A, x) in enumerate(blocks):
      A = np.asarray(A, dtype=np.float64).astype(dtype)
      x = np.asarray(x, dtype=np.float64).astype(dtype)
      for k in range(A.shape[2]):
        t = A[:, :, k] * x[:, k, None]
        if drop is not None and bi == len(blocks) - 1 and k == A.shape[2] - 1:
          t[drop[0], drop[1]] = T(0)
        s += t
        sc += np.abs(A[:, :, k] * x[:, k, None])
    if beta == 0.0:
      y = T(alpha) * s
      sc = abs(T(alpha)) * sc
    else:
      y0 = np.asarray(y0, dtype=np.float64).astype(dtype)
      y = T(beta) * y0 + T(alpha) * s
      sc = abs(T(alpha)) * sc + np.abs(T(beta) * y0)
  return y, sc


def block_fraction(y_got, A1, A2, x1, x2, y0, alpha, beta):
  """worst row's fraction of gamma_{c1+c2+2} scale"""
  y_e, sc = block_apply(A1, A2, x1, x2, y0, alpha, beta, EXT)
  m = sum(np.shape(A)[2] for A in (A1, A2) if A is not None) + 2
  return cw_ratio(np.asarray(y_got, dtype=np.float64).astype(EXT) - y_e, sc) / float(gamma(m) / EXT(U))


def row_scales(rng, nb, rows):
  """powers of ten from 1e-8 to 1e8, one per row, every power present when rows >= 17"""
  e = np.arange(rows) % 17 - 8
  return 10.0 ** np.stack([rng.permutation(e) for _ in range(nb)]).astype(np.float64)


BLOCK_COLS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 96, 97, 127, 128, 129, 257)
BLOCK_ROWS = (1, 2, 3, 4, 5, 6, 8, 9, 63, 64, 65, 126, 129)
PC_SHAPES_NB = (1, 12, 16, 17, 32, 33, 42)
ALPHA_BETA = ((1.0, 0.0), (1.0, 1.0), (-1.0, 1.0), (0.5, -1.0), (0.0, 0.5), (-1.0, 0.0), (0.5, 0.5), (0.0, 0.0))


def block_case(nb, r1, c1, r2, c2, seed):
  """random blocks whose rows are scaled by powers of ten; -> dict of float64 arrays"""
  rng = np.random.RandomState(seed)
  s1, s2 = row_scales(rng, nb, r1), row_scales(rng, nb, r2)
  d = dict(A11=rng.randn(nb, r1, c1) * s1[:, :, None], A12=rng.randn(nb, r1, c2) * s1[:, :, None],
           A21=rng.randn(nb, r2, c1) * s2[:, :, None], A22=rng.randn(nb, r2, c2) * s2[:, :, None],
           x1=rng.randn(nb, c1), x2=rng.randn(nb, c2), y1=rng.randn(nb, r1) * s1, y2=rng.randn(nb, r2) * s2)
  return d


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU tests (the host test measures C over exactly these)
# ---------------------------------------------------------------------------------------------------------------------
ROD_N_B = (3, 16, 17, 42)
SKEW_CASES = (("dense", 16, "wall"), ("dense", 22, "wall"))        # one per kernel; n = 66 is the first size past a 64-lane row
INDEPENDENCE_N_B = (16, 17)
CONFIG_SHAPES = ((1, 5), (2, 5), (7, 5), (16, 5), (42, 7), (257, 4))          # (n_b, bodies): 42 x 7 = 294 crosses one 256-thread block
ADVANCE_BODIES = (1, 255, 256, 257)


def kernel_of(n_b):
  return "large" if 3 * n_b > SMALL_MAX_N else "small"


def expected_info(family, n_b):
  """1 for a body whose resistance K^T M^-1 K has no inverse: one or two blobs, or blobs on one line"""
  return int(n_b <= 2 or family in RANK_DEFICIENT)


def pc_launches():
  """(family, n_b, boundary) of every three-body launch of the preconditioner test"""
  out = [(f, n_b, bnd) for n_b in N_B_ALL for f in families_of(n_b) for bnd in BOUNDARIES]
  out += [("rod", n_b, bnd) for n_b in ROD_N_B for bnd in BOUNDARIES]
  return out


def independence_launch(n_b):
  """[A, B, bad, C, D]: (M (5, n, n), K (5, n, 6)).  n_b = 16: `bad` is not positive definite (its matrix negated);
  n_b = 17: its K has rank 3 (every blob at the tracking point)."""
  fam = ("shell", "dense", "loose", "overlap", "bent")
  got = [body(f, n_b, "wall", 1) for f in fam]
  M, K = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
  if n_b == 16:
    M[2] = -M[2]
  else:
    K[2, :, 3:] = 0.0
  return M, K


def config_case(n_b, nb):
  """ref (nb, n_b, 3) with components from 1e-6 to 1e3 within every body, loc (nb, 3), quat (nb, 4): body 0 (1, 0, 0, 0),
  body 1 (0, 1, 0, 0), body 2 next to the identity (s = 1 - 2^-40), the others random"""
  rng = np.random.RandomState(600 + 7 * n_b + nb)
  ref = rng.randn(nb, n_b, 3) * 10.0 ** rng.uniform(-6.0, 3.0, size=(nb, n_b, 3))
  ref[:, 0, 0], ref[:, -1, 2] = 1e-6, 1e3
  loc = rng.randn(nb, 3) * 3.0
  quat = unit_quaternions(rng, nb)
  quat[0] = (1.0, 0.0, 0.0, 0.0)
  if nb > 1:
    quat[1] = (0.0, 1.0, 0.0, 0.0)
  if nb > 2:
    s = EXT(1) - EXT(2.0) ** -40
    ax = np.array([0.6, 0.0, 0.8], dtype=EXT)
    quat[2] = np.concatenate([[s], np.sqrt(EXT(1) - s * s) * ax]).astype(np.float64)
  assert quat_norm_defect(quat) <= UNIT_QUAT_TOL
  return ref, loc, quat


def block_cases():
  """(nb, r1, c1, r2, c2, alpha, beta, seed) of the shape sweep: every column count with every row count, the lower blocks
  6 x 6 as in the preconditioner; alpha, beta and the batch cycle"""
  out = []
  for i, c1 in enumerate(BLOCK_COLS):
    for j, r1 in enumerate(BLOCK_ROWS):
      k = i * len(BLOCK_ROWS) + j
      al, be = ALPHA_BETA[k % len(ALPHA_BETA)]
      out.append((1 if k % 2 else 3, r1, c1, 6, 6, al, be, 9000 + k))
  for k, n_b in enumerate(PC_SHAPES_NB):
    al, be = ALPHA_BETA[k % len(ALPHA_BETA)]
    out.append((3 if k % 2 else 1, 3 * n_b, 3 * n_b, 6, 6, al, be, 9500 + k))
  return out


def block_extra_cases():
  """(label, how, case dict, alpha, beta, blocks as the product sees them) beyond the shape sweep.  how: "plain"; "transposed"
  (A21 is handed over as its transpose's storage); "strided" (every block a slice of a larger tensor); "operator" (top = y - K U,
  bottom = -K^T lambda with one K, handed over once as A12 and once transposed as A21)"""
  out = []
  for r2 in (6, 12):            # long strided rows: walked wave = row up to 8 rows, thread = row above
    d = block_case(3, 126, 126, r2, 6, 9700 + r2)
    out.append((("transposed", r2), "transposed", d, 1.0, 0.0, [d["A11"], d["A12"], d["A21"], d["A22"]]))
  d = block_case(3, 126, 126, 6, 6, 9706)
  out.append(("operator", "operator", d, -1.0, 1.0, [None, d["A12"], np.ascontiguousarray(d["A12"].transpose(0, 2, 1)), None]))
  d = block_case(3, 65, 97, 9, 17, 9800)
  full = [d["A11"], d["A12"], d["A21"], d["A22"]]
  out.append(("strided", "strided", d, 0.5, -1.0, full))
  for k in range(4):
    out.append((("absent", k), "plain", d, -1.0, 0.0 if k % 2 else 1.0, [None if q == k else A for q, A in enumerate(full)]))
  e = block_case(3, 5, 0, 3, 2, 9802)
  out.append(("c1 = 0", "plain", e, 1.0, 0.5, [e["A11"], e["A12"], e["A21"], e["A22"]]))
  out.append(("c1 = 0, half absent", "plain", e, 0.5, 0.0, [None, e["A12"], None, e["A22"]]))
  return out
