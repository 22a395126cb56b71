"""numpy restatement of the pair blocks of the blob mobility, written from oracle/oracle_mobility.c and the mirror-image
formulas of the README -- TEST infrastructure.

  blocks(kind, boundary, r, a, eta, L, dtype)  (N, N, 3, 3): block [i, j] maps the vector of blob j to the result at blob i
  scale(kind, boundary, r, a, eta, L)          (N, N): the size every rounding bound of a block is stated against

kind: tt, tr, rt, rr.  boundary:
  "none"  unbounded RPY tensors (overlap patches for r < 2a, self 4/(3a), 0, 0, 1/a^3 in units of 1/(8 pi eta))
  "wall"  no-slip wall at z = 0 (Swan & Brady) WITH what the product wrappers do around the kernel: z <= a is clamped to a
          and a blob with z < a is damped by b = z/a on both sides (block_ij *= b_i b_j)
  "free"  stress-free surface at z = 0, raw heights: M_tt = B_tt(d) + B_tt(R) S, M_tr = B_tr(d) - B_tr(R) S,
          M_rt = B_rt(d) + B_rt(R) S, M_rr = B_rr(d) - B_rr(R) S, S = diag(1, 1, -1), R = (d_x, d_y, z_i + z_j), the image
          of a blob's own block by the PAIR formula at R = (0, 0, 2 z_i)
L: pseudo-periodic lengths, the oracle's rule: nearest image d - trunc(d/L + sign(d)/2) L plus the boxes -1, 0, +1 in every
periodic direction.  in_plane: the z row and column of tt, the z row / column entries of tr the oracle masks.

The separations are formed from the float64 positions in `dtype`: with dtype = EXT (np.longdouble, 64-bit mantissa) they
are exact, and every block is good to ~2^-64 of `scale`: the yardstick of the HIP pair algebra (pair_ops.h, pair_blocks*.h),
which is deliberately NOT this algebra (closed-form wall polynomials, unscaled positions, folded constants, rsqrt + one
cubic step).  dtype = np.float64 is the oracle's arithmetic in numpy, dtype = np.float32 the reference's
`precision = 'single'` arithmetic on separations taken exactly from the float64 positions.

The metric:  err_ij,cd / (eps * s_ij),   s_ij = (1/(8 pi eta)) sum_boxes (1/max(r_ij, a)^p + [image] / R_ij^p) * |b_i b_j|,
p = 1 (tt), 2 (tr, rt), 3 (rr); self blocks 1/a^p plus the image term at R = 2 z.  (b_i b_j: a damped block is smaller by
that factor and so are its roundings; without it a blob at z = a/2 would be tested four times as loosely.)

C_ORACLE / C_ORACLE32: the worst value of that metric for the fp64 oracle (eps = 2^-53) and for the float32 restatement
(eps = 2^-24) against EXT on the regime clouds below -- measured by tests/test_pair_blocks_host.py, which asserts that the
recomputed values do not exceed the table.  Regenerate with

    python -m pytest tests/test_pair_blocks_host.py -k yardstick -s        (prints both tables)

The GPU test allows MARGIN times these per element.  They come from the reference side only, never from a kernel."""
import numpy as np

LONG_DOUBLE = np.finfo(np.longdouble).nmant >= 63
EXT = np.longdouble if LONG_DOUBLE else np.float64

KINDS = ("tt", "tr", "rt", "rr")
POWER = {"tt": 1, "tr": 2, "rt": 2, "rr": 3}
_PI = "3.14159265358979323846264338327950288"
MARGIN = 4.0

# (kind, boundary, periodic) -> worst |oracle_fp64 - EXT| / (2^-53 s) over the regime clouds (open: plain + offset cloud;
# periodic: the two boxes), rounded up.  Measured on x86-64 (80-bit long double), gcc -O2 oracle.
C_ORACLE = {
    ("tt", "none", False): 14.0, ("tt", "wall", False): 13.0, ("tt", "free", False): 13.0,       # measured 13.27, 12.10, 12.29
    ("tr", "none", False): 8.0, ("tr", "wall", False): 17.0, ("tr", "free", False): 7.0,         # 7.14, 16.34, 6.95
    ("rt", "none", False): 8.0, ("rt", "wall", False): 17.0, ("rt", "free", False): 7.0,         # 7.14, 16.34, 6.95
    ("rr", "none", False): 16.0, ("rr", "wall", False): 21.0, ("rr", "free", False): 16.0,       # 15.56, 20.98, 15.09
    # in a box the oracle wraps in fp64, r - (double)k * L: the product k L is rounded at the size of the UNWRAPPED
    # difference (hundreds of a) and the error lands on a wrapped separation of a few a -- its own conditioning, in every kind
    ("tt", "none", True): 115.0, ("tt", "wall", True): 111.0, ("tt", "free", True): 113.0,       # 114.85, 110.21, 112.77
    ("tr", "none", True): 164.0, ("tr", "wall", True): 165.0, ("tr", "free", True): 164.0,       # 163.18, 164.22, 163.21
    ("rt", "none", True): 164.0, ("rt", "wall", True): 164.0, ("rt", "free", True): 164.0,       # 163.18, 163.63, 163.21
    ("rr", "none", True): 254.0, ("rr", "wall", True): 254.0, ("rr", "free", True): 255.0,       # 253.24, 253.31, 254.26
}
# the same for blocks(..., dtype=np.float32) in units of 2^-24 s (open boundaries: the fp32 kernels have no periodic twin)
C_ORACLE32 = {
    ("tt", "none"): 16.0, ("tt", "wall"): 10.0, ("tt", "free"): 15.0,        # measured 15.38, 9.79, 14.69
    ("tr", "none"): 8.0, ("tr", "wall"): 15.0, ("tr", "free"): 7.0,          # 7.45, 14.25, 6.58
    ("rt", "none"): 8.0, ("rt", "wall"): 15.0, ("rt", "free"): 7.0,          # 7.45, 14.25, 6.58
    ("rr", "none"): 15.0, ("rr", "wall"): 24.0, ("rr", "free"): 15.0,        # 14.10, 23.89, 14.09
}


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
def _outer(c, s):
  return (c[..., None, None] * s[..., :, None]) * s[..., None, :]


def _eye(c):
  return c[..., None, None] * np.eye(3, dtype=c.dtype)


def _cross_matrix(c, s):
  """c eps.s as the oracle writes it: M[0,1] = c s_z, M[0,2] = -c s_y, M[1,2] = c s_x, antisymmetric."""
  M = np.zeros(c.shape + (3, 3), dtype=c.dtype)
  M[..., 0, 1] = c * s[..., 2]; M[..., 0, 2] = -(c * s[..., 1]); M[..., 1, 2] = c * s[..., 0]
  M[..., 1, 0] = -M[..., 0, 1]; M[..., 2, 0] = -M[..., 0, 2]; M[..., 2, 1] = -M[..., 1, 2]
  return M


def _safe(r, self_mask):
  return np.where(self_mask, np.ones_like(r), r)


def _rpy(kind, s, self_mask):
  """Unbounded block of separations s (..., 3) in units of a (rpy_tt / rpy_coupling / rpy_rr of the oracle)."""
  T = s.dtype.type
  r2 = s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1] + s[..., 2] * s[..., 2]
  r = _safe(np.sqrt(r2), self_mask)
  r2 = _safe(r2, self_mask)
  with np.errstate(all="ignore"):
    if kind == "tt":
      invr = T(1) / r
      invr2 = invr * invr
      far = _eye((T(1) + T(2) / (T(3) * r2)) * invr) + _outer((T(1) - T(2) * invr2) * invr2, s) * invr[..., None, None]
      near = _eye((T(4) / T(3)) * (T(1) - T(0.28125) * r)) + _outer((T(4) / T(3)) * T(0.09375) * invr, s)
      M = np.where((r > 2)[..., None, None], far, near)
      own = (T(4) / T(3)) * np.eye(3, dtype=s.dtype)
    elif kind in ("tr", "rt"):
      far = _cross_matrix(T(1) / (r2 * r), s)
      near = _cross_matrix(T(0.5) * (T(1) - T(0.375) * r), s)
      M = np.where((r >= 2)[..., None, None], far, near)
      own = np.zeros((3, 3), dtype=s.dtype)
    else:
      r3 = r2 * r
      invr3 = T(1) / r3
      far = (_eye(np.full_like(r, -0.5)) + _outer(T(1.5) / r2, s)) * invr3[..., None, None]
      near = _eye(T(1) - T(0.84375) * r + T(0.078125) * r3) + _outer(T(0.28125) / r - T(0.046875) * r, s)
      M = np.where((r >= 2)[..., None, None], far, near)
      own = np.eye(3, dtype=s.dtype)
  return np.where(self_mask[..., None, None], own, M)


def _wall(kind, sx, sy, Rz, h, self_mask):
  """Swan & Brady correction (wall_tt / wall_tr / wall_rt / wall_rr of the oracle): (sx, sy) in-plane separation, Rz the
  height sum, h the anchoring height, all in units of a.  For tr the caller passes the NEGATED in-plane separation and the
  TARGET height."""
  T = sx.dtype.type
  W = np.zeros(sx.shape + (3, 3), dtype=sx.dtype)
  with np.errstate(all="ignore"):
    invR = T(1) / np.sqrt(sx * sx + sy * sy + Rz * Rz)
    ex, ey, ez = sx * invR, sy * invR, Rz * invR
    e = (ex, ey, ez)
    hh = h / Rz
    iZ = T(1) / h
    if kind == "tt":
      invR3 = invR * invR * invR
      invR5 = invR3 * invR * invR
      ez2 = ez * ez
      f1 = -(T(3) * (T(1) + T(2) * hh * (T(1) - hh) * ez2) * invR + T(2) * (T(1) - T(3) * ez2) * invR3 - T(2) * (T(1) - T(5) * ez2) * invR5) / T(3)
      f2 = -(T(3) * (T(1) - T(6) * hh * (T(1) - hh) * ez2) * invR - T(6) * (T(1) - T(5) * ez2) * invR3 + T(10) * (T(1) - T(7) * ez2) * invR5) / T(3)
      f3 = ez * (T(3) * hh * (T(1) - T(6) * (T(1) - hh) * ez2) * invR - T(6) * (T(1) - T(5) * ez2) * invR3 + T(10) * (T(2) - T(7) * ez2) * invR5) * T(2) / T(3)
      f4 = ez * (T(3) * hh * invR - T(10) * invR5) * T(2) / T(3)
      f5 = -(T(3) * hh * hh * ez2 * invR + T(3) * ez2 * invR3 + (T(2) - T(15) * ez2) * invR5) * T(4) / T(3)
      for p in range(3):
        for q in range(3):
          W[..., p, q] = f2 * e[p] * e[q]
        W[..., p, p] += f1
      for p in range(2):
        W[..., p, 2] += f3 * e[p]
        W[..., 2, p] += f4 * e[p]
      W[..., 2, 2] += f3 * ez + f4 * ez + f5
      iZ3 = iZ * iZ * iZ
      iZ5 = iZ3 * iZ * iZ
      par = -(T(9) * iZ - T(2) * iZ3 + iZ5) / T(12)
      own = (par, par, -(T(9) * iZ - T(4) * iZ3 + iZ5) / T(6))
    elif kind in ("tr", "rt"):
      invR2 = invR * invR
      invR4 = invR2 * invR2
      f1 = invR2
      f2 = (T(6) * hh * ez * ez * invR2 + (T(1) - T(10) * ez * ez) * invR4) * T(2)
      f3 = -ez * (T(3) * hh * invR2 - T(5) * invR4) * T(2)
      f4 = -ez * (hh * invR2 - invR4) * T(2)
      a01 = -f1 * ez + f3 * ex * ex - f4
      a10 = f1 * ez - f3 * ey * ey + f4
      col = (-f1 * ey - f2 * ey - f3 * ey * ez, f1 * ex + f2 * ex + f3 * ex * ez)
      W[..., 0, 0] = f3 * ex * ey
      W[..., 1, 1] = -(f3 * ex * ey)
      if kind == "tr":      # M -= (...)
        W[..., 0, 1] = -a01; W[..., 1, 0] = -a10
        W[..., 0, 2] = -(f1 * ey); W[..., 1, 2] = f1 * ex
        W[..., 2, 0] = -col[0]; W[..., 2, 1] = -col[1]
      else:                 # the transposed pattern
        W[..., 0, 1] = -a10; W[..., 1, 0] = -a01
        W[..., 2, 0] = -(f1 * ey); W[..., 2, 1] = f1 * ex
        W[..., 0, 2] = -col[0]; W[..., 1, 2] = -col[1]
      iZ4 = iZ * iZ * iZ * iZ
      own = None
    else:
      invR3 = invR * invR * invR
      f1 = ((T(1) - T(6) * ez * ez) * invR3) * T(0.5)
      f2 = -(T(9) * invR3) / T(6)
      f3 = T(3) * invR3 * ez
      f4 = T(3) * invR3
      W[..., 0, 0] = f1 + f2 * ex * ex + f4 * ey * ey
      W[..., 0, 1] = (f2 - f4) * ex * ey
      W[..., 0, 2] = f2 * ex * ez
      W[..., 1, 0] = (f2 - f4) * ex * ey
      W[..., 1, 1] = f1 + f2 * ey * ey + f4 * ex * ex
      W[..., 1, 2] = f2 * ey * ez
      W[..., 2, 0] = f2 * ez * ex + f3 * ex
      W[..., 2, 1] = f2 * ez * ey + f3 * ey
      W[..., 2, 2] = f1 + f2 * ez * ez + f3 * ez
      iZ3 = iZ * iZ * iZ
      own = (-iZ3 * T(0.3125), -iZ3 * T(0.3125), -iZ3 * T(0.125))
  S = np.zeros_like(W)
  if own is None:           # tr: M[0,1] -= -iZ4/8, M[1,0] -= iZ4/8;  rt: M[0,1] += -iZ4/8, M[1,0] += iZ4/8
    sgn = T(1) if kind == "tr" else T(-1)
    S[..., 0, 1] = sgn * iZ4 * T(0.125)
    S[..., 1, 0] = -sgn * iZ4 * T(0.125)
  else:
    for p in range(3):
      S[..., p, p] = own[p]
  return np.where(self_mask[..., None, None], S, W)


_TT_MASK = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=bool)
_TR_MASK = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], dtype=bool)


def _wrap(d, Lk):
  return d - np.trunc(d / Lk + d.dtype.type(0.5) * np.sign(d)) * Lk


def _boxes(L):
  rng = [(-1, 0, 1) if L[k] > 0 else (0,) for k in range(3)]
  return [(bx, by, bz) for bx in rng[0] for by in rng[1] for bz in rng[2]]


def _period(L):
  return np.zeros(3) if L is None else np.asarray(L, dtype=np.float64).reshape(3)


def wall_heights(r, a):
  """(z clamped as the wrappers do, damping factor b) in float64: z <= a -> a;  b = z/a for z < a, else 1."""
  z = np.asarray(r, dtype=np.float64).reshape(-1, 3)[:, 2]
  return np.where(z <= a, a, z), np.where(z < a, z / a, 1.0)


def blocks(kind, boundary, r, a, eta, L=None, dtype=EXT, in_plane=False, rows=None):
  """rows: indices of the target blobs to evaluate (default all): (len(rows), N, 3, 3)."""
  if kind not in KINDS or boundary not in ("none", "wall", "free"):
    raise ValueError((kind, boundary))
  if in_plane and (kind not in ("tt", "tr") or boundary != "wall"):
    raise ValueError("in_plane: tt / tr above the wall")
  T = np.dtype(dtype).type
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  n = len(r)
  L = _period(L)
  x = r.copy()
  damp = np.ones(n, dtype=dtype)
  if boundary == "wall":
    z, b = wall_heights(r, a)
    x[:, 2] = z
    zc = np.asarray(r[:, 2], dtype=dtype)
    damp = np.where(np.asarray(b) < 1.0, zc / T(a), T(1))         # the quotient in `dtype`
  # separations: in EXT the differences of float64 numbers are exact; float32 takes them from the float64 positions
  wide = np.float64 if np.dtype(dtype) == np.dtype(np.float32) else dtype
  rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
  m = len(rows)
  xw = x.astype(wide)
  d0 = xw[rows, None, :] - xw[None, :, :]
  for k in range(3):
    if L[k] > 0:
      d0[..., k] = _wrap(d0[..., k], np.dtype(wide).type(L[k]))
  Rz = (xw[rows, None, 2] + xw[None, :, 2]).astype(dtype)
  zi = np.broadcast_to(x[rows, None, 2].astype(dtype), (m, n))
  zj = np.broadcast_to(x[None, :, 2].astype(dtype), (m, n))
  inva = T(1) / T(a)
  norm = T(1) / (T(8) * T(_PI) * T(eta) * T(a) ** POWER[kind])
  eye = rows[:, None] == np.arange(n)[None, :]
  no_self = np.zeros((m, n), dtype=bool)
  M = np.zeros((m, n, 3, 3), dtype=dtype)
  for box in _boxes(L):
    d = d0.copy()
    for k in range(3):
      if box[k]:
        d[..., k] = d[..., k] + np.dtype(wide).type(box[k]) * np.dtype(wide).type(L[k])
    s = d.astype(dtype) * inva
    own = eye if box == (0, 0, 0) else no_self
    B = _rpy(kind, s, own)
    if boundary == "wall":
      if in_plane:
        B = np.where(_TT_MASK if kind == "tt" else _TR_MASK, B, T(0))
      if kind == "tr":
        W = _wall(kind, -s[..., 0], -s[..., 1], Rz * inva, zi * inva, own)
      else:
        W = _wall(kind, s[..., 0], s[..., 1], Rz * inva, zj * inva, own)
      if in_plane:
        W = np.where(_TT_MASK if kind == "tt" else _TR_MASK, W, T(0))
      B = B + W
    elif boundary == "free":
      sR = s.copy()
      sR[..., 2] = Rz * inva
      I = _rpy(kind, sR, no_self).copy()
      I[..., :, 2] = -I[..., :, 2]                                   # B(R) S
      B = B + I if kind in ("tt", "rt") else B - I
    M = M + B * norm
  return M * (damp[rows, None] * damp[None, :])[..., None, None]


def dense(M):
  """(M, N, 3, 3) -> (3M, 3N)"""
  return M.transpose(0, 2, 1, 3).reshape(3 * M.shape[0], 3 * M.shape[1])


def from_dense(D):
  """(3M, 3N) -> (M, N, 3, 3)"""
  return D.reshape(D.shape[0] // 3, 3, D.shape[1] // 3, 3).transpose(0, 2, 1, 3)


def scale(kind, boundary, r, a, eta, L=None):
  """s_ij in EXT (see the module text)."""
  p = POWER[kind]
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  n = len(r)
  L = _period(L)
  x = r.copy()
  damp = np.ones(n, dtype=EXT)
  if boundary == "wall":
    x[:, 2], b = wall_heights(r, a)
    damp = np.abs(np.where(b < 1.0, r[:, 2].astype(EXT) / EXT(a), EXT(1)))
  xw = x.astype(EXT)
  d0 = xw[:, None, :] - xw[None, :, :]
  for k in range(3):
    if L[k] > 0:
      d0[..., k] = _wrap(d0[..., k], EXT(L[k]))
  Rz = xw[:, None, 2] + xw[None, :, 2]
  s = np.zeros((n, n), dtype=EXT)
  for box in _boxes(L):
    d = d0 + np.array(box, dtype=EXT) * L.astype(EXT)
    rho2 = d[..., 0] ** 2 + d[..., 1] ** 2
    dist = np.maximum(np.sqrt(rho2 + d[..., 2] ** 2), EXT(a))
    s = s + EXT(1) / dist ** p
    if boundary != "none":
      s = s + EXT(1) / np.sqrt(rho2 + Rz ** 2) ** p
  return s / (EXT(8) * EXT(_PI) * EXT(eta)) * (damp[:, None] * damp[None, :])


def worst_ratio(got, ref, s, eps):
  """max over pairs and elements of |got - ref| / (eps s), and where: (ratio, i, j, c, d)."""
  err = np.abs(np.asarray(got, dtype=EXT) - ref) / (EXT(eps) * s[..., None, None])
  k = int(np.argmax(err))
  i, j, c, d = np.unravel_index(k, err.shape)
  return float(err.reshape(-1)[k]), int(i), int(j), int(c), int(d)


# ---------------------------------------------------------------------------------------------------------------------
# the designed configuration
# ---------------------------------------------------------------------------------------------------------------------
HEIGHTS = (0.6, 1.0, 1.0 + 1e-9, 1.1, 3.0, 1.0e3)                       # z/a of the six groups
SEPARATIONS = (1e-7, 0.5, 2.0 - 4e-12, 2.0, 2.0 + 4e-12, 2.5, 10.0)     # r/a of an anchor's partners
DIRECTIONS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.6, 0.0, 0.8))
N_CLOUD = 200                                                           # three full 64-blob tiles and one of eight
BOXES = {"odd": (61.7, 93.1, 0.0), "pow2": (64.0, 128.0, 0.0)}          # in units where a = 0.5


def ties(r, L, tol=1e-9):
  """Number of unordered pairs with |d/L - (k + 1/2)| < tol in a periodic direction: at an exact tie the image choice
  legitimately changes the block, so such inputs are not compared."""
  L = _period(L)
  x = np.asarray(r, dtype=np.float64).reshape(-1, 3).astype(EXT)
  bad = np.zeros((len(x), len(x)), dtype=bool)
  for k in range(3):
    if L[k] > 0:
      q = (x[:, None, k] - x[None, :, k]) / EXT(L[k])
      bad |= np.abs(q - np.floor(q) - EXT(0.5)) < tol
  return int(np.triu(bad, 1).sum())


def untie(r, L, tol=1e-9, step=2e-8):
  """Rebuild an input that fails the tie check: the later blob of every tied pair moves by step L in the tied direction
  (as points_with_margin does for the histogram), until none is left."""
  L = _period(L)
  r = np.array(r, dtype=np.float64).reshape(-1, 3)
  for _ in range(64):
    if ties(r, L, tol) == 0:
      return r
    x = r.astype(EXT)
    for k in range(3):
      if L[k] > 0:
        q = (x[:, None, k] - x[None, :, k]) / EXT(L[k])
        bad = np.triu(np.abs(q - np.floor(q) - EXT(0.5)) < tol, 1)
        r[np.unique(np.nonzero(bad)[1]), k] += step * L[k]
  raise RuntimeError("untie: ties left after 64 passes")


def regime_cloud(a, periodic=False, offset=0.0):
  """The designed configuration: (r (N_CLOUD, 3) float64, L or None).  Six groups, one per height of HEIGHTS, each an anchor
  blob and a partner at every separation of SEPARATIONS along every direction of DIRECTIONS; the groups stand 1000 a apart
  (the far field along the wall), or 2.37 periods apart in a box (`periodic`: "odd" or "pow2", lengths of BOXES scaled by
  a / 0.5), where two more blobs sit 3e-7 of a period from the half period of an anchor.  A blob at 1000 a right above the
  lowest anchor, two free ones, the rest seeded fill; listed in a seeded random order, so that designed pairs fall inside
  one 64-blob tile and across tiles, the partial last one included.  offset: added to every x and y."""
  L = None
  if periodic:
    L = np.array(BOXES[periodic]) * (a / 0.5)
  pts, anchors = [], []
  for g, h in enumerate(HEIGHTS):
    if L is None:
      anchor = np.array([1000.0 * a * g, 17.0 * a * g, h * a])
    else:
      anchor = np.array([2.37 * L[0] * g, 1.21 * L[1] * g, h * a])
    pts.append(anchor)
    anchors.append(anchor)
    for sep in SEPARATIONS:
      if offset and abs(sep - 2.0) < 1e-9 and sep != 2.0:
        continue                    # not representable next to the offset: they would fall onto the r = 2a partner
      for dr in DIRECTIONS:
        if h < 1.0 and dr[2] == 1.0 and h + sep <= 1.0:
          continue                  # the wall clamp would put it onto its anchor
        pts.append(anchor + sep * a * np.array(dr))
    if L is not None and g in (1, 4):
      pts.append(anchor + np.array([L[0] * (0.5 - 3e-7), 0.0, 0.0]))
      pts.append(anchor + np.array([0.0, L[1] * (1.5 + 3e-7), 2.0 * a]))
  pts.append(pts[0] + np.array([0.0, 0.0, 1000.0 * a]))              # stacked 1000 a above the lowest anchor
  pts.append(np.array([3.0 * a, 40.0 * a, 0.3 * a]))                  # a second and third damped blob, in contact
  pts.append(np.array([3.0 * a, 41.5 * a, 0.9 * a]))
  rng = np.random.RandomState(1234)
  while len(pts) < N_CLOUD:
    g = rng.randint(len(HEIGHTS) - 1)
    pts.append(anchors[g] * np.array([1.0, 1.0, 0.0]) + a * np.array([30 * rng.rand() - 15, 30 * rng.rand() + 4, 1.0 + 4 * rng.rand()]))
  r = np.array(pts[:N_CLOUD])
  assert len(pts) == N_CLOUD
  r = r[np.random.RandomState(99).permutation(N_CLOUD)]
  r[:, :2] += offset
  if L is not None:
    r = untie(r, L)
  return r, L


def coverage(r, a, L=None):
  """Counts of the ordered pairs i != j (nearest image) and of the blobs in each regime class."""
  L = _period(L)
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  x = r.astype(EXT)
  n = len(x)
  d = x[:, None, :] - x[None, :, :]
  raw = d.copy()
  for k in range(3):
    if L[k] > 0:
      d[..., k] = _wrap(d[..., k], EXT(L[k]))
  off = ~np.eye(n, dtype=bool)
  rho2 = d[..., 0] ** 2 + d[..., 1] ** 2
  r2 = rho2 + d[..., 2] ** 2
  q = np.sqrt(r2) / EXT(a)
  flat = (d[..., 2] == 0) & off
  stacked = (rho2 == 0) & off
  below = (q < 2) & (2 - q <= 1e-11) & off
  above = (q > 2) & (q - 2 <= 1e-11) & off
  exact = (r2 == 4 * EXT(a) * EXT(a)) & off
  z = x[:, 2] / EXT(a)
  with np.errstate(divide="ignore", invalid="ignore"):
    ratio = np.where(x[None, :, 2] > 0, x[:, None, 2] / x[None, :, 2], 0)
  upper = np.triu(np.ones((n, n), dtype=bool), 1)
  c = {
      "near2_below_inplane": int((below & flat).sum()), "near2_below_vertical": int((below & stacked).sum()),
      "near2_above_inplane": int((above & flat).sum()), "near2_above_vertical": int((above & stacked).sum()),
      "exact2_inplane": int((exact & flat).sum()), "exact2_vertical": int((exact & stacked).sum()),
      "coincident": int(((q <= 1e-6) & off).sum()), "exactly_coincident": int(((r2 == 0) & off).sum()),
      "overlap": int(((q > 0.1) & (q < 1.9) & off).sum()), "mid": int(((q > 2.1) & (q < 20) & off).sum()),
      "far_low": int(((q >= 1e3) & (z[:, None] <= 3) & (z[None, :] <= 3) & off).sum()),
      "stacked": int(stacked.sum()), "inplane": int(flat.sum()),
      "z_below": int((z < 1).sum()), "z_exact": int((z == 1).sum()), "z_just_above": int(((z > 1) & (z <= 1 + 2e-9)).sum()),
      "z_high": int((z >= 1e3).sum()),
      "zratio_ij": int(((ratio >= 1e3) & upper).sum()), "zratio_ji": int(((ratio >= 1e3) & upper.T).sum()),
      "offset": int(((np.abs(x[:, 0]) >= 5e5 * a) & (np.abs(x[:, 1]) >= 5e5 * a)).sum()),
      "cross_edge": 0, "beyond_period": 0, "half_period": 0, "ties": ties(r, L),
  }
  for k in range(3):
    if L[k] > 0:
      Lk = EXT(L[k])
      t = raw[..., k] / Lk
      frac = np.abs(t - np.floor(t) - EXT(0.5))
      c["cross_edge"] += int(((d[..., k] != raw[..., k]) & (np.abs(raw[..., k]) < Lk) & off).sum())
      c["beyond_period"] += int(((np.abs(raw[..., k]) > Lk) & off).sum())
      c["half_period"] += int(((frac >= 1e-9) & (frac < 1e-6) & off).sum())
  return c


OPEN_CLASSES = ("near2_below_inplane", "near2_below_vertical", "near2_above_inplane", "near2_above_vertical", "exact2_inplane",
                "exact2_vertical", "coincident", "overlap", "mid", "far_low", "stacked", "inplane", "z_below", "z_exact",
                "z_just_above", "z_high", "zratio_ij", "zratio_ji")
PERIODIC_CLASSES = tuple(k for k in OPEN_CLASSES if k != "far_low") + ("cross_edge", "beyond_period", "half_period")
# at |x|, |y| ~ 1e6 a one unit in the last place of a coordinate is 1e-10 a: separations of 2 a -+ 4e-12 a do not exist there
OFFSET_CLASSES = tuple(k for k in OPEN_CLASSES if not k.startswith("near2")) + ("offset",)


def assert_coverage(r, a, L=None, classes=OPEN_CLASSES):
  c = coverage(r, a, L)
  missing = [k for k in classes if c[k] < 1]
  assert not missing, (missing, c)
  assert c["exactly_coincident"] == 0 and c["ties"] == 0, c
  if "offset" in classes:
    assert c["offset"] == len(np.asarray(r).reshape(-1, 3)), c
  return c


def regime_of(r, a, i, j, L=None):
  """The regime classes of one pair, for a failure message."""
  x = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  if i == j:
    return "self z/a=%.9g" % (x[i, 2] / a)
  d = (x[i] - x[j]).astype(EXT)
  L = _period(L)
  for k in range(3):
    if L[k] > 0:
      d[k] = _wrap(d[k:k + 1], EXT(L[k]))[0]
  q = float(np.sqrt((d ** 2).sum()) / EXT(a))
  tags = ["r/a=%.17g" % q, "z_i/a=%.9g" % (x[i, 2] / a), "z_j/a=%.9g" % (x[j, 2] / a)]
  if d[2] == 0:
    tags.append("in-plane")
  if d[0] == 0 and d[1] == 0:
    tags.append("stacked")
  if abs(q - 2) <= 1e-11:
    tags.append("at the r = 2a switch")
  return " ".join(tags)


# ---------------------------------------------------------------------------------------------------------------------
# the four clouds of the tests, their EXT blocks (computed once per process), and the fp64 oracle in block form
# ---------------------------------------------------------------------------------------------------------------------
A, ETA = 0.5, 1.3          # a = 1/2: r = 2a is the representable number 1
CLOUDS = {"open": (False, 0.0, OPEN_CLASSES), "offset": (False, 1.0e6 * A, OFFSET_CLASSES),
          "odd": ("odd", 0.0, PERIODIC_CLASSES), "pow2": ("pow2", 0.0, PERIODIC_CLASSES)}
_cache = {}


def cloud(name):
  """(r, L) of one of CLOUDS, coverage asserted."""
  if ("cloud", name) not in _cache:
    periodic, offset, classes = CLOUDS[name]
    r, L = regime_cloud(A, periodic, offset)
    assert_coverage(r, A, L, classes)
    _cache["cloud", name] = (r, L)
  return _cache["cloud", name]


def reference(name, kind, boundary, in_plane=False):
  """(EXT blocks, scale) of cloud `name`; shared by every test of a process."""
  key = ("ref", name, kind, boundary, bool(in_plane))
  if key not in _cache:
    r, L = cloud(name)
    _cache[key] = (blocks(kind, boundary, r, A, ETA, L, in_plane=in_plane), scale(kind, boundary, r, A, ETA, L))
  return _cache[key]


_SIGN = {"tt": 1.0, "tr": -1.0, "rt": 1.0, "rr": -1.0}       # of the image term B(R) S above a free surface
_STEM = {"tt": "trans_times_force", "tr": "trans_times_torque", "rt": "rot_times_force", "rr": "rot_times_torque"}


def oracle_blocks(oracle, kind, boundary, r, a, eta, L=None, cols=None, in_plane=False):
  """The fp64 oracle (oracle/oracle_mobility.c through oracle/oracle.py) in block form, (N, len(cols), 3, 3); cols: source
  blobs (default all).  Open boundaries: its dense builder -- above a free surface on the doubled system [r; S r] of
  tests/_free_surface_mirror.py.  Pseudo-periodic or in_plane: its products on unit vectors, one per column (every other
  source contributes an exact zero)."""
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  n = len(r)
  L = _period(L)
  cols = np.arange(n) if cols is None else np.asarray(cols, dtype=np.int64)
  if not L.any() and not in_plane:
    if boundary == "free":
      D = oracle.dense(kind, 0, np.concatenate([r, r * np.array([1.0, 1.0, -1.0])]), eta, a)
      I = D[:3 * n, 3 * n:].copy()
      I[:, 2::3] = -I[:, 2::3]
      M = D[:3 * n, :3 * n] + _SIGN[kind] * I
    elif boundary == "wall":
      z, b = wall_heights(r, a)
      x = r.copy(); x[:, 2] = z
      b3 = np.repeat(b, 3)
      M = oracle.dense(kind, 1, x, eta, a) * b3[:, None] * b3[None, :]
    else:
      M = oracle.dense(kind, 0, r, eta, a)
    return from_dense(M)[:, cols]
  import _free_surface_mirror as mirror
  out = np.empty((n, len(cols), 3, 3))
  e = np.zeros(3 * n)
  for c, j in enumerate(cols):
    for q in range(3):
      e[3 * j + q] = 1.0
      if boundary == "free":
        u = mirror.product(oracle, kind, r, e, eta, a, L if L.any() else None)
      else:
        u = oracle._wrapped(kind, 1 if boundary == "wall" else 0, r, e, eta, a, in_plane=in_plane, periodic_length=L)
      out[:, c, :, q] = u.reshape(n, 3)
      e[3 * j + q] = 0.0
  return out
