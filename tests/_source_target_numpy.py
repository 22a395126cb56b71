"""numpy restatement of the source -> target operators, written from oracle/oracle_mobility.c and the formulas -- TEST
infrastructure, the companion of tests/_mobility_numpy.py for the kernels with the most hand-rewritten algebra:

  st_blocks(mode, src, tgt, rad_s, rad_t, eta, L, dtype)    (nt, ns, 3, 3): translation mobility with per-blob radii,
      mode 0 unbounded (Zuk et al., three regimes in r against a_t + a_s and |a_t - a_s|), 1 no-slip wall (the five image
      tensors for unequal radii) WITH the per-blob height clamp z <= a -> a and the damping b = z/a on both sides,
      2 stress-free surface (the three-regime tensor at the mirror image, z column negated, raw heights)
  pressure_rows(wall, src, tgt, dtype)                      (nt, ns, 3): p_t = sum_s row[t, s] . f_s
  dl_blocks(variant, src, tgt, normals, weights, a, dtype)  (nt, ns, 3, 3) acting on `vector`; variant "free" / "wall"
      (pairs with r > 1e-14 only, the image of a node kept) / "rpy" (blob radius a, pairs with r < 1e-14 skipped)
  st_scale / pressure_scale / dl_scale                      the size every rounding bound of a block is stated against

Every block is written ONE TENSOR TERM AT A TIME (c I, c R R^T, c R z^T, c z R^T, c z z^T, added up in the order the formulas
list them): deliberately neither the five scalars alpha .. eps of pair_st / st_coeffs nor the common w/R^5 of aux_pair.
The separations are formed from the float64 inputs in `dtype`: with dtype = EXT (np.longdouble) they are exact and a block
is good to ~2^-64 of its scale; dtype = np.float64 is the oracle's arithmetic, np.float32 the single-precision twin's on
separations taken from the float64 positions.  Pseudo-periodic images follow the oracle's rule (_mobility_numpy._wrap, the
boxes -1, 0, 1 of every periodic direction; the image height sum is NOT wrapped).

Scales (constants of order one do not matter, the yardsticks absorb them):
  st        s_ts = (1/(8 pi eta)) |b_t b_s| sum_boxes (1/max(r, a_>) + [image] 1/max(R, a_>)),  a_> = max(a_t, a_s)
  pressure  (1/(4 pi)) (1/r^2 + [wall] 1/R^2)
  dl        (3/(4 pi)) |w_s| |n_s| ([r > 1e-14] 1/r^2 + [wall] 1/R^2);   rpy: (3/(4 pi)) |w_s| |n_s| (1/r^2 + a^2/r^4)

Yardsticks: the fp64 oracle's worst |oracle - EXT| / (2^-53 s) on the designed clouds below (C_ST, C_P, C_DL), the float32
restatement's in units of 2^-24 s (C_ST32), and the same ratio for whole products at the edge shapes against the per-target
scale sum_s s_ts |f_s|_max (C_*_SUM).  tests/test_source_target_blocks_host.py measures them and asserts that the
recomputed values do not exceed the tables; regenerate with

    python -m pytest tests/test_source_target_blocks_host.py -k yardstick -s

They come from the reference side only, never from a kernel.  The GPU test allows MARGIN times these."""
import numpy as np

import _mobility_numpy as mn
from _mobility_numpy import EXT, MARGIN, _PI, _boxes, _period, _wrap      # noqa: F401  (re-exported)

A, ETA = 0.5, 1.3                  # the base radius (dyadic) and the viscosity of every designed cloud
A_RPY = 0.25                       # blob radius of the RPY double layer
MODES = (0, 1, 2)
DL_VARIANTS = ("free", "wall", "rpy")

# (mode, periodic) -> worst |oracle_fp64 - EXT| / (2^-53 s) over the designed clouds, rounded up.  x86-64, gcc -O2 oracle.
C_ST = {
    (0, False): 11.0, (1, False): 14.0, (2, False): 10.0,         # measured 10.83, 13.05, 9.52
    # in a box the oracle wraps in fp64: the product k L is rounded at the size of the unwrapped difference
    (0, True): 55.0, (1, True): 44.0, (2, True): 45.0,            # 54.69, 43.24, 44.35
}
# blocks(..., dtype=np.float32) in units of 2^-24 s, open boundaries, the sources == targets cloud included (the float
# twin exists for sources == targets, unbounded and above the wall)
C_ST32 = {0: 19.0, 1: 19.0}                                       # measured 18.53, 18.28
C_P = {0: 9.0, 1: 15.0}                                           # measured 8.27, 14.28
C_DL = {"free": 9.0, "wall": 9.0, "rpy": 9.0}                     # measured 8.18, 8.85, 8.16
# whole products at EDGE_SHAPES, random vectors: |oracle - EXT| / (2^-53 sum_s s_ts |f_s|_max) per target
C_ST_SUM = {0: 7.0, 1: 7.0, 2: 10.0}                              # measured 6.73, 6.26, 9.02
C_P_SUM = {0: 6.0, 1: 13.0}                                       # measured 5.67, 12.90
C_DL_SUM = {"free": 3.0, "wall": 6.0, "rpy": 6.0}                 # measured 2.69, 5.24, 5.20

EDGE_SHAPES = ((1, 1), (1, 65), (4, 64), (5, 63), (511, 1), (512, 64), (513, 65), (1025, 129))      # (ns, nt)
EDGE_CHUNKS = (1, 2, 3, 7)


# ---------------------------------------------------------------------------------------------------------------------
# tensor terms
# ---------------------------------------------------------------------------------------------------------------------
def _eye(c):
  return c[..., None, None] * np.eye(3, dtype=c.dtype)


def _outer(c, u, v):
  return c[..., None, None] * u[..., :, None] * v[..., None, :]


def _zz(c):
  J = np.zeros((3, 3), dtype=c.dtype); J[2, 2] = 1
  return c[..., None, None] * J


def _zuk(d, at, as_):
  """The unbounded tensor C1 I + C2 d d^T of two blobs of radii at, as_ at separation d (..., 3), three regimes."""
  T = d.dtype.type
  r2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
  r = np.sqrt(r2)
  s2 = as_ * as_ + at * at
  with np.errstate(all="ignore"):
    far1 = (T(1) + s2 / (T(3) * r2)) / r
    far2 = ((T(1) - s2 / r2) / r2) / r
    r3 = r2 * r
    dm = (as_ - at) * (as_ - at)
    mid1 = ((T(16) * (as_ + at) * r3 - (dm + T(3) * r2) * (dm + T(3) * r2)) / (T(32) * r3)) * (T(4) / T(3)) / (as_ * at)
    mid2 = ((T(3) * (dm - r2) * (dm - r2) / (T(32) * r3)) / r2) * (T(4) / T(3)) / (as_ * at)
    in1 = (T(4) / T(3)) / np.maximum(at, as_)
  far = r > at + as_
  mid = ~far & (r > np.abs(as_ - at))
  C1 = np.where(far, far1, np.where(mid, mid1, in1))
  C2 = np.where(far, far2, np.where(mid, mid2, T(0)))
  return _eye(C1) + _outer(C2, d, d)


def _wall_image(R, x3, y3, at, as_):
  """T(R) of the no-slip wall for unequal radii: the sum of five tensors, each term on its own.  R = (d_x, d_y, x3 + y3),
  x3 / y3 the target / source height."""
  T = R.dtype.type
  z = np.zeros_like(R); z[..., 2] = 1
  R2 = R[..., 0] * R[..., 0] + R[..., 1] * R[..., 1] + R[..., 2] * R[..., 2]
  Rn = np.sqrt(R2)
  R3 = R2 * Rn; R5 = R3 * R2; R7 = R5 * R2; R9 = R7 * R2
  a2, b2, rz = at * at, as_ * as_, R[..., 2]
  with np.errstate(all="ignore"):
    # G_ab(R)
    W = _eye((T(1) + (b2 + a2) / (T(3) * R2)) / Rn)
    W = W + _outer((T(1) - (b2 + a2) / R2) / R2 / Rn, R, R)
    # 2 (-J/R - R x3 z^T/R^3 - y3 z R^T/R^3 + x3 y3 (I/R^3 - 3 R R^T/R^5))
    W = W + _zz(-T(2) / Rn)
    W = W + _outer(-T(2) * x3 / R3, R, z)
    W = W + _outer(-T(2) * y3 / R3, z, R)
    W = W + _eye(T(2) * x3 * y3 / R3)
    W = W + _outer(-T(6) * x3 * y3 / R5, R, R)
    # (2 a_t^2/3)(-J/R^3 + 3 rz R z^T/R^5 - y3 (3 rz I/R^5 + 3 z R^T/R^5 + 3 R z^T/R^5 - 15 rz R R^T/R^7))
    c = T(2) * a2 / T(3)
    W = W + _zz(-c / R3)
    W = W + _outer(c * T(3) * rz / R5, R, z)
    W = W + _eye(-c * y3 * T(3) * rz / R5)
    W = W + _outer(-c * y3 * T(3) / R5, z, R)
    W = W + _outer(-c * y3 * T(3) / R5, R, z)
    W = W + _outer(c * y3 * T(15) * rz / R7, R, R)
    # (2 a_s^2/3)(-J/R^3 + 3 rz z R^T/R^5 - x3 (the same bracket))
    c = T(2) * b2 / T(3)
    W = W + _zz(-c / R3)
    W = W + _outer(c * T(3) * rz / R5, z, R)
    W = W + _eye(-c * x3 * T(3) * rz / R5)
    W = W + _outer(-c * x3 * T(3) / R5, z, R)
    W = W + _outer(-c * x3 * T(3) / R5, R, z)
    W = W + _outer(c * x3 * T(15) * rz / R7, R, R)
    # (2 a_t^2 a_s^2/3)(-I/R^5 + 5 rz^2 I/R^7 - 2 J/R^5 + 10 rz (z R^T + R z^T)/R^7 + 5 R R^T/R^7 - 35 rz^2 R R^T/R^9)
    c = T(2) * a2 * b2 / T(3)
    W = W + _eye(c * (-T(1) / R5 + T(5) * rz * rz / R7))
    W = W + _zz(-T(2) * c / R5)
    W = W + _outer(c * T(10) * rz / R7, z, R)
    W = W + _outer(c * T(10) * rz / R7, R, z)
    W = W + _outer(c * (T(5) / R7 - T(35) * rz * rz / R9), R, R)
  return W


def st_heights(pos, rad, mode):
  """(effective height, damping factor b) in float64 as the wrappers form them: mode 1 clamps z <= a to a and damps a blob
  with z < a by z/a; the other modes take the raw height."""
  pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
  rad = np.broadcast_to(np.asarray(rad, dtype=np.float64).reshape(-1), (len(pos),))
  z = pos[:, 2]
  if mode != 1:
    return z.copy(), np.ones(len(pos))
  return np.where(z > rad, z, rad), np.where(z < rad, z / np.where(rad > 0, rad, 1.0), 1.0)


def _st_setup(mode, src, tgt, rad_s, rad_t, L, dtype):
  T = np.dtype(dtype).type
  src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
  tgt = np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
  rs = np.ascontiguousarray(np.broadcast_to(np.asarray(rad_s, dtype=np.float64).reshape(-1), (len(src),)))
  rt = np.ascontiguousarray(np.broadcast_to(np.asarray(rad_t, dtype=np.float64).reshape(-1), (len(tgt),)))
  L = _period(L)
  xs, xt = src.copy(), tgt.copy()
  xs[:, 2], bs = st_heights(src, rs, mode)
  xt[:, 2], bt = st_heights(tgt, rt, mode)
  with np.errstate(all="ignore"):          # the quotient z/a in `dtype`
    ds = np.where(bs < 1.0, src[:, 2].astype(dtype) / np.where(rs > 0, rs, 1.0).astype(dtype), T(1))
    dt = np.where(bt < 1.0, tgt[:, 2].astype(dtype) / np.where(rt > 0, rt, 1.0).astype(dtype), T(1))
  wide = np.float64 if np.dtype(dtype) == np.dtype(np.float32) else dtype
  d0 = xt.astype(wide)[:, None, :] - xs.astype(wide)[None, :, :]
  for k in range(3):
    if L[k] > 0:
      d0[..., k] = _wrap(d0[..., k], np.dtype(wide).type(L[k]))
  Rz = xt.astype(wide)[:, None, 2] + xs.astype(wide)[None, :, 2]
  return xs, xt, rs, rt, L, ds, dt, wide, d0, Rz


def st_blocks(mode, src, tgt, rad_s, rad_t, eta, L=None, dtype=EXT):
  if mode not in MODES:
    raise ValueError(mode)
  T = np.dtype(dtype).type
  xs, xt, rs, rt, L, ds, dt, wide, d0, Rz = _st_setup(mode, src, tgt, rad_s, rad_t, L, dtype)
  nt, ns = len(xt), len(xs)
  at = np.broadcast_to(rt.astype(dtype)[:, None], (nt, ns))
  as_ = np.broadcast_to(rs.astype(dtype)[None, :], (nt, ns))
  x3 = np.broadcast_to(xt[:, 2].astype(dtype)[:, None], (nt, ns))
  y3 = np.broadcast_to(xs[:, 2].astype(dtype)[None, :], (nt, ns))
  pref = T(1) / (T(8) * T(_PI) * T(eta))
  M = np.zeros((nt, ns, 3, 3), dtype=dtype)
  for box in _boxes(L):
    d = d0.copy()
    for k in range(3):
      if box[k]:
        d[..., k] = d[..., k] + np.dtype(wide).type(box[k]) * np.dtype(wide).type(L[k])
    d = d.astype(dtype)
    B = _zuk(d, at, as_)
    if mode:
      R = d.copy()
      R[..., 2] = Rz.astype(dtype)
      I = (_zuk(R, at, as_) if mode == 2 else -_wall_image(R, x3, y3, at, as_)).copy()
      I[..., :, 2] = -I[..., :, 2]                # T(R) P, P = diag(1, 1, -1)
      B = B + I
    M = M + B * pref
  return M * (dt[:, None] * ds[None, :])[..., None, None]


def st_scale(mode, src, tgt, rad_s, rad_t, eta, L=None):
  xs, xt, rs, rt, L, ds, dt, wide, d0, Rz = _st_setup(mode, src, tgt, rad_s, rad_t, L, EXT)
  big = np.maximum(rt.astype(EXT)[:, None], rs.astype(EXT)[None, :])
  s = np.zeros(d0.shape[:2], dtype=EXT)
  with np.errstate(divide="ignore"):
    for box in _boxes(L):
      d = d0 + np.array(box, dtype=EXT) * L.astype(EXT)
      rho2 = d[..., 0] ** 2 + d[..., 1] ** 2
      s = s + EXT(1) / np.maximum(np.sqrt(rho2 + d[..., 2] ** 2), big)
      if mode:
        s = s + EXT(1) / np.maximum(np.sqrt(rho2 + Rz ** 2), big)
  return s / (EXT(8) * EXT(_PI) * EXT(eta)) * np.abs(dt[:, None] * ds[None, :])


def _sep(src, tgt, dtype):
  src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
  tgt = np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
  wide = np.float64 if np.dtype(dtype) == np.dtype(np.float32) else dtype
  d = (tgt.astype(wide)[:, None, :] - src.astype(wide)[None, :, :]).astype(dtype)
  R = d.copy()
  R[..., 2] = (tgt.astype(wide)[:, None, 2] + src.astype(wide)[None, :, 2]).astype(dtype)
  zt = np.broadcast_to(tgt[:, 2].astype(dtype)[:, None], d.shape[:2])
  h = np.broadcast_to(src[:, 2].astype(dtype)[None, :], d.shape[:2])
  return d, R, zt, h


def _norm(v):
  return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def pressure_rows(wall, src, tgt, dtype=EXT):
  """row[t, s] with p_t = sum_s row[t, s] . f_s: r/(4 pi r^3), and above the wall the Blake images -R/R^3,
  6 h R_z (R_x, R_y, 0)/R^5 and 2 h (1/R^3 - 3 R_z^2/R^5) z.  A coincident pair is 0/0: non-finite, as in the oracle."""
  T = np.dtype(dtype).type
  d, R, zt, h = _sep(src, tgt, dtype)
  with np.errstate(all="ignore"):
    r = _norm(d)
    row = d / (r * r * r)[..., None]
    if wall:
      Rn = _norm(R)
      R3 = Rn * Rn * Rn
      R5 = R3 * Rn * Rn
      row = row - R / R3[..., None]
      xy = R.copy(); xy[..., 2] = 0
      row = row + (T(6) * h * R[..., 2] / R5)[..., None] * xy
      row[..., 2] = row[..., 2] + T(2) * h * (T(1) / R3 - T(3) * R[..., 2] * R[..., 2] / R5)
  return row * (T(1) / (T(4) * T(_PI)))


def pressure_scale(wall, src, tgt):
  d, R, zt, h = _sep(src, tgt, EXT)
  with np.errstate(divide="ignore"):
    s = EXT(1) / _norm(d) ** 2
    if wall:
      s = s + EXT(1) / _norm(R) ** 2
  return s / (EXT(4) * EXT(_PI))


def dl_blocks(variant, src, tgt, normals, weights, a=A_RPY, dtype=EXT):
  """B[t, s] with u_t = sum_s B[t, s] v_s, the factor -3/(4 pi) and the weight included."""
  if variant not in DL_VARIANTS:
    raise ValueError(variant)
  T = np.dtype(dtype).type
  d, R, zt, h = _sep(src, tgt, dtype)
  nt, ns = d.shape[:2]
  n = np.broadcast_to(np.asarray(normals, dtype=np.float64).reshape(-1, 3).astype(dtype)[None, :, :], (nt, ns, 3))
  w = np.broadcast_to(np.asarray(weights, dtype=np.float64).reshape(-1).astype(dtype)[None, :], (nt, ns))
  S = np.array([1, 1, -1], dtype=dtype)
  with np.errstate(all="ignore"):
    r = _norm(d)
    r2 = r * r
    r5 = r2 * r2 * r
    rn = d[..., 0] * n[..., 0] + d[..., 1] * n[..., 1] + d[..., 2] * n[..., 2]
    if variant == "rpy":
      a2 = T(a) * T(a)
      B = _outer((T(1) - T(10) * a2 / (T(3) * r2)) * rn * w / r5, d, d)
      c1 = (T(2) * a2 / T(3)) * w / r5
      B = B + _outer(c1, d, n)          # (n.v) r
      B = B + _outer(c1, n, d)          # (r.v) n
      B = B + _eye(c1 * rn)             # (r.n) v
      B = np.where((r < T(1e-14))[..., None, None], T(0), B)
    else:
      B = np.where((r > T(1e-14))[..., None, None], _outer(rn * w / r5, d, d), T(0))
      if variant == "wall":
        Rn = _norm(R)
        R2 = Rn * Rn
        R3 = R2 * Rn
        R5 = R3 * R2
        RS = R * S                       # (R_x, R_y, -R_z): R.(S v) = RS.v
        nI = n * S
        rnI = R[..., 0] * n[..., 0] + R[..., 1] * n[..., 1] - R[..., 2] * n[..., 2]
        zhat = np.zeros_like(R); zhat[..., 2] = 1
        # the reflected double layer
        B = B - _outer(rnI * w / R5, R, RS)
        # -2 z_t (n.v) (-R_x R_z/R^2, -R_y R_z/R^2, 1/3 - R_z^2/R^2) w/R^3
        g = -R * (R[..., 2] / R2)[..., None]
        g[..., 2] = T(1) / T(3) - R[..., 2] * R[..., 2] / R2
        B = B + _outer(-T(2) * zt * w / R3, g, n)
        # -2 z_t h (R (n.v) + S v (R.nI) + nI (R.Sv) - 5 R (R.Sv)(R.nI)/R^2) w/R^5
        c = -T(2) * zt * h * w / R5
        B = B + _outer(c, R, n)
        B = B + (c * rnI)[..., None, None] * np.diag(S)
        B = B + _outer(c, nI, RS)
        B = B + _outer(-T(5) * c * rnI / R2, R, RS)
        # z: 2 (n.v) R_z w/(3 R^3)  and  2 h (-(n.v)/3 + (R.Sv)(R.nI)/R^2) w/R^3
        B = B + _outer(T(2) * R[..., 2] * w / (T(3) * R3), zhat, n)
        B = B + _outer(-T(2) * h * w / (T(3) * R3), zhat, n)
        B = B + _outer(T(2) * h * rnI * w / (R2 * R3), zhat, RS)
  return B * (-T(3) / (T(4) * T(_PI)))


def dl_scale(variant, src, tgt, normals, weights, a=A_RPY):
  d, R, zt, h = _sep(src, tgt, EXT)
  wn = np.abs(np.asarray(weights, dtype=np.float64).reshape(-1).astype(EXT)) * _norm(np.asarray(normals, dtype=np.float64).reshape(-1, 3).astype(EXT))
  with np.errstate(divide="ignore", invalid="ignore"):
    r = _norm(d)
    if variant == "rpy":
      s = EXT(1) / r ** 2 + EXT(a) ** 2 / r ** 4
    else:
      s = np.where(r > EXT(1e-14), EXT(1) / r ** 2, EXT(0))
      if variant == "wall":
        s = s + EXT(1) / _norm(R) ** 2
  return s * wn[None, :] * (EXT(3) / (EXT(4) * EXT(_PI)))


def worst(got, ref, s, eps):
  """max |got - ref| / (eps s) over the finite entries of ref with s > 0, and where: (ratio, flat index tuple).  s is
  broadcast over the trailing axes of ref."""
  ref = np.asarray(ref)
  s = np.asarray(s, dtype=EXT).reshape(s.shape + (1,) * (ref.ndim - s.ndim))
  with np.errstate(all="ignore"):
    err = np.abs(np.asarray(got, dtype=EXT) - ref) / (EXT(eps) * s)
  err = np.where(np.isfinite(ref) & (np.broadcast_to(s, ref.shape) > 0), err, EXT(0))
  err = np.where(np.isnan(err), EXT(np.inf), err)
  k = int(np.argmax(err))
  return float(err.reshape(-1)[k]), tuple(int(i) for i in np.unravel_index(k, err.shape))


# ---------------------------------------------------------------------------------------------------------------------
# the designed clouds
# ---------------------------------------------------------------------------------------------------------------------
STEP = 6.75                 # x distance of the groups (dyadic; no multiple of it is half a period of either box)
TINY = 4e-12 * A            # "4e-12 a on either side"
ST_BOXES = {"odd": (61.7, 0.0, 0.0), "pow2": (64.0, 128.0, 0.0)}       # periodic in x only / in x and y
N_SOURCES, N_TARGETS = 64, 240                # targets: three full 64-target tiles and one of 48


def st_cloud(periodic=False, offset=0.0):
  """(src, rad_s, tgt, rad_t, L): the designed source -> target configuration.  Targets 0..63 and 64..127 are the two lane
  tiles (one 64-target workgroup each): of the first exactly one target overlaps source 2 and none overlaps source 0, all
  of the second overlap source 3.  Every other designed pair is a source and the targets listed right after it."""
  a = A
  S, T_ = [], []          # (position, radius)
  tiles = []

  def src(g, z, rad, y=0.0):
    S.append(((STEP * g, y, z), rad))
    return np.array([STEP * g, y, z])

  def tgt(p, rad):
    T_.append((tuple(float(c) for c in p), rad))

  # --- group 0: the Zuk switches, a_s = 1/2, in the plane z = 4 (above every radius: the wall mode does not clamp them)
  p = src(0, 4.0, a)
  for ax in (np.array([1.0, 0, 0]), np.array([0, 0, 1.0])):
    for r in (0.75 - TINY, 0.75, 0.75 + TINY, 0.25 - TINY, 0.25, 0.25 + TINY, 0.5, 1e-7 * a):
      tgt(p + r * ax, 0.25)                                  # a_t = 1/4: a_t + a_s = 3/4, |a_t - a_s| = 1/4
  tgt(p + np.array([0.375, 0, 0.5]), 0.125)                  # 3-4-5 / 8: r = 5/8 = a_t + a_s exactly, oblique
  tgt(p + np.array([0.375, 0, -0.5]), 1.125)                 # r = 5/8 = |a_t - a_s| exactly, oblique
  tgt(p, a); tgt(p, 0.25); tgt(p, 2.0)                       # concentric: equal, smaller, larger
  # --- group 1: tracer targets (radius 0) around a source of radius 1/2
  p = src(1, 4.0, a)
  for q in ([2.5, 0, 0], [1.5, 0, 2.0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [0.25, 0, 0], [0, 0, -0.125], [0, 0, 0]):
    tgt(p + np.array(q), 0.0)
  tgt([STEP + 1.0, 0.0, 0.0], 0.0); tgt([STEP + 0.5, 0.25, 0.0], 0.0)       # tracers on the wall, z = 0
  # --- group 2 / 3: the lane tiles
  p2 = src(2, 4.0, a)
  tiles.append([((p2[0], 0.625 + i, 4.0), 0.25) for i in range(64)])        # i = 0 overlaps (5/8 < 3/4), the others do not
  p3 = src(3, 16.0, 8.0)
  tiles.append([((p3[0], -7.875 + 0.25 * i, 16.0), 0.25) for i in range(64)])   # r <= 7.875: all overlap, both regimes
  # --- groups 4..9: heights (wall mode: clamp and damping on one side, the other, both; free surface: images that overlap)
  for g, zs in ((4, 0.3), (5, 1.0), (6, a), (7, a * (1 + 1e-9)), (8, 0.0), (9, 0.0625)):
    p = src(g, zs, a)
    for zt in (0.125, 0.25, 0.25 * (1 + 1e-9), 0.0, 1.0):
      tgt([p[0] + 1.5, 0.0, zt], 0.25)                       # apart
    tgt([p[0] + 0.25, 0.0, 0.125], 0.25)                     # overlapping, both low: z_t + z_s < a_t + a_s
    tgt([p[0] + 0.125, 0.0, 0.0625], 0.25)
    tgt([p[0], 0.0, zs + 3.0], 0.25)                         # stacked
    tgt([p[0], 0.0, zs], 0.25)                               # same point, smaller radius
    tgt([p[0] + 1.5, 0.0, zs], 0.25)                         # in-plane
  if not periodic:            # (in a box the oracle's fp64 wrap of a separation of 1000 a would set the yardstick)
    tgt([STEP * 5 + 1000 * a, 0.0, 1.0], 0.25)               # 1000 a along the wall, both low: wall and free parts nearly cancel
    tgt([STEP * 5 + 1000 * a, 3.0, 0.25], 0.0)
  tgt([STEP * 5, 0.0, 1000 * a], 0.25)                       # 1000 a above
  # --- radius ratios 1e-3 and 1e3, on their own 8192 a away: the middle regime divides by a_t a_s and loses a_> / a_< of its
  # digits, so these pairs stand at contact (exact operands), inside, and apart -- never strictly between the two switches
  far_y = -24.0 if periodic else -4096.0
  p = np.array([0.0, far_y, 4.0])
  S.append((tuple(p), a))
  tgt(p + np.array([a + a / 1024, 0, 0]), a / 1024)          # ratio 1e-3 at contact, inside, apart
  tgt(p + np.array([0.125, 0, 0]), a / 1024)
  tgt(p + np.array([0, 0, 1.0]), a / 1024)
  p = np.array([STEP, far_y, 4.0])
  S.append((tuple(p), a / 1024))                             # ratio 1e3 from a small source: at contact, around it, apart
  tgt(p + np.array([a + a / 1024, 0, 0]), a)
  tgt(p + np.array([0.125, 0, 0]), a)
  tgt(p + np.array([0, 0, 1.0]), a)
  if not periodic:           # a blob of 1024 a (larger than either box): at contact (clamped and damped by the wall mode), around the source
    p = np.array([0.0, far_y, 4.0])
    tgt(p + np.array([a + 1024 * a, 0, 0]), 1024 * a)
    tgt(p + np.array([3.0, 0, 0]), 1024 * a)
  L = None
  if periodic:
    L = np.array(ST_BOXES[periodic])
    tgt([L[0] * (0.5 - 3e-7), 0.0, 4.0], 0.25)               # 3e-7 of a period from the half period of source 0
    tgt([STEP * 5 + L[0] * (1.5 + 3e-7), 0.0, 1.0], 0.25)
    tgt([STEP + L[0] - 0.5, 0.0, 4.0], 0.25)                 # across the cell edge, in contact with source 1
  # --- seeded fill
  rng = np.random.RandomState(4321)
  while len(S) < N_SOURCES:
    g = rng.randint(10)
    S.append(((STEP * g + 3 * rng.rand() - 1.5, 4 * rng.rand() + 2.0, 0.1 + 3 * rng.rand()), float(2.0 ** -rng.randint(0, 4))))
  n_designed = len(T_)
  while 128 + len(T_) < N_TARGETS:
    g = rng.randint(10)
    T_.append(((STEP * g + 3 * rng.rand() - 1.5, 4 * rng.rand() + 2.0, 0.1 + 3 * rng.rand()), float(2.0 ** -rng.randint(1, 5)) * rng.randint(0, 2)))
  assert len(S) == N_SOURCES and 128 + len(T_) == N_TARGETS and n_designed <= N_TARGETS - 128, (len(S), len(T_), n_designed)
  T_ = tiles[0] + tiles[1] + T_
  src_p, rad_s = np.array([s[0] for s in S]), np.array([s[1] for s in S])
  tgt_p, rad_t = np.array([t[0] for t in T_]), np.array([t[1] for t in T_])
  src_p[:, :2] += offset
  tgt_p[:, :2] += offset
  return src_p, rad_s, tgt_p, rad_t, L


def st_same_cloud(periodic=False):
  """(r, rad, L) with N = 200 for sources == targets: the sources of st_cloud and its designed targets as ONE set of blobs
  (tracers get the radius a/8: the symmetric kernels divide by a_t a_s), listed in a seeded random order."""
  src_p, rad_s, tgt_p, rad_t, L = st_cloud(periodic)
  r = np.concatenate([src_p, tgt_p[128:], tgt_p[:64]])[:200]
  rad = np.concatenate([rad_s, rad_t[128:], rad_t[:64]])[:200]
  rad = np.where(rad > 0, rad, A / 8)
  perm = np.random.RandomState(77).permutation(200)
  return r[perm], rad[perm], L


def st_ties(src, tgt, L, tol=1e-9):
  L = _period(L)
  bad = 0
  for k in range(3):
    if L[k] > 0:
      q = (np.asarray(tgt)[:, None, k].astype(EXT) - np.asarray(src)[None, :, k].astype(EXT)) / EXT(L[k])
      bad += int((np.abs(q - np.floor(q) - EXT(0.5)) < tol).sum())
  return bad


def st_coverage(mode, src, rad_s, tgt, rad_t, L=None):
  """Counts of the (target, source) pairs (nearest image, effective heights of `mode`) and of the blobs per regime class."""
  xs, xt, rs, rt, L, ds, dt, wide, d, Rz = _st_setup(mode, src, tgt, rad_s, rad_t, L, EXT)
  raw = xt.astype(EXT)[:, None, :] - xs.astype(EXT)[None, :, :]
  at, as_ = rt.astype(EXT)[:, None], rs.astype(EXT)[None, :]
  rho2 = d[..., 0] ** 2 + d[..., 1] ** 2
  r2 = rho2 + d[..., 2] ** 2
  r = np.sqrt(r2)
  R = np.sqrt(rho2 + Rz ** 2)
  sm, df = at + as_, np.abs(at - as_)
  blob = (at > 0) & (as_ > 0)
  big = np.maximum(at, as_)
  zs, zt = np.asarray(src, dtype=np.float64).reshape(-1, 3)[:, 2], np.asarray(tgt, dtype=np.float64).reshape(-1, 3)[:, 2]
  near = lambda x, y: (np.abs(x - y) <= 1e-11 * A) & (x != y)       # noqa: E731
  ov = r <= sm
  tile = [ov[k * 64:(k + 1) * 64].sum(axis=0) for k in range(2)]
  with np.errstate(divide="ignore", invalid="ignore"):
    ratio = np.where(as_ > 0, at / as_, 0)
  c = {
      "sum_exact": int(((r2 == sm * sm) & blob).sum()), "sum_below": int((near(r, sm) & (r < sm) & blob).sum()),
      "sum_above": int((near(r, sm) & (r > sm) & blob).sum()),
      "diff_exact": int(((r2 == df * df) & blob & (df > 0)).sum()), "diff_below": int((near(r, df) & (r < df) & blob).sum()),
      "diff_above": int((near(r, df) & (r > df) & blob).sum()),
      "sum_exact_oblique": int(((r2 == sm * sm) & blob & (rho2 > 0) & (d[..., 2] != 0)).sum()),
      "diff_exact_oblique": int(((r2 == df * df) & blob & (df > 0) & (rho2 > 0) & (d[..., 2] != 0)).sum()),
      "concentric_equal": int(((r2 == 0) & (at == as_) & blob).sum()), "concentric_unequal": int(((r2 == 0) & (at != as_) & blob).sum()),
      "deep_inside": int(((r2 > 0) & (r <= 1e-6 * big) & blob).sum()),
      "regime_far": int((r > sm).sum()), "regime_mid": int(((r <= sm) & (r > df)).sum()), "regime_in": int((r <= df).sum()),
      "ratio_small": int(((ratio > 0) & (ratio <= 1e-3) & ov).sum()), "ratio_large": int(((ratio >= 1e3) & ov).sum()),
      "tracer_outside": int(((at == 0) & (r > as_)).sum()), "tracer_on_surface": int(((at == 0) & (r2 == as_ * as_) & (as_ > 0)).sum()),
      "tracer_inside": int(((at == 0) & (r < as_)).sum()), "tracer_z0": int(((rt == 0) & (zt == 0)).sum()),
      "tile_one_lane": int((tile[0] == 1).sum()) if tile[0][2 % len(tile[0])] == 1 else 0,
      "tile_no_lane": int((tile[0] == 0).sum()) if tile[0][0] == 0 else 0,
      "tile_all_lanes": int((tile[1] == 64).sum()) if tile[1][3 % len(tile[1])] == 64 else 0,
      "stacked": int(((rho2 == 0) & (r2 > 0)).sum()), "inplane": int(((d[..., 2] == 0) & (r2 > 0)).sum()),
      "far_low": int(((np.sqrt(rho2) >= 900 * A) & (zt[:, None] <= 1.0) & (zs[None, :] <= 1.0)).sum()),
      "far_above": int(((rho2 == 0) & (r >= 900 * A)).sum()),
      "src_below_only": int(((zs < rs)[None, :] & (zs > 0)[None, :] & (zt >= rt)[:, None] & blob).sum()),
      "tgt_below_only": int(((zs >= rs)[None, :] & (zt < rt)[:, None] & (zt > 0)[:, None] & blob).sum()),
      "both_below": int(((zs < rs)[None, :] & (zs > 0)[None, :] & (zt < rt)[:, None] & (zt > 0)[:, None]).sum()),
      "z_exact": int((zs == rs).sum()) * int(((zt == rt) & (rt > 0)).sum()),
      "z_just_above": int(((zs > rs) & (zs <= rs * (1 + 2e-9))).sum()) * int(((zt > rt) & (zt <= rt * (1 + 2e-9))).sum()),
      "z0_source": int(((zs == 0) & (rs > 0)).sum()), "z0_target": int(((zt == 0) & (rt > 0)).sum()),
      "image_mid": int(((R <= sm) & (R > df) & blob).sum()), "image_in": int(((R <= df) & blob).sum()),
      "image_is_pair": int(((Rz == d[..., 2]) & (r2 > 0)).sum()),
      "offset": int((np.abs(xt[:, :2]).min() >= 5e5 * A) and (np.abs(xs[:, :2]).min() >= 5e5 * A)),
      "cross_edge": 0, "beyond_period": 0, "half_period": 0, "ties": st_ties(src, tgt, L),
  }
  for k in range(3):
    if L[k] > 0:
      Lk = EXT(L[k])
      t = raw[..., k] / Lk
      frac = np.abs(t - np.floor(t) - EXT(0.5))
      c["cross_edge"] += int(((d[..., k] != raw[..., k]) & (np.abs(raw[..., k]) < Lk)).sum())
      c["beyond_period"] += int((np.abs(raw[..., k]) > Lk).sum())
      c["half_period"] += int(((frac >= 1e-9) & (frac < 1e-6)).sum())
  return c


_ZUK = ("sum_exact", "sum_below", "sum_above", "diff_exact", "diff_below", "diff_above", "sum_exact_oblique", "diff_exact_oblique",
        "concentric_equal", "concentric_unequal", "deep_inside", "regime_far", "regime_mid", "regime_in", "ratio_small", "ratio_large",
        "tracer_outside", "tracer_on_surface", "tracer_inside", "tracer_z0", "tile_one_lane", "tile_no_lane", "tile_all_lanes",
        "stacked", "inplane", "far_low", "far_above")
_HEIGHTS = ("src_below_only", "tgt_below_only", "both_below", "z_exact", "z_just_above", "z0_source", "z0_target")
ST_CLASSES = {0: _ZUK, 1: _ZUK + _HEIGHTS, 2: _ZUK + ("image_mid", "image_in", "image_is_pair", "z0_source", "z0_target")}
# next to 1e6 a one unit in the last place is 1e-10 a: the separations 4e-12 a and 1e-7 a from a switch do not exist there
_NOT_AT_OFFSET = ("sum_below", "sum_above", "diff_below", "diff_above", "deep_inside")
ST_PERIODIC = ("cross_edge", "beyond_period", "half_period")
ST_CLOUDS = {"open": (False, 0.0), "offset": (False, 1.0e6 * A), "odd": ("odd", 0.0), "pow2": ("pow2", 0.0)}


def st_classes(mode, name):
  periodic, offset = ST_CLOUDS[name]
  cl = ST_CLASSES[mode]
  if offset:
    cl = tuple(k for k in cl if k not in _NOT_AT_OFFSET) + ("offset",)
  if periodic:
    cl = tuple(k for k in cl if k != "far_low") + ST_PERIODIC
  return cl


def assert_st_coverage(mode, name, cloud):
  c = st_coverage(mode, *cloud)
  missing = [k for k in st_classes(mode, name) if c[k] < 1]
  assert not missing, (mode, name, missing, c)
  assert c["ties"] == 0, c
  return c


def aux_cloud(offset=0.0):
  """(src, normals, weights, tgt) of the pressure and double-layer tests: at most 64 sources, 200 targets."""
  S, N, W, T_ = [], [], [], []

  def src(p, n, w=0.75):
    S.append(p); N.append(n); W.append(w)
    return np.array(p, dtype=np.float64)

  p = src([0.0, 0.0, 1.0], [0.0, 0.0, 1.0])
  T_ += [p + [0.5e-14, 0, 0], p + [2e-14, 0, 0], p + [0, 2e-14, 0], p + [0, 0.5e-14, 0]]        # either side of the 1e-14 skip
  p = src([4.0, 0.0, 1.0], [0.0, 0.0, 1.0])
  T_ += [p + [1.0, 0, 0], p + [0, 2.0, 0]]                                                       # n perpendicular to r, exactly
  p = src([8.0, 0.0, 2.0 ** -30], [0.6, 0.0, 0.8])
  T_ += [p + [1.0, 0, 0], [9.0, 0.5, 0.0], [8.0, 0.0, 0.0], [8.0, 1.0, 0.0], [8.0, 0.0, 2.0]]    # z_s -> 0, z_t = 0
  p = src([12.0, 0.0, 1.0], [0.0, 0.8, -0.6], 1.25)
  T_ += [p + [0, 0, 2.0], p + [0, 0, -0.5], p + [1.0, 0, 0], p + [1000.0, 0, 0], p + [0, 0, 1000.0]]   # stacked, in-plane, far
  p = src([16.0, 0.0, 2.0], [1.0, 0.0, 0.0], 0.5)
  # RPY: a sqrt(10/3) = 0.45644 for a = 1/4: either side, and r << a
  T_ += [p + [0.4375, 0, 0], p + [0.5, 0, 0], p + [0, 0, 0.4375], p + [0.28125, 0, 0.375], p + [2.0 ** -20, 0, 0], p + [0, 0, 2.0 ** -12]]
  rng = np.random.RandomState(2024)
  while len(S) < 40:
    n = rng.randn(3)
    src(list(rng.rand(3) * [20.0, 6.0, 3.0] + [0.0, 1.0, 0.05]), list(n / np.linalg.norm(n)), 0.05 + rng.rand())
  T_ += [np.array(s) for s in S]                                                                 # targets equal to sources
  while len(T_) < 200:
    T_.append(rng.rand(3) * [20.0, 6.0, 3.0] + [0.0, 1.0, 0.0])
  src_p, tgt_p = np.array(S, dtype=np.float64), np.array([np.asarray(t, dtype=np.float64) for t in T_])
  src_p[:, :2] += offset
  tgt_p[:, :2] += offset
  return src_p, np.array(N, dtype=np.float64), np.array(W, dtype=np.float64), tgt_p


def aux_coverage(src, normals, weights, tgt, a=A_RPY):
  d, R, zt, h = _sep(src, tgt, EXT)
  r = _norm(d)
  n = np.asarray(normals, dtype=np.float64).astype(EXT)
  rn = (d * n[None, :, :]).sum(axis=2)
  edge = EXT(a) * np.sqrt(EXT(10) / EXT(3))
  rho = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
  return {
      "below_skip": int(((r > 0) & (r < 1e-14)).sum()), "above_skip": int(((r > 1e-14) & (r < 1e-13)).sum()),
      "coincident": int((r == 0).sum()), "zs_small": int((np.asarray(src)[:, 2] <= 1e-8).sum()), "zt_zero": int((np.asarray(tgt)[:, 2] == 0).sum()),
      "stacked": int(((rho == 0) & (r > 0.1)).sum()), "inplane": int(((d[..., 2] == 0) & (r > 0.1)).sum()),
      "far": int((r >= 1000).sum()), "n_perp_r": int(((rn == 0) & (r > 0.1)).sum()),
      "rpy_inside_edge": int(((r < edge) & (r > 0.9 * edge)).sum()), "rpy_outside_edge": int(((r > edge) & (r < 1.2 * edge)).sum()),
      "rpy_deep": int(((r > 1e-14) & (r < 1e-3 * a)).sum()),
      "offset": int(np.abs(np.asarray(src)[:, :2]).min() >= 5e5 and np.abs(np.asarray(tgt)[:, :2]).min() >= 5e5),
  }


AUX_CLASSES = ("below_skip", "above_skip", "coincident", "zs_small", "zt_zero", "stacked", "inplane", "far", "n_perp_r",
               "rpy_inside_edge", "rpy_outside_edge", "rpy_deep")
# next to 1e6 the separations of 1e-14 and 2^-20 collapse onto the source: they count as coincident there
AUX_OFFSET_CLASSES = tuple(k for k in AUX_CLASSES if k not in ("below_skip", "above_skip", "rpy_deep")) + ("offset",)
AUX_CLOUDS = {"open": (0.0, AUX_CLASSES), "offset": (1.0e6, AUX_OFFSET_CLASSES)}


def assert_aux_coverage(name, cloud):
  c = aux_coverage(*cloud)
  missing = [k for k in AUX_CLOUDS[name][1] if c[k] < 1]
  assert not missing, (name, missing, c)
  return c


# ---------------------------------------------------------------------------------------------------------------------
# clouds and references, once per process
# ---------------------------------------------------------------------------------------------------------------------
_cache = {}


def cloud(name):
  """(src, rad_s, tgt, rad_t, L) of ST_CLOUDS[name], coverage of every mode asserted."""
  if ("st", name) not in _cache:
    c = st_cloud(*ST_CLOUDS[name])
    for mode in MODES:
      assert_st_coverage(mode, name, c)
    _cache["st", name] = c
  return _cache["st", name]


def same_cloud(name):
  """(r, rad, L), N = 200, sources == targets; name "open" / "odd" / "pow2"."""
  if ("same", name) not in _cache:
    r, rad, L = st_same_cloud(ST_CLOUDS[name][0])
    assert st_ties(r, r, L) == 0
    for mode in (0, 1):
      c = st_coverage(mode, r, rad, r, rad, L)
      need = ("sum_exact", "diff_exact", "concentric_unequal", "regime_far", "regime_mid", "regime_in", "stacked", "inplane") + \
          (("src_below_only", "tgt_below_only", "both_below", "z_exact", "z0_source") if mode else ())
      assert all(c[k] >= 1 for k in need), (name, mode, c)
    _cache["same", name] = (r, rad, L)
  return _cache["same", name]


def aux(name):
  if ("aux", name) not in _cache:
    c = aux_cloud(AUX_CLOUDS[name][0])
    assert_aux_coverage(name, c)
    _cache["aux", name] = c
  return _cache["aux", name]


def st_reference(name, mode):
  """(EXT blocks, scale) of cloud `name`."""
  key = ("st_ref", name, mode)
  if key not in _cache:
    src, rs, tgt, rt, L = cloud(name)
    _cache[key] = (st_blocks(mode, src, tgt, rs, rt, ETA, L), st_scale(mode, src, tgt, rs, rt, ETA, L))
  return _cache[key]


def same_reference(name, mode):
  key = ("same_ref", name, mode)
  if key not in _cache:
    r, rad, L = same_cloud(name)
    _cache[key] = (st_blocks(mode, r, r, rad, rad, ETA, L), st_scale(mode, r, r, rad, rad, ETA, L))
  return _cache[key]


def pressure_reference(name, wall):
  key = ("p_ref", name, wall)
  if key not in _cache:
    src, nrm, w, tgt = aux(name)
    _cache[key] = (pressure_rows(wall, src, tgt), pressure_scale(wall, src, tgt))
  return _cache[key]


def dl_reference(name, variant):
  key = ("dl_ref", name, variant)
  if key not in _cache:
    src, nrm, w, tgt = aux(name)
    _cache[key] = (dl_blocks(variant, src, tgt, nrm, w), dl_scale(variant, src, tgt, nrm, w))
  return _cache[key]


def edge_problem(ns, nt):
  """Seeded inputs of a whole product at an edge shape: blobs of mixed radii in a box dense enough for every regime, some
  below their radius, a few tracer targets; normals, weights and the vectors of the aux operators."""
  key = ("edge", ns, nt)
  if key not in _cache:
    rng = np.random.RandomState(1000 * ns + nt)
    box = max(2.0, (max(ns, nt) ** (1.0 / 3.0)) * 0.8)
    src = rng.rand(ns, 3) * box + [0.0, 0.0, 0.05]
    tgt = rng.rand(nt, 3) * box + [0.0, 0.0, 0.05]
    rs = 2.0 ** -rng.randint(0, 5, size=ns).astype(np.float64)
    rt = 2.0 ** -rng.randint(0, 5, size=nt).astype(np.float64) * (rng.rand(nt) > 0.15)
    nrm = rng.randn(ns, 3)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    _cache[key] = dict(src=src, tgt=tgt, rs=rs, rt=rt, f=rng.randn(ns, 3), nrm=nrm, v=rng.randn(ns, 3), w=0.05 + rng.rand(ns))
  return _cache[key]


def edge_reference(op, ns, nt):
  """(EXT product (nt, 3) or (nt,), per-target scale sum_s s_ts |f_s|_max) of operator `op`: ("st", mode), ("p", wall),
  ("dl", variant), with the vectors of edge_problem."""
  key = ("edge_ref", op, ns, nt)
  if key not in _cache:
    e = edge_problem(ns, nt)
    if op[0] == "st":
      B, s = st_blocks(op[1], e["src"], e["tgt"], e["rs"], e["rt"], ETA), st_scale(op[1], e["src"], e["tgt"], e["rs"], e["rt"], ETA)
      vec = e["f"]
      u = np.einsum("tspq,sq->tp", B, vec.astype(EXT))
    elif op[0] == "p":
      B, s = pressure_rows(op[1], e["src"], e["tgt"]), pressure_scale(op[1], e["src"], e["tgt"])
      vec = e["f"]
      u = np.einsum("tsq,sq->t", B, vec.astype(EXT))
    else:
      B, s = dl_blocks(op[1], e["src"], e["tgt"], e["nrm"], e["w"]), dl_scale(op[1], e["src"], e["tgt"], e["nrm"], e["w"])
      vec = e["v"]
      u = np.einsum("tspq,sq->tp", B, vec.astype(EXT))
    _cache[key] = (u, (s * np.abs(vec).max(axis=1).astype(EXT)[None, :]).sum(axis=1), B, s)
  return _cache[key][:2]


def edge_blocks(op, ns, nt):
  """(EXT blocks -- (nt, ns, 3) rows for the pressure --, scale) behind edge_reference."""
  edge_reference(op, ns, nt)
  return _cache["edge_ref", op, ns, nt][2:]


def tracer_problem():
  """Tracers (radius 0) ON the no-slip wall, z_t = 0, under blobs of mixed radii, some of them below their radius."""
  rng = np.random.RandomState(31)
  src = rng.rand(48, 3) * [6.0, 6.0, 2.0] + [0.0, 0.0, 0.05]
  rs = 2.0 ** -rng.randint(0, 4, size=48).astype(np.float64)
  tgt = np.concatenate([rng.rand(64, 3) * [6.0, 6.0, 0.0], src * [1.0, 1.0, 0.0]])       # also right under every source
  return src, rs, tgt, np.zeros(len(tgt)), rng.randn(48, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 oracle in block form: one source at a time (every call is a product with a single source)
# ---------------------------------------------------------------------------------------------------------------------
_ST_ORACLE = {0: "no_wall_mobility_trans_times_force_source_target_oracle", 1: "single_wall_mobility_trans_times_force_source_target_oracle",
              2: "free_surface_mobility_trans_times_force_source_target_oracle"}


def oracle_st_product(oracle, mode, src, tgt, force, rad_s, rad_t, eta, L=None):
  kw = {} if L is None else {"periodic_length": np.asarray(L, dtype=np.float64)}
  return getattr(oracle, _ST_ORACLE[mode])(src, tgt, force, rad_s, rad_t, eta, **kw).reshape(-1, 3)


def oracle_st_blocks(oracle, mode, src, tgt, rad_s, rad_t, eta, L=None):
  ns, nt = len(src), len(tgt)
  out = np.empty((nt, ns, 3, 3))
  for j in range(ns):
    for q in range(3):
      e = np.zeros((1, 3)); e[0, q] = 1.0
      out[:, j, :, q] = oracle_st_product(oracle, mode, src[j:j + 1], tgt, e, rad_s[j:j + 1], rad_t, eta, L)
  return out


def oracle_pressure_product(oracle, wall, src, tgt, force):
  fn = oracle.single_wall_pressure_Stokeslet_oracle if wall else oracle.no_wall_pressure_Stokeslet_oracle
  return fn(src, tgt, force)


def oracle_pressure_rows(oracle, wall, src, tgt):
  out = np.empty((len(tgt), len(src), 3))
  with np.errstate(all="ignore"):
    for j in range(len(src)):
      for q in range(3):
        e = np.zeros((1, 3)); e[0, q] = 1.0
        out[:, j, q] = oracle_pressure_product(oracle, wall, src[j:j + 1], tgt, e)
  return out


def oracle_dl_product(oracle, variant, src, tgt, normals, vector, weights, a=A_RPY):
  if variant == "rpy":
    return oracle.no_wall_double_layer_source_target_oracle(src, tgt, normals, vector, weights, a).reshape(-1, 3)
  return oracle.double_layer_source_target_oracle(src, tgt, normals, vector, weights, wall=1 if variant == "wall" else 0).reshape(-1, 3)


def oracle_dl_blocks(oracle, variant, src, tgt, normals, weights, a=A_RPY):
  out = np.empty((len(tgt), len(src), 3, 3))
  for j in range(len(src)):
    for q in range(3):
      e = np.zeros((1, 3)); e[0, q] = 1.0
      out[:, j, :, q] = oracle_dl_product(oracle, variant, src[j:j + 1], tgt, normals[j:j + 1], e, weights[j:j + 1], a)
  return out
