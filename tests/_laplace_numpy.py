"""numpy restatement of the six Laplace layer operators (Laplace_kernels_numba.py), written from the formulas:
1/(4 pi) sum_j w_j f_j K(r_i - r_j), wall images (x_j, y_j, -z_j) with normals (n_x, n_y, -n_z).  The self operators skip
the free-space term of j == i by index and keep its image; the source -> target ones skip |r| < 1e-12.  Vectorised over
the sources, looped over target blocks: fine for a few hundred targets against tens of thousands of sources.

`apply(..., ext=True)` evaluates and accumulates every term in np.longdouble (EXT; float64 where the platform's long
double has no 64-bit mantissa -- EXT_NAME says which), and `with_scale=True` returns next to each value the
condition-aware scale  A_i = 1/(4 pi) sum_j |w_j f_j| |K|_ij  (free and image terms counted separately; |K| = 1/r for
S, |n|/r^2 for D, 4|n|/r^3 for G, 1/r^2 for P: a bound of every term, whatever the cancellation).  `dense` builds the
(N, N) / (N, 3, N) matrices of the same operators; `dense_slip` solves the concentration problem of the phoretic slip
 with them."""
import numpy as np

LONG_DOUBLE = np.finfo(np.longdouble).nmant >= 63
EXT = np.longdouble if LONG_DOUBLE else np.float64
EXT_NAME = "longdouble" if LONG_DOUBLE else "float64-fallback"
_F = 1.0 / (4.0 * np.pi)
_F_EXT = EXT(1) / (16 * np.arctan(EXT(1)))
_FLIP = np.array([1.0, 1.0, -1.0])


def _image(src, normals=None):
  s = src * _FLIP
  return s, (None if normals is None else normals * _FLIP)


def _kernel(kind, d, n):
  """K for the displacement block d (t, s, 3) and source normals n (s, 3) -> (t, s) or (t, s, 3)."""
  with np.errstate(divide="ignore", invalid="ignore"):
    return _kernel_values(kind, d, n)


def _kernel_values(kind, d, n):
  r2 = np.einsum("tsk,tsk->ts", d, d)
  ir = 1 / np.sqrt(r2)
  ir3 = ir ** 3
  if kind == "S":
    return ir
  if kind == "P":
    return d * ir3[..., None]
  rn = np.einsum("tsk,sk->ts", d, n)
  if kind == "D":
    return rn * ir3
  # G: (n - 3 r (r.n)/r^2) / r^3
  return (n[None, :, :] - 3 * d * (rn * ir ** 2)[..., None]) * ir3[..., None]


def _kernel_bound(kind, d, n):
  """|K| of the scale: 1/r (S), |n|/r^2 (D), 4|n|/r^3 (G), 1/r^2 (P); (t, s)."""
  with np.errstate(divide="ignore"):
    r2 = np.einsum("tsk,tsk->ts", d, d).astype(np.float64)
    if kind == "S":
      return 1.0 / np.sqrt(r2)
    if kind == "P":
      return 1.0 / r2
    nn = np.sqrt(np.einsum("sk,sk->s", n, n).astype(np.float64))[None, :]
    return nn / r2 if kind == "D" else 4.0 * nn / (r2 * np.sqrt(r2))


def _self_mask(idx, b0, block, n_src):
  return idx[b0:b0 + block, None] == np.arange(n_src)[None, :]


def apply(kind, src, field, weights, normals=None, wall=0, tgt=None, targets_idx=None, block=64, ext=False,
          with_scale=False):
  """kind in S, D, G, P.  tgt None = self operator (targets = sources, optionally only the rows targets_idx);
  otherwise source -> target.  Returns (nt,) or (nt, 3) (EXT with ext=True), and with with_scale=True also the (nt,)
  float64 scale A."""
  dt = EXT if ext else np.float64
  F = _F_EXT if ext else _F
  src = np.asarray(src, dtype=np.float64).reshape(-1, 3).astype(dt)
  fw = (np.asarray(field, dtype=np.float64).reshape(-1).astype(dt) * np.asarray(weights, dtype=np.float64).reshape(-1))
  afw = np.abs(fw).astype(np.float64)
  nrm = None if normals is None else np.asarray(normals, dtype=np.float64).reshape(-1, 3).astype(dt)
  self_op = tgt is None
  if self_op:
    idx = np.arange(len(src)) if targets_idx is None else np.asarray(targets_idx)
    t = src[idx]
  else:
    t = np.asarray(tgt, dtype=np.float64).reshape(-1, 3).astype(dt)
    idx = None
  vec = kind in ("G", "P")
  out = np.zeros((len(t), 3) if vec else len(t), dtype=dt)
  scale = np.zeros(len(t))
  if wall:
    si, ni = _image(src, nrm)
  for b0 in range(0, len(t), block):
    tb = t[b0:b0 + block]
    d = tb[:, None, :] - src[None, :, :]
    K = _kernel(kind, d, nrm)
    if self_op:
      mask = _self_mask(idx, b0, block, len(src))
    else:
      mask = np.einsum("tsk,tsk->ts", d, d) < 1e-24
    K = np.where(mask[..., None] if vec else mask, 0, K)
    if with_scale:
      scale[b0:b0 + block] = np.where(mask, 0.0, _kernel_bound(kind, d, nrm)) @ afw
    if wall:
      dI = tb[:, None, :] - si[None, :, :]
      K = K + _kernel(kind, dI, ni)
      if with_scale:
        scale[b0:b0 + block] += _kernel_bound(kind, dI, ni) @ afw
    out[b0:b0 + block] = np.einsum("ts...,s->t...", K, fw)
  out = F * out
  return (out, _F * scale) if with_scale else out


def apply_ext(kind, src, field, weights, normals=None, wall=0, tgt=None, targets_idx=None):
  """apply(..., ext=True, with_scale=True): (EXT values, float64 scale)."""
  return apply(kind, src, field, weights, normals, wall=wall, tgt=tgt, targets_idx=targets_idx, ext=True, with_scale=True)


def dense(kind, r, weights, normals=None, wall=0):
  """Matrix M of the self operator: apply(kind, r, f, weights, normals, wall) == M @ f (float64).  (N, N) for S and D,
  (N, 3, N) for G and P.  Same index skip (j == i) and image rule (kept for j == i) as apply."""
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  w = np.asarray(weights, dtype=np.float64).reshape(-1)
  nrm = None if normals is None else np.asarray(normals, dtype=np.float64).reshape(-1, 3)
  n = len(r)
  vec = kind in ("G", "P")
  K = _kernel(kind, r[:, None, :] - r[None, :, :], nrm)
  eye = np.eye(n, dtype=bool)
  K = np.where(eye[..., None] if vec else eye, 0.0, K)
  if wall:
    si, ni = _image(r, nrm)
    K = K + _kernel(kind, r[:, None, :] - si[None, :, :], ni)
  K = _F * K * (w[None, :, None] if vec else w[None, :])
  return np.ascontiguousarray(np.moveaxis(K, 1, 2)) if vec else K


def rotation_matrix(q):
  """Rotation of the unit quaternion q = (s, p): R = (s^2 - p.p) I + 2 p p^T + 2 s [p]x."""
  s, p = float(q[0]), np.asarray(q[1:4], dtype=np.float64)
  px = np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])
  return (s * s - p @ p) * np.eye(3) + 2.0 * np.outer(p, p) + 2.0 * s * px


def bodies_to_lab(vertices, normals_body, locations, quaternions):
  """Per body b: nodes location_b + R_b vertex and normals R_b n; vertices / normals_body: one (n_b, 3) array per body.
  -> (N, 3) positions, (N, 3) normals in blob order."""
  rs, ns = [], []
  for v, nb, x, q in zip(vertices, normals_body, locations, quaternions):
    R = rotation_matrix(q)
    rs.append(np.asarray(x, dtype=np.float64)[None, :] + np.asarray(v, dtype=np.float64) @ R.T)
    ns.append(np.asarray(nb, dtype=np.float64) @ R.T)
  return np.concatenate(rs), np.concatenate(ns)


def hessian(background):
  """Symmetric, traceless H from background[4:9] = (H_xx, H_xy, H_xz, H_yy, H_yz); H_zz = -H_xx - H_yy."""
  bg = np.zeros(9)
  bg[:len(np.ravel(background))] = np.ravel(background)
  xx, xy, xz, yy, yz = bg[4:9]
  return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, -xx - yy]])


def dense_slip(r, normals, weights, k, e, mu, background, Dc, wall):
  """Dense restatement of the phoretic slip: with c_bg(r) = c0 + b.r + r.H r,
      (1/2 I - D + S diag(k / Dc)) c = c_bg + S[e / Dc]                        (np.linalg.solve)
      g = 4 H r + 2 b + 2 G[c] - 2 P[(e - k c) / Dc],   slip = mu (g - n (n.g))
  r, normals (N, 3) lab frame; k, e, mu, weights (N,); background = background_Laplace (c0, b, H as in hessian).
  -> (c (N,), slip (N, 3))."""
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
  n = len(r)
  bg = np.zeros(9)
  bg[:len(np.ravel(background))] = np.ravel(background)
  c0, b = bg[0], bg[1:4]
  H = hessian(bg)
  S = dense("S", r, weights, wall=wall)
  D = dense("D", r, weights, nrm, wall=wall)
  G = dense("G", r, weights, nrm, wall=wall)
  P = dense("P", r, weights, wall=wall)
  k, e = np.asarray(k, dtype=np.float64) / Dc, np.asarray(e, dtype=np.float64) / Dc
  Hr = r @ H.T
  A = 0.5 * np.eye(n) - D + S * k[None, :]
  c = np.linalg.solve(A, c0 + r @ b + np.einsum("ik,ik->i", r, Hr) + S @ e)
  g = 4.0 * Hr + 2.0 * b[None, :] + 2.0 * np.einsum("ikj,j->ik", G, c) - 2.0 * np.einsum("ikj,j->ik", P, e - k * c)
  slip = np.asarray(mu, dtype=np.float64).reshape(-1, 1) * (g - nrm * np.einsum("ik,ik->i", nrm, g)[:, None])
  return c, slip
