"""float64 numpy restatement of the six Laplace layer operators (Laplace_kernels_numba.py), written from the formulas:
1/(4 pi) sum_j w_j f_j K(r_i - r_j), wall images (x_j, y_j, -z_j) with normals (n_x, n_y, -n_z).  The self operators skip
the free-space term of j == i by index and keep its image; the source -> target ones skip |r| < 1e-12.  Vectorised over
the sources, looped over target blocks: fine for a few hundred targets against tens of thousands of sources."""
import numpy as np

_F = 1.0 / (4.0 * np.pi)


def _image(src, normals=None):
  s = src * np.array([1.0, 1.0, -1.0])
  return s, (None if normals is None else normals * np.array([1.0, 1.0, -1.0]))


def _kernel(kind, d, n):
  """K for the displacement block d (t, s, 3) and source normals n (s, 3) -> (t, s) or (t, s, 3)."""
  with np.errstate(divide="ignore", invalid="ignore"):
    return _kernel_values(kind, d, n)


def _kernel_values(kind, d, n):
  r2 = np.einsum("tsk,tsk->ts", d, d)
  ir = 1.0 / np.sqrt(r2)
  ir3 = ir ** 3
  if kind == "S":
    return ir
  if kind == "P":
    return d * ir3[..., None]
  rn = np.einsum("tsk,sk->ts", d, n)
  if kind == "D":
    return rn * ir3
  # G: (n - 3 r (r.n)/r^2) / r^3
  return (n[None, :, :] - 3.0 * d * (rn * ir ** 2)[..., None]) * ir3[..., None]


def apply(kind, src, field, weights, normals=None, wall=0, tgt=None, targets_idx=None, block=64):
  """kind in S, D, G, P.  tgt None = self operator (targets = sources, optionally only the rows targets_idx);
  otherwise source -> target.  Returns (nt,) or (nt, 3)."""
  src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
  fw = np.asarray(field, dtype=np.float64).reshape(-1) * np.asarray(weights, dtype=np.float64).reshape(-1)
  nrm = None if normals is None else np.asarray(normals, dtype=np.float64).reshape(-1, 3)
  self_op = tgt is None
  if self_op:
    idx = np.arange(len(src)) if targets_idx is None else np.asarray(targets_idx)
    t = src[idx]
  else:
    t = np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    idx = None
  vec = kind in ("G", "P")
  out = np.zeros((len(t), 3) if vec else len(t))
  for b0 in range(0, len(t), block):
    tb = t[b0:b0 + block]
    d = tb[:, None, :] - src[None, :, :]
    K = _kernel(kind, d, nrm)
    if self_op:
      mask = idx[b0:b0 + block, None] == np.arange(len(src))[None, :]
    else:
      mask = np.einsum("tsk,tsk->ts", d, d) < 1e-24
    K = np.where(mask[..., None] if vec else mask, 0.0, K)
    if wall:
      si, ni = _image(src, nrm)
      K = K + _kernel(kind, tb[:, None, :] - si[None, :, :], ni)
    out[b0:b0 + block] = np.einsum("ts...,s->t...", K, fw)
  return _F * out
