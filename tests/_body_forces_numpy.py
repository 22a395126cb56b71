"""numpy restatement of the reference's body-body law (multi_bodies_functions.py:359-408), in long double by default:
   F_i = sum_{j != i} -(eps/b + eps/r) exp(-r/b) d / r^2,   d = x_j - x_i in the minimal image of every direction with
   L > 0 (project_to_periodic_image, :71-82: the image count is truncated after adding half away from zero),
and of the Yukawa pair energy U = sum_{i<j} eps exp(-r/b) / r the law derives from.  Row blocks keep the memory of the
pair arrays bounded; no culling, every pair is evaluated."""
import numpy as np


def _pairs(x, L, lo, hi, dtype):
  d = x[None, :, :] - x[lo:hi, None, :]        # d[i, j] = x_j - x_i
  for k in range(3):
    if L[k] > 0:
      Lk = dtype(L[k])
      d[..., k] -= np.trunc(d[..., k] / Lk + dtype(0.5) * np.sign(d[..., k])) * Lk
  r = np.sqrt(np.sum(d * d, axis=-1))
  r[np.arange(hi - lo), np.arange(lo, hi)] = np.inf      # no self term (exp(-inf) = 0)
  return d, r


def forces(x, L, eps, b, dtype=np.longdouble, block=256):
  """(n, 3) forces in `dtype` arithmetic."""
  x = np.asarray(x, dtype=dtype).reshape(-1, 3)
  L = np.zeros(3) if L is None else np.asarray(L, dtype=np.float64).reshape(3)
  eps, b = dtype(eps), dtype(b)
  n = len(x)
  F = np.zeros((n, 3), dtype=dtype)
  for lo in range(0, n, block):
    hi = min(n, lo + block)
    d, r = _pairs(x, L, lo, hi, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):      # coincident centres: 0/0, as the reference
      f0 = -((eps / b) + (eps / r)) * np.exp(-r / b) / (r * r)
      f0[np.isinf(r)] = 0
      F[lo:hi] = np.sum(f0[..., None] * d, axis=1)
  return F


def energy(x, L, eps, b, dtype=np.longdouble, block=256):
  """U = sum over unordered pairs of eps exp(-r/b) / r."""
  x = np.asarray(x, dtype=dtype).reshape(-1, 3)
  L = np.zeros(3) if L is None else np.asarray(L, dtype=np.float64).reshape(3)
  eps, b = dtype(eps), dtype(b)
  U = dtype(0)
  for lo in range(0, len(x), block):
    hi = min(len(x), lo + block)
    _, r = _pairs(x, L, lo, hi, dtype)
    U += np.sum(eps * np.exp(-r / b) / r)
  return U / 2


def lattice_cloud(n, seed, spacing=1.3, jitter=0.1, dims=3):
  """n jittered lattice points (smallest separation >= spacing - 2 sqrt(dims) jitter) and the box that holds the lattice."""
  rng = np.random.RandomState(seed)
  m = max(1, int(np.ceil(n ** (1.0 / dims))))
  grid = np.stack(np.meshgrid(*([np.arange(m)] * dims), indexing="ij"), -1).reshape(-1, dims).astype(float)
  x = np.zeros((n, 3))
  x[:, :dims] = grid[rng.permutation(len(grid))[:n]] * spacing
  x += jitter * (2.0 * rng.rand(n, 3) - 1.0) + 0.5 * spacing
  return x, spacing * m


# The cloud of the gradient tests (host: the law itself; GPU: force sweep against the energy sweep): 300 centres on a
# jittered square lattice of spacing 1.3 above z = 0 (smallest separation >= 0.9 = b), periodic in x and y.
GRADIENT = dict(n=300, seed=1605, directions=3, eps=1.7, b=0.9, h=1e-4 * 0.9)


def gradient_cloud():
  x, box = lattice_cloud(GRADIENT["n"], GRADIENT["seed"], dims=2)
  x[:, 2] += 1.0 + 2.0 * np.random.RandomState(GRADIENT["seed"] + 1).rand(len(x))      # all z > 0
  assert x[:, 2].min() > 0
  return x, np.array([box, box, 0.0]), GRADIENT["eps"], GRADIENT["b"], GRADIENT["h"]
