"""numpy restatement of the equilibrium sampler's potential energy, written from the formulas of DESIGN 3.9 (both forms):

  U = sum_i u1(z_i) + sum_{i<j, z_i > 0} u2(|r_i - r_j|),   a blob with z_i <= 0 contributes 1e5 (1 - z_i) instead of u1
  soft:    u1 = w z + (z < a ? e_w + e_w (a - z)/b_w : e_w exp(-(z - a)/b_w)),   u2 = r < 2a ? e + e (2a - r)/b : e exp(-(r - 2a)/b)
  yukawa:  u1 = w z + e_w a exp(-(z - a)/b_w)/|z - a| (+ 1e12 e_w when z < a),   u2 = e exp(-r/b)/r

with the minimal image in x and y (d - trunc(d/L + sign(d)/2) L).  Every term is evaluated and accumulated in
np.longdouble (EXT; float64 where long double has no 64-bit mantissa).  `energy` returns (U_one, U_pair, S) with
S = sum of |terms|: the scale a rounding bound of the sum is stated against (`split=True`: S of the one-blob and of the
pair terms separately).  `method`: "loops" = plain Python loops over
i < j (small N), "blocked" = rows of i against all j > i in vector form, "neighbours" = only the pairs within `reach`
(k-d tree; the caller states why the dropped terms do not matter).  This is the yardstick of the HIP energies: the
reference's kernel is a CUDA string nothing here can run."""
import numpy as np

LONG_DOUBLE = np.finfo(np.longdouble).nmant >= 63
EXT = np.longdouble if LONG_DOUBLE else np.float64


def _params(kw):
  L = kw.get("periodic_length")
  L = np.zeros(3) if L is None else np.asarray(L, dtype=np.float64)
  eps_w = kw.get("repulsion_strength_wall") or 0.0
  return (L, EXT(kw["repulsion_strength"]), EXT(kw["debye_length"]), EXT(eps_w), EXT(kw.get("debye_length_wall") or 1.0),
          EXT(kw.get("weight") or 0.0), EXT(kw["blob_radius"]), kw.get("potential", "soft"))


def one_blob_terms(z, eps_w, b_w, w, a, form):
  """u1 of every blob (EXT array); blobs with z <= 0 get 1e5 (1 - z)."""
  z = np.asarray(z, dtype=EXT)
  u = w * z
  if eps_w != 0:
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
      if form == "soft":
        u = u + np.where(z < a, eps_w + eps_w * (a - z) / b_w, eps_w * np.exp(-(z - a) / b_w))
      else:
        u = u + eps_w * a * np.exp(-(z - a) / b_w) / np.abs(z - a) + np.where(z < a, eps_w * EXT(1e12), EXT(0))
  return np.where(z > 0, u, EXT(1e5) * (1 - z))


def pair_terms(d, L, eps, b, a, form):
  """u2 for separations d (..., 3) (EXT), minimal image in x and y."""
  d = np.array(d, dtype=EXT)
  for k in (0, 1):
    if L[k] > 0:
      Lk = EXT(L[k])
      d[..., k] = d[..., k] - np.trunc(d[..., k] / Lk + EXT(0.5) * np.sign(d[..., k])) * Lk
  r = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2)
  with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
    if form == "soft":
      return np.where(r < 2 * a, eps + eps * (2 * a - r) / b, eps * np.exp(-np.maximum(r - 2 * a, 0) / b))
    return eps * np.exp(-r / b) / r


def energy(r_vectors, method=None, reach=None, split=False, **kw):
  L, eps, b, eps_w, b_w, w, a, form = _params(kw)
  r = np.asarray(r_vectors, dtype=np.float64).reshape(-1, 3)
  n = r.shape[0]
  x = r.astype(EXT)
  u1 = one_blob_terms(x[:, 2], eps_w, b_w, w, a, form)
  U_one, S_one = u1.sum(dtype=EXT), np.abs(u1).sum(dtype=EXT)
  S = EXT(0)       # of the pair terms, until the end
  U_pair = EXT(0)
  above = r[:, 2] > 0
  if method is None:
    method = "loops" if n <= 96 else "blocked"
  if method == "loops":
    for i in range(n):
      if not above[i]:
        continue
      for j in range(i + 1, n):
        t = pair_terms(x[i] - x[j], L, eps, b, a, form)
        U_pair = U_pair + t
        S = S + abs(t)
  elif method == "blocked":
    block = max(1, min(256, (1 << 21) // max(n, 1)))
    for i0 in range(0, n, block):
      i1 = min(n, i0 + block)
      t = pair_terms(x[i0:i1, None, :] - x[None, i0 + 1:, :], L, eps, b, a, form)        # (rows, j from i0 + 1 on)
      keep = (np.arange(i0 + 1, n)[None, :] > np.arange(i0, i1)[:, None]) & above[i0:i1, None]
      t = np.where(keep, t, EXT(0))
      U_pair = U_pair + t.sum(dtype=EXT)
      S = S + np.abs(t).sum(dtype=EXT)
  elif method == "neighbours":
    from scipy.spatial import cKDTree
    box = np.array([L[0] if L[0] > 0 else 0.0, L[1] if L[1] > 0 else 0.0, 0.0])
    y = r.copy()
    for k in (0, 1):
      if box[k] > 0:
        y[:, k] = np.mod(y[:, k], box[k])
        y[y[:, k] >= box[k], k] = 0.0
    tree = cKDTree(y, boxsize=box if box.any() else None)
    pairs = tree.query_pairs(float(reach), output_type="ndarray")
    lo, hi = np.minimum(pairs[:, 0], pairs[:, 1]), np.maximum(pairs[:, 0], pairs[:, 1])
    sel = above[lo]
    lo, hi = lo[sel], hi[sel]
    for c0 in range(0, lo.size, 1 << 18):
      t = pair_terms(x[lo[c0:c0 + (1 << 18)]] - x[hi[c0:c0 + (1 << 18)]], L, eps, b, a, form)
      U_pair = U_pair + t.sum(dtype=EXT)
      S = S + np.abs(t).sum(dtype=EXT)
  else:
    raise ValueError(method)
  if split:         # the two absolute-term sums separately: (U_one, U_pair, S_one, S_pair)
    return U_one, U_pair, S_one, S
  return U_one, U_pair, S_one + S


def total(r_vectors, **kw):
  """float64 total energy: what the reference's compute_total_energy returns (body potentials are empty)."""
  u1, u2, _ = energy(r_vectors, **kw)
  return float(u1 + u2)
