"""numpy restatement of the bond-orientational order sweeps (rmb_bond_order_frames_device, rmb_pair_field_frames_device), shared
by the host and GPU tests.

Pass 1 (neighbour_sums): per frame and point i, the neighbours j with d_ij^2 < r_cut^2 and rho_ij^2 > 0 -- separations in the
minimal image of every direction with a positive period (d - trunc(d / L + 0.5 sign(d)) L), rho the in-plane distance, d = rho
(plane "xy") or the 3-D distance ("xyz") -- and the sums of cos(m theta), sin(m theta), theta = atan2(dy, dx): in np.longdouble
with TRUE trigonometry (the kernel has none).  neighbour_sums_fp64 is the kernel's arithmetic in plain fp64 numpy (one
reciprocal square root, binary powering).  sum_bound is the bound of DESIGN.md 3.9.4 on |kernel - long double| per sum,
computed from the data: N E_m + N (N - 1) 2^-53, E_m = m (eps_rsqrt + c 2^-53 max_j |d_raw| / rho) + 2 floor(log2 m) sqrt(5) 2^-53.

Pass 2 (pair_field): per frame and unordered pair with r < r_max, binned as _pair_hist_numpy.counts: counts[bin] += 1,
sums[bin] += (a_i a_j + b_i b_j + 2^29) >> 30 in int64.

Preconditions that make exact equality of neighbour sets and counts a fair demand (cut_margin, bin_margin, MARGIN): in long
double no pair has d / r_cut within 1e-9 of 1, and no pair has r / dr within 1e-9 of an integer."""
import numpy as np

import _pair_hist_numpy as phnp

EXT = np.longdouble
MARGIN = 1e-9
U = 2.0 ** -53
EPS_RSQRT = 3e-16      # rsqrt_f64 (pair_ops.h; DESIGN.md 2: "third-order correction, 3e-16")
C_SEP = 9.0            # 6 sqrt(2) rounded up: the separation's roundings as they reach z
SLACK = 1.0 + 2.0 ** -20      # second-order terms of the first-order bound, and the long-double reference's own error


def _images(x, L, plane, dtype):
  """(raw, d): x_i - x_j as they are, and in the minimal image; plane "xy" leaves z alone (it is not used)"""
  raw = x[:, None, :] - x[None, :, :]
  d = raw.copy()
  for k in range(2 if plane == "xy" else 3):
    Lk = dtype(L[k])
    if Lk > 0:
      d[:, :, k] -= np.trunc(d[:, :, k] / Lk + dtype(0.5) * np.sign(d[:, :, k])) * Lk
  return raw, d


def _neighbourhood(frame, L, r_cut, plane, dtype):
  x = np.asarray(frame, dtype=np.float64).reshape(-1, 3).astype(dtype)
  raw, d = _images(x, L, plane, dtype)
  rho2 = d[:, :, 0] ** 2 + d[:, :, 1] ** 2
  d2 = rho2 if plane == "xy" else rho2 + d[:, :, 2] ** 2
  rc = dtype(r_cut)
  return raw, d, rho2, d2, (d2 < rc * rc) & (rho2 > 0)


def neighbour_sums(frames, L, r_cut, orders, plane="xy", dtype=EXT):
  """-> N int64 (F, n), S dtype (F, n, K, 2), ratio float64 (F, n): max over the neighbours of max(|dx_raw|, |dy_raw|) / rho"""
  f = np.asarray(frames, dtype=np.float64)
  f = f.reshape(-1, f.shape[-2], 3)
  F, n, K = f.shape[0], f.shape[1], len(orders)
  N, S, ratio = np.zeros((F, n), dtype=np.int64), np.zeros((F, n, K, 2), dtype=dtype), np.zeros((F, n))
  for t in range(F):
    raw, d, rho2, _, nb = _neighbourhood(f[t], L, r_cut, plane, dtype)
    N[t] = nb.sum(axis=1)
    theta = np.arctan2(d[:, :, 1], d[:, :, 0])
    for k, m in enumerate(orders):
      S[t, :, k, 0] = np.where(nb, np.cos(dtype(m) * theta), dtype(0)).sum(axis=1)
      S[t, :, k, 1] = np.where(nb, np.sin(dtype(m) * theta), dtype(0)).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
      q = np.maximum(np.abs(raw[:, :, 0]), np.abs(raw[:, :, 1])) / np.sqrt(rho2)
    ratio[t] = np.where(nb, q, dtype(0)).max(axis=1).astype(np.float64) if n else 0.0
  return N, S, ratio


def neighbour_sums_fp64(frames, L, r_cut, orders, plane="xy"):
  """the kernel's arithmetic in fp64 numpy: z = d / sqrt(rho^2), z^m by left-to-right binary powering -> N, S (F, n, K, 2)"""
  f = np.asarray(frames, dtype=np.float64)
  f = f.reshape(-1, f.shape[-2], 3)
  F, n, K = f.shape[0], f.shape[1], len(orders)
  N, S = np.zeros((F, n), dtype=np.int64), np.zeros((F, n, K, 2))
  for t in range(F):
    _, d, rho2, _, nb = _neighbourhood(f[t], L, r_cut, plane, np.float64)
    N[t] = nb.sum(axis=1)
    ir = 1.0 / np.sqrt(np.where(nb, rho2, 1.0))
    zx, zy = np.where(nb, d[:, :, 0] * ir, 0.0), np.where(nb, d[:, :, 1] * ir, 0.0)
    for k, m in enumerate(orders):
      px, py = zx, zy
      for b in range(int(m).bit_length() - 2, -1, -1):
        px, py = px * px - py * py, 2.0 * (px * py)
        if (m >> b) & 1:
          px, py = px * zx - py * zy, px * zy + py * zx
      S[t, :, k, 0], S[t, :, k, 1] = px.sum(axis=1), py.sum(axis=1)
  return N, S


def sum_bound(N, ratio, orders):
  """the derived bound on |kernel sum - long-double sum| per component: float64 (F, n, K)"""
  N = np.asarray(N, dtype=np.float64)[..., None]
  m = np.asarray(orders, dtype=np.float64)
  E = m * (EPS_RSQRT + C_SEP * U * np.asarray(ratio)[..., None]) + 2.0 * np.floor(np.log2(m)) * np.sqrt(5.0) * U
  return (N * E + N * (N - 1.0) * U) * SLACK


def psi_of(N, S):
  """psi = S / N (0 where N = 0), complex128 (F, n, K)"""
  Nf = np.asarray(N, dtype=np.float64)[..., None]
  S = np.asarray(S, dtype=np.float64)
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.where(Nf > 0, S[..., 0] / Nf, 0.0) + 1j * np.where(Nf > 0, S[..., 1] / Nf, 0.0)


def cut_margin(frames, L, r_cut, plane="xy"):
  """smallest |d / r_cut - 1| over all pairs of all frames, in long double (inf without pairs)"""
  f = np.asarray(frames, dtype=np.float64)
  f = f.reshape(-1, f.shape[-2], 3)
  m = np.inf
  for frame in f:
    n = frame.shape[0]
    for i0 in range(0, n, 256):
      x = frame.astype(EXT)
      d = x[i0:i0 + 256, None, :] - x[None, :, :]
      for k in range(2 if plane == "xy" else 3):
        Lk = EXT(L[k])
        if Lk > 0:
          d[:, :, k] -= np.trunc(d[:, :, k] / Lk + EXT(0.5) * np.sign(d[:, :, k])) * Lk
      d2 = d[:, :, 0] ** 2 + d[:, :, 1] ** 2 + (0 if plane == "xy" else d[:, :, 2] ** 2)
      off = np.abs(np.sqrt(d2) / EXT(r_cut) - 1)
      off[np.arange(d.shape[0]), np.arange(i0, i0 + d.shape[0])] = np.inf
      if off.size:
        m = min(m, float(off.min()))
  return m


def _in_plane(frames, L, plane):
  """the in-plane distance is the 3-D distance of the points with z = 0 in a box that is open in z"""
  f = np.array(frames, dtype=np.float64)
  f = f.reshape(-1, f.shape[-2], 3)
  L = np.array(L, dtype=np.float64)
  if plane == "xy":
    f[:, :, 2] = 0.0
    L[2] = 0.0
  return f, L


def bin_margin(frames, L, r_max, n_bins, plane="xy", allow_zero=False):
  f, L = _in_plane(frames, L, plane)
  return phnp.edge_margin(f, L, r_max, n_bins, allow_zero)


def frames_with_margin(make, L, r_cut, plane="xy", r_max=None, n_bins=0, seed=0, tries=20, allow_zero=False):
  """make(rng) -> frames; the first seed from `seed` on whose frames keep every pair off the cutoff and (n_bins > 0) off the
  bin edges -> frames"""
  for s in range(seed, seed + tries):
    frames = make(np.random.RandomState(s))
    if cut_margin(frames, L, r_cut, plane) > MARGIN and (not n_bins or bin_margin(frames, L, r_max, n_bins, plane, allow_zero) > MARGIN):
      return frames
  raise AssertionError("no seed in %d ... %d satisfies the margins" % (seed, seed + tries - 1))


def pair_field(frames, field, L, r_max, n_bins, plane="xy"):
  """-> counts int64 [n_bins], sums int64 [n_bins]"""
  f, L = _in_plane(frames, L, plane)
  q = np.asarray(field, dtype=np.int64).reshape(f.shape[0], f.shape[1], 2)
  dr = float(r_max) / int(n_bins)
  counts, sums = np.zeros(int(n_bins), dtype=np.int64), np.zeros(int(n_bins), dtype=np.int64)
  for frame, fld in zip(f, q):
    n = frame.shape[0]
    for i0 in range(0, n, 128):
      rows = slice(i0, min(i0 + 128, n))
      d, mask = phnp._separations(frame, L, np.float64, rows)
      r = np.sqrt(np.sum(d * d, axis=2))
      mask &= r < r_max
      i, j = np.nonzero(mask)
      b = np.minimum((r[i, j] / dr).astype(np.int64), int(n_bins) - 1)
      i = i + i0
      term = (fld[i, 0] * fld[j, 0] + fld[i, 1] * fld[j, 1] + (1 << 29)) >> 30
      counts += np.bincount(b, minlength=int(n_bins))
      np.add.at(sums, b, term)
  return counts, sums


def random_field(rng, shape):
  """int32 (..., 2) in [-2^30, 2^30] with the extremes and 0 planted"""
  q = rng.randint(-2 ** 30, 2 ** 30 + 1, size=tuple(shape) + (2,)).astype(np.int64)
  flat = q.reshape(-1)
  special = np.array([2 ** 30, -2 ** 30, 0, 2 ** 30, -2 ** 30, 0])
  idx = rng.permutation(flat.size)[:min(flat.size, 3 * special.size)]
  flat[idx] = special[np.arange(idx.size) % special.size]
  return q.astype(np.int32)


def triangular_lattice(nx, ny, a=1.0):
  """nx x ny points (ny even) of spacing a in the periodic box (nx a, ny a sqrt(3) / 2, 0) -> points (n, 3), L"""
  i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
  x = (i + 0.5 * (j % 2)) * a
  y = j * (a * np.sqrt(3.0) / 2.0)
  pts = np.stack([x.reshape(-1), y.reshape(-1), np.zeros(nx * ny)], axis=1)
  return pts, np.array([nx * a, ny * a * np.sqrt(3.0) / 2.0, 0.0])


def square_lattice(nx, ny, a=1.0):
  i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
  pts = np.stack([(i * a).reshape(-1).astype(np.float64), (j * a).reshape(-1).astype(np.float64), np.zeros(nx * ny)], axis=1)
  return pts, np.array([nx * a, ny * a, 0.0])


def lag_sums(psi, n_lags, origins):
  """C[k, l] = sum_o sum_i Re psi(o + l, i, k) conj psi(o, i, k) in long double; psi complex (F, n, K) -> (C (K, n_lags), A): A
  the same sums of |term| <= |psi||psi| (the scale of the bound), n_origins per lag"""
  F, n, K = psi.shape
  re, im = psi.real.astype(EXT), psi.imag.astype(EXT)
  C, A, n_or = np.zeros((K, n_lags), dtype=EXT), np.zeros((K, n_lags), dtype=EXT), np.zeros(n_lags, dtype=np.int64)
  last = F - n_lags + 1 if origins == "window" else F
  for l in range(n_lags):
    for o in range(0, max(last, 0)):
      if o + l >= F:
        break
      t = re[o + l] * re[o] + im[o + l] * im[o]
      C[:, l] += t.sum(axis=0)
      A[:, l] += (np.abs(re[o + l] * re[o]) + np.abs(im[o + l] * im[o])).sum(axis=0)
      n_or[l] += 1
  return C, A, n_or
