"""numpy restatement of the scattering sums (rigidmultiblobswall_amd/csrc/scattering_kernels.h), with a dtype argument:
np.float64 is what plain double arithmetic gives, np.longdouble the extended-precision reference of the tests.  The phase
takes the kernel's route: c_d = n_d / L_d, turns t = (x c_x + y c_y) + z c_z, r = t - rint(t), theta = 2 pi r.

  modes(frames, L, kint)                  rho_k(f) as (F, K, 2) = (sum cos, -sum sin)
  collective(modes, n_lags, ...)          C[l, k] = sum_o Re(rho(o + l) conj rho(o))
  self_sums(frames, L, kint, n_lags, ...) Sf[l, k] = sum_o sum_j cos(theta_j(o + l) - theta_j(o)), as Re(z(o + l) conj z(o))

each with absolute=True also the absolute sums its bound needs (modes_bound, collective_bound, self_bound; derivation in
test_gpu_scattering.py)."""
import numpy as np

U = 2.0 ** -53
C0, C1 = 4.0, 32.0


def pi(dtype):
  return dtype(4) * np.arctan(dtype(1))


def coefficients(L, kint, dtype=np.float64):
  n = np.asarray(kint).reshape(-1, 3)
  Ld = np.asarray(L, dtype=np.float64).reshape(3).astype(dtype)
  safe = np.where(Ld > 0, Ld, dtype(1))
  return np.where(n != 0, n.astype(dtype) / safe[None, :], dtype(0))


def reduced_turns(frames, L, kint, dtype=np.float64):
  """r (F, N, K): the phase in turns, reduced to [-1/2, 1/2], by the kernel's route"""
  x = np.asarray(frames, dtype=np.float64).astype(dtype)
  c = coefficients(L, kint, dtype)
  t = (x[..., 0, None] * c[:, 0] + x[..., 1, None] * c[:, 1]) + x[..., 2, None] * c[:, 2]
  return t - np.rint(t)


def turn_magnitudes(frames, L, kint):
  """T (F, N, K) = sum_d |n_d x_d / L_d|, float64: what a rounding of the turn count scales with"""
  x = np.abs(np.asarray(frames, dtype=np.float64))
  c = np.abs(coefficients(L, kint))
  return x[..., 0, None] * c[:, 0] + x[..., 1, None] * c[:, 1] + x[..., 2, None] * c[:, 2]


def phase_factors(frames, L, kint, dtype=np.float64):
  """z = exp(-i theta) as (re, im) = (cos theta, -sin theta), each (F, N, K)"""
  theta = (dtype(2) * pi(dtype)) * reduced_turns(frames, L, kint, dtype)
  return np.cos(theta), -np.sin(theta)


def modes(frames, L, kint, dtype=np.float64, absolute=False):
  re, im = phase_factors(frames, L, kint, dtype)
  rho = np.stack([re.sum(axis=1), im.sum(axis=1)], axis=-1)
  if absolute:
    return rho, turn_magnitudes(frames, L, kint).sum(axis=1)      # (F, K)
  return rho


def modes_bound(n_points, T_sum):
  return U * ((n_points + C0) * n_points + C1 * T_sum)


def _origins(F, n_lags, o_begin, o_end, origins):
  if o_end is None:
    o_end = max(F - n_lags + 1, 0) if origins == "window" else F
  return int(o_begin), int(o_end)


def collective(rho, n_lags, o_begin=0, o_end=None, origins="all", dtype=np.float64, absolute=False):
  """C (n_lags, K), the number of origins per lag, and with absolute=True A = sum_o (|a_r b_r| + |a_i b_i|)"""
  rho = np.asarray(rho).astype(dtype)
  F, K = rho.shape[0], rho.shape[1]
  o_begin, o_end = _origins(F, n_lags, o_begin, o_end, origins)
  C, A, n = np.zeros((n_lags, K), dtype=dtype), np.zeros((n_lags, K)), np.zeros(n_lags, dtype=np.int64)
  for lag in range(n_lags):
    hi = min(o_end, F - lag)
    if hi <= o_begin:
      continue
    a, b = rho[o_begin:hi], rho[o_begin + lag:hi + lag]
    C[lag] = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).sum(axis=0)
    A[lag] = (np.abs(a[..., 0] * b[..., 0]) + np.abs(a[..., 1] * b[..., 1])).sum(axis=0).astype(np.float64)
    n[lag] = hi - o_begin
  return (C, n, A) if absolute else (C, n)


def collective_bound(n_origins, A):
  return U * (n_origins[:, None] + 3.0) * A


def self_sums(frames, L, kint, n_lags, o_begin=0, o_end=None, origins="all", dtype=np.float64, absolute=False):
  """Sf (n_lags, K), the number of TERMS per lag (origins x points), and with absolute=True TT = sum (T_j(o) + T_j(o + l))"""
  re, im = phase_factors(frames, L, kint, dtype)
  T = turn_magnitudes(frames, L, kint) if absolute else None
  F, N, K = re.shape
  o_begin, o_end = _origins(F, n_lags, o_begin, o_end, origins)
  S, TT, n = np.zeros((n_lags, K), dtype=dtype), np.zeros((n_lags, K)), np.zeros(n_lags, dtype=np.int64)
  for lag in range(n_lags):
    hi = min(o_end, F - lag)
    if hi <= o_begin:
      continue
    S[lag] = (re[o_begin:hi] * re[o_begin + lag:hi + lag] + im[o_begin:hi] * im[o_begin + lag:hi + lag]).sum(axis=(0, 1))
    if absolute:
      TT[lag] = (T[o_begin:hi] + T[o_begin + lag:hi + lag]).sum(axis=(0, 1))
    n[lag] = (hi - o_begin) * N
  return (S, n, TT) if absolute else (S, n)


def self_bound(n_terms, TT):
  n = n_terms[:, None].astype(np.float64)
  return U * ((n + C0) * n + C1 * TT)


def pair_sum(frame, L, kint):
  """N + 2 sum_{i < j} cos k . r_ij in long double, (K,): |rho_k|^2 by another route"""
  x = np.asarray(frame, dtype=np.float64).astype(np.longdouble)
  c = coefficients(L, kint, np.longdouble)
  i, j = np.triu_indices(x.shape[0], 1)
  d = x[i] - x[j]
  t = d @ c.T
  return x.shape[0] + 2 * np.cos(2 * pi(np.longdouble) * (t - np.rint(t))).sum(axis=0)


def random_frames(F, N, L, seed, step=0.05, shift=0.0):
  """a random walk of N points from uniform positions in the box (open directions: a layer of height 1), every point
  shifted by `shift` periods along every direction"""
  rng = np.random.RandomState(seed)
  box = np.where(np.asarray(L, dtype=np.float64) > 0, np.asarray(L, dtype=np.float64), 1.0)
  x0 = rng.uniform(0, 1, (N, 3)) * box
  walk = np.cumsum(step * rng.standard_normal((F, N, 3)), axis=0)
  return np.ascontiguousarray(x0[None] + walk + shift * box)


def mixed_wavevectors(K, seed, n_max=9, plane="xyz"):
  """K distinct integer triples with mixed signs, n = 0 not among them"""
  rng = np.random.RandomState(seed)
  seen, out = set(), []
  while len(out) < K:
    n = tuple(int(v) for v in rng.randint(-n_max, n_max + 1, 3))
    if plane == "xy":
      n = (n[0], n[1], 0)
    if n != (0, 0, 0) and n not in seen:
      seen.add(n)
      out.append(n)
  return np.array(out, dtype=np.int32)


def config_text(frames):
  """a `.config` trajectory of the points of `frames` (F, N, 3), orientation columns 1 0 0 0"""
  lines = []
  for frame in frames:
    lines.append("%d" % frame.shape[0])
    lines.extend("%.17g %.17g %.17g 1 0 0 0" % tuple(p) for p in frame)
  return "\n".join(lines) + "\n"


def parse_output(text):
  """blocks of the command line's output: [(t or None, n_origins or None, rows (n, columns))]"""
  blocks, rows, head = [], [], (None, None)
  for line in text.splitlines():
    if line.startswith("# t"):
      if rows:
        blocks.append(head + (np.array(rows),))
      tok = line.split()
      head, rows = (float(tok[2]), int(tok[3])), []
    elif line.strip():
      rows.append([float(v) for v in line.split()])
  blocks.append(head + (np.array(rows),))
  return blocks
