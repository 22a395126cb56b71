"""numpy restatement of the hydrodynamic function's raw sums (rigidmultiblobswall_amd/csrc/hydro_function_kernels.h) and the
bound its tests hold the kernel to -- TEST infrastructure.

  S_self[f, m] = sum_i      b_i^2    e_m^T M_ii e_m
  S_dist[f, m] = sum_{i!=j} b_i b_j  e_m^T M_ij e_m  cos(theta_i - theta_j),      theta_i = k_m . x_i

M (damping included) is _mobility_numpy.blocks("tt", boundary, r, a, eta, mob_L, dtype): np.longdouble is the reference,
np.float64 what plain double arithmetic gives.  The phases are _scattering_numpy.reduced_turns on the RAW coordinates.

terms(...) returns the per-pair terms, so that one evaluation of the largest configuration serves every smaller test shape:
the block of a pair does not depend on the other points, the first N' points and the first K' wavevectors are a sub-array.

The bound (absolute, per frame and wavevector), u = 2^-53:

  tol_m = u * sum_ij [ 4 C + c_phase_ijm + c_sum ] s_ij

  s_ij      _mobility_numpy.scale("tt", ...): (1 / (8 pi eta)) sum_boxes (1 / max(r, a) + [wall] 1 / R) |b_i b_j|
  C         _mobility_numpy.C_ORACLE["tt", boundary, periodic]; 4 C u s_ij is the element bound of
            _pair_blocks_gpu.bound, MARGIN = 4 times the fp64 oracle's own worst error
  c_phase   a point's phase factor is off by at most u (C0 + C1 T_im), T_im = sum_d |n_d x_d / L_d| the size of its turn
            count (_scattering_numpy.modes_bound's per-point term); cos(theta_i - theta_j) = c_i c_j + s_i s_j takes it
            twice: c_phase_ijm = 2 C0 + C1 (T_im + T_jm)
  c_sum     the number of sequential additions a term passes through in the kernel: its lane's running sum sees at most
            one term per rotation step of the frame, 64 U with U = T (T + 1) / 2 units of T = ceil(N / 64) tiles; then 6
            levels of the wave's butterfly; then the finishing launch adds the records of the chunks that touch the frame,
            at most 64 U / spw + 2 of spw steps each.  A lane's part of a record is at most spw long, so the three together
            never exceed 64 U + 9 = c_sum.  (The self sums: at most ceil(N / 256) in a thread, 8 tree levels -- less.)
No figure in it comes from a kernel's output."""
import numpy as np

import _mobility_numpy as mn
import _scattering_numpy as sn
from _mobility_numpy import EXT

U = sn.U


def c_sum(n_points):
  tiles = (int(n_points) + 63) // 64
  return 64.0 * (tiles * (tiles + 1) // 2) + 9.0


def mob_lengths(mob_L):
  L = np.zeros(3) if mob_L is None else np.asarray(mob_L, dtype=np.float64).reshape(3)
  return L if L.any() else None


def terms(frame, a, eta, boundary, mob_L, L, kint, pol, dtype=EXT):
  """(self_terms (N, K), pair_terms (N, N, K), zero diagonal) of one frame (N, 3) in `dtype`."""
  T = np.dtype(dtype).type
  r = np.asarray(frame, dtype=np.float64).reshape(-1, 3)
  n = len(r)
  M = mn.blocks("tt", boundary, r, a, eta, mob_lengths(mob_L), dtype=dtype)      # (N, N, 3, 3), b_i b_j included
  e = np.asarray(pol, dtype=np.float64).reshape(-1, 3).astype(dtype)
  q = np.zeros((n, n, len(e)), dtype=dtype)
  for c in range(3):
    for d in range(3):
      q = q + M[:, :, c, d, None] * (e[:, c] * e[:, d])[None, None, :]
  turns = sn.reduced_turns(r[None], L, kint, dtype)[0]                           # (N, K)
  theta = (T(2) * sn.pi(T)) * turns
  co, si = np.cos(theta), np.sin(theta)
  phase = co[:, None, :] * co[None, :, :] + si[:, None, :] * si[None, :, :]
  idx = np.arange(n)
  self_terms = q[idx, idx, :].copy()
  pair = q * phase
  pair[idx, idx, :] = 0
  return self_terms, pair


def sums(frames, a, eta, boundary, mob_L, L, kint, pol, dtype=EXT):
  """(F, K, 2) = (S_self, S_dist) in `dtype`."""
  frames = np.asarray(frames, dtype=np.float64)
  out = np.zeros((frames.shape[0], len(np.asarray(kint).reshape(-1, 3)), 2), dtype=dtype)
  for f, frame in enumerate(frames):
    s, p = terms(frame, a, eta, boundary, mob_L, L, kint, pol, dtype)
    out[f, :, 0] = s.sum(axis=0)
    out[f, :, 1] = p.sum(axis=(0, 1))
  return out


def weights(frame, a, eta, boundary, mob_L, L, kint):
  """(s (N, N) float64, w (N, N, K) float64): the block scale, and s_ij (4 C + c_phase_ijm) -- everything of the bound but c_sum."""
  r = np.asarray(frame, dtype=np.float64).reshape(-1, 3)
  mL = mob_lengths(mob_L)
  s = np.asarray(mn.scale("tt", boundary, r, a, eta, mL), dtype=np.float64)
  C = mn.C_ORACLE["tt", boundary, mL is not None]
  T = sn.turn_magnitudes(r[None], L, kint)[0]                                    # (N, K)
  w = s[:, :, None] * (4.0 * C + 2.0 * sn.C0 + sn.C1 * (T[:, None, :] + T[None, :, :]))
  return s, w


def bounds(s, w, n_points=None):
  """(K, 2): the bound of (S_self, S_dist) from weights() of the first n_points points (sub-arrays are the caller's)."""
  n = s.shape[0] if n_points is None else int(n_points)
  idx = np.arange(s.shape[0])
  cs = c_sum(n)
  d_self = w[idx, idx, :].sum(axis=0) + cs * s[idx, idx].sum()
  total = w.sum(axis=(0, 1)) + cs * s.sum()
  return U * np.stack([d_self, total - d_self], axis=1)


def bounds_of(frames, a, eta, boundary, mob_L, L, kint):
  """(F, K, 2)"""
  return np.stack([bounds(*weights(fr, a, eta, boundary, mob_L, L, kint)) for fr in np.asarray(frames, dtype=np.float64)])


# ---------------------------------------------------------------------------------------------------------------------
# the designed trajectories of the tests: three frames of the 200-point regime cloud of _mobility_numpy
# ---------------------------------------------------------------------------------------------------------------------
A, ETA = mn.A, mn.ETA
LZ = 7.3                      # reference length of the wavevectors' z direction (the mobility is never periodic in z here)
CASES = {"wall_open": ("wall", False), "none_open": ("none", False), "wall_periodic": ("wall", "odd"), "none_periodic": ("none", "odd")}
SPECIAL_Z = (-0.3, 0.0, -1e-9, 0.5 * A)      # clamp and damping: below the wall, on it, just below, half a radius up
N_FRAMES, K_MAX = 3, 19
_cache = {}


def trajectory(case, shift=0.0):
  """(frames (3, 200, 3), L of the wavevectors, mob_L or None) of CASES[case]; every x and y shifted by `shift` periods."""
  boundary, periodic = CASES[case]
  base = np.array(mn.BOXES["odd"]) * (A / 0.5)
  L = np.array([base[0], base[1], LZ])
  # a shifted cloud is built shifted (regime_cloud then leaves out the partners at 2a -+ 4e-12 a, which do not exist next to
  # the offset and would fall onto the r = 2a partner): by `shift` periods in x there, the rest of the y shift here
  r, boxL = mn.regime_cloud(A, periodic, shift * L[0])
  r = r.copy()
  r[:, 1] += shift * (L[1] - L[0])
  # blobs well above the wall with nobody above or below them (the clamp would put two stacked ones onto each other)
  alone = [i for i in range(len(r)) if np.sum((r[:, 0] == r[i, 0]) & (r[:, 1] == r[i, 1])) == 1]
  order = [i for i in alone if r[i, 2] > 1.5 * A][:len(SPECIAL_Z)]
  for i, z in zip(order, SPECIAL_Z):
    r[i, 2] = z
  # the first two points of every sub-shape carry special heights: below the wall (b < 0) and half a radius up
  lead = [order[0], order[3]]
  rest = [i for i in range(len(r)) if i not in lead]
  r = r[lead + rest]
  rng = np.random.RandomState(7)
  frames = np.stack([r, r + 0.01 * A * rng.standard_normal(r.shape), r + 0.01 * A * rng.standard_normal(r.shape)])
  mob_L = np.array([L[0], L[1], 0.0]) if periodic else None
  return frames, L, mob_L


def wavevectors_and_polarisations():
  kint = sn.mixed_wavevectors(K_MAX, 5, n_max=6, plane="xyz")
  rng = np.random.RandomState(11)
  e = rng.standard_normal((K_MAX, 3))
  e /= np.sqrt((e * e).sum(axis=1))[:, None]
  e[0] = (1.0, 0.0, 0.0); e[1] = (0.0, 0.0, 1.0)
  return kint, np.ascontiguousarray(e)


def reference(case, shift=0.0):
  """Everything the GPU tests compare against, computed once per process: frames, L, mob_L, kint, pol, and per frame the EXT
  terms (self (N, K), pair (N, N, K)) and the weights (s, w)."""
  key = (case, shift)
  if key not in _cache:
    boundary, _ = CASES[case]
    frames, L, mob_L = trajectory(case, shift)
    kint, pol = wavevectors_and_polarisations()
    per = []
    for fr in frames:
      st, pt = terms(fr, A, ETA, boundary, mob_L, L, kint, pol)
      assert np.all(np.isfinite(st.astype(np.float64))) and np.all(np.isfinite(pt.astype(np.float64))), "non-finite reference: coincident points?"
      per.append((st, pt) + weights(fr, A, ETA, boundary, mob_L, L, kint))
    _cache[key] = dict(boundary=boundary, frames=frames, L=L, mob_L=mob_L, kint=kint, pol=pol, per=per)
  return _cache[key]


def expected(ref, n_points, K, n_frames):
  """(sums (n_frames, K, 2) EXT, bounds (n_frames, K, 2) float64) of the first n_points points, K wavevectors, n_frames frames."""
  S = np.zeros((n_frames, K, 2), dtype=EXT)
  B = np.zeros((n_frames, K, 2))
  for f in range(n_frames):
    st, pt, s, w = ref["per"][f]
    S[f, :, 0] = st[:n_points, :K].sum(axis=0)
    S[f, :, 1] = pt[:n_points, :n_points, :K].sum(axis=(0, 1))
    B[f] = bounds(s[:n_points, :n_points], w[:n_points, :n_points, :K], n_points)
  return S, B


def worst(got, S, B):
  """max |got - S| / B"""
  err = np.abs(np.asarray(got, dtype=EXT) - S).astype(np.float64)
  return float(np.max(err / B))
