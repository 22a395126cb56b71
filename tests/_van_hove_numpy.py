"""numpy restatement of the van Hove lag histograms (rmb_van_hove_*_frames_device), shared by the host and GPU tests.

Frames (F, n, 3), origins o in [o_begin, o_end), lags l in [0, n_lags), a pair (o, l) only where o + l < F.
  self      the displacement x_j(o + l) - x_j(o) as it is; counts per bin and the moments sum r^2, sum r^4 over ALL terms;
  distinct  ORDERED pairs i != j: the separation x_i(o + l) - x_j(o), its minimal image in every direction with a positive period
            (d - trunc(d / L + 0.5 sign(d)) L, _pair_hist_numpy's formula).
plane "xy" drops the z component.  r = sqrt(sum d^2), bin = int(r / dr) with dr = r_max / n_bins, counted when r < r_max.
Everything takes dtype = np.float64 or np.longdouble (EXT); the inputs are always the fp64 frames.

edge_margin_*(): the precondition that makes exact equality of integer counts a fair demand -- in long double, no term has
r / dr within MARGIN = 1e-9 of an integer (r_max sits at the integer n_bins, so it is covered).  Terms at exactly r = 0 (every
self term of lag 0; coincident points built on purpose) are exempt."""
import numpy as np

import _pair_hist_numpy as phnp

EXT = np.longdouble
MARGIN = phnp.MARGIN
PLANES = {"xyz": 0, "xy": 1}


def origin_range(n_frames, n_lags, origins):
  """[0, o_end) of the convention: "window" -- only origins that have every lag; "all" -- every frame"""
  return 0, (max(n_frames - n_lags + 1, 0) if origins == "window" else n_frames)


def n_origins(n_frames, n_lags, o_begin, o_end):
  """origins per lag, int64 (n_lags,)"""
  return np.array([max(min(o_end, n_frames - l) - o_begin, 0) for l in range(n_lags)], dtype=np.int64)


def _frames(frames, dtype):
  f = np.asarray(frames, dtype=np.float64)
  return f.reshape(-1, f.shape[-2], 3).astype(dtype)


def _norm(d, plane, dtype):
  if plane == "xy":
    d = d[..., :2]
  return np.sqrt(np.sum(d * d, axis=-1, dtype=dtype))


def self_distances(frames, n_lags, o_begin, o_end, plane="xyz", dtype=np.float64):
  """list over lags of the displacement lengths of all (origin, point) terms, one flat array each"""
  f = _frames(frames, dtype)
  out = []
  for l in range(n_lags):
    last = min(o_end, f.shape[0] - l)
    if last <= o_begin:
      out.append(np.zeros(0, dtype=dtype))
      continue
    out.append(_norm(f[o_begin + l:last + l] - f[o_begin:last], plane, dtype).reshape(-1))
  return out


def distinct_distances(frames, L, n_lags, o_begin, o_end, plane="xyz", dtype=np.float64):
  """list over lags of the lengths of the imaged separations x_i(o + l) - x_j(o), i != j, one flat array each"""
  f = _frames(frames, dtype)
  n = f.shape[1]
  off = ~np.eye(n, dtype=bool)
  out = []
  for l in range(n_lags):
    rs = []
    for o in range(o_begin, min(o_end, f.shape[0] - l)):
      d = f[o + l][:, None, :] - f[o][None, :, :]
      for k in range(3):
        Lk = dtype(L[k])
        if Lk > 0:
          d[:, :, k] -= np.trunc(d[:, :, k] / Lk + dtype(0.5) * np.sign(d[:, :, k])) * Lk
      rs.append(_norm(d, plane, dtype)[off])
    out.append(np.concatenate(rs) if rs else np.zeros(0, dtype=dtype))
  return out


def _bin(distances, r_max, n_bins):
  n_bins = int(n_bins)
  h = np.zeros((len(distances), n_bins), dtype=np.int64)
  for l, r in enumerate(distances):
    r = np.asarray(r, dtype=np.float64)
    r = r[r < r_max]
    h[l] = np.bincount(np.minimum((r / (float(r_max) / n_bins)).astype(np.int64), n_bins - 1), minlength=n_bins)
  return h


def self_counts(frames, n_lags, o_begin, o_end, r_max, n_bins, plane="xyz"):
  return _bin(self_distances(frames, n_lags, o_begin, o_end, plane), r_max, n_bins)


def distinct_counts(frames, L, n_lags, o_begin, o_end, r_max, n_bins, plane="xyz"):
  return _bin(distinct_distances(frames, L, n_lags, o_begin, o_end, plane), r_max, n_bins)


def moments(frames, n_lags, o_begin, o_end, plane="xyz", dtype=np.float64):
  """(M (n_lags, 2) of `dtype`: sum r^2, sum r^4 over every term; n_terms (n_lags,))"""
  f = _frames(frames, dtype)
  M = np.zeros((n_lags, 2), dtype=dtype)
  terms = np.zeros(n_lags, dtype=np.int64)
  for l in range(n_lags):
    last = min(o_end, f.shape[0] - l)
    if last <= o_begin:
      continue
    d = f[o_begin + l:last + l] - f[o_begin:last]
    if plane == "xy":
      d = d[..., :2]
    r2 = np.sum(d * d, axis=-1, dtype=dtype).reshape(-1)
    M[l, 0], M[l, 1], terms[l] = np.sum(r2, dtype=dtype), np.sum(r2 * r2, dtype=dtype), r2.size
  return M, terms


def moment_bound(M_ext, n_terms):
  """|M - M_ext| <= (n_terms + 16) 2^-53 M_ext per lag and moment: every term non-negative, so any summation order stays within
  (n_terms - 1) units of the sum; a term carries at most 5 roundings in r^2 and 11 in r^4"""
  return (np.asarray(n_terms, dtype=EXT)[:, None] + 16) * EXT(2.0) ** -53 * np.asarray(M_ext, dtype=EXT)


def _margin(distances, r_max, n_bins):
  m = np.inf
  for r in distances:
    q = r / (EXT(r_max) / EXT(int(n_bins)))
    q = q[q != 0]
    if q.size:
      m = min(m, float(np.min(np.abs(q - np.rint(q)))))
  return m


def edge_margin_self(frames, n_lags, o_begin, o_end, r_max, n_bins, plane="xyz"):
  """smallest |r / dr - nearest integer| over the self terms with r != 0, in long double (inf without terms)"""
  return _margin(self_distances(frames, n_lags, o_begin, o_end, plane, EXT), r_max, n_bins)


def edge_margin_distinct(frames, L, n_lags, o_begin, o_end, r_max, n_bins, plane="xyz"):
  """the same over the cross-frame ordered pairs"""
  return _margin(distinct_distances(frames, L, n_lags, o_begin, o_end, plane, EXT), r_max, n_bins)


def random_walk(n, n_frames, box, step=0.05, periods=None):
  """make(rng) -> frames (n_frames, n, 3): a cloud over `box`, steps of size `step` per frame and coordinate, and -- periods (3,)
  of 0 / 1 -- per point a whole-period offset of up to +-2 periods in the marked directions, the same in every frame, as an
  unwrapped trajectory that crossed the box earlier carries"""
  def make(rng):
    x = rng.uniform(0, 1, (n, 3)) * box
    f = x[None] + np.cumsum(step * rng.standard_normal((n_frames, n, 3)), axis=0)
    if periods is not None:
      f = f + (rng.randint(-2, 3, (n, 3)) * (np.asarray(box) * np.asarray(periods))[None, :])[None]
    return f
  return make


def trajectory_with_margin(make, L, n_lags, r_max, n_bins, self_r_max, self_n_bins, seed, planes=("xyz", "xy"), tries=20):
  """make(rng) -> frames; the first seed from `seed` on whose frames keep every self and distinct term of every origin (the
  widest range: "all") MARGIN away from a bin edge under every plane asked for.  -> frames"""
  for s in range(seed, seed + tries):
    frames = make(np.random.RandomState(s))
    F = frames.shape[0]
    if all(edge_margin_self(frames, n_lags, 0, F, self_r_max, self_n_bins, p) > MARGIN and
           edge_margin_distinct(frames, L, n_lags, 0, F, r_max, n_bins, p) > MARGIN for p in planes):
      return frames
  raise AssertionError("no seed in %d ... %d keeps every term %g away from a bin edge" % (seed, seed + tries - 1, MARGIN))
