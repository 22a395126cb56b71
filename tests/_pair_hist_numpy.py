"""numpy restatement of the pair-distance histogram (rmb_pair_histogram*) and of the reference program's g(r)
(multi_bodies/examples/Radial_Dist_Test/gr_pseudo2D_single_blob.cpp), shared by the host and GPU tests.

Per frame and unordered pair i < j: the separation, its minimal image in every direction with a positive period
(d - trunc(d / L + 0.5 sign(d)) L, the program's formula), r = sqrt(dx^2 + dy^2 + dz^2), bin = int(r / dr) with
dr = r_max / n_bins, counted when r < r_max.  Counts are of UNORDERED pairs; the program's integer column is twice that.

edge_margin(): the precondition that makes exact equality of integer counts a fair demand -- in long double, no pair has
r / dr within 1e-9 of an integer (r_max sits at the integer n_bins, so it is covered)."""
import numpy as np

EXT = np.longdouble


def _separations(x, L, dtype, rows):
  """yields (d, mask): separations x_i - x_j of the row block `rows` against all points, imaged; mask = j > i"""
  n = x.shape[0]
  d = x[rows, None, :] - x[None, :, :]
  for k in range(3):
    Lk = dtype(L[k])
    if Lk > 0:
      d[:, :, k] -= np.trunc(d[:, :, k] / Lk + dtype(0.5) * np.sign(d[:, :, k])) * Lk
  mask = np.arange(n)[None, :] > np.arange(n)[rows][:, None]
  return d, mask


def pair_distances(frame, L, dtype=np.float64, block=128):
  """distances of all unordered pairs of one frame (n, 3), as one array"""
  x = np.asarray(frame, dtype=np.float64).reshape(-1, 3).astype(dtype)
  out = []
  for i0 in range(0, x.shape[0], block):
    d, mask = _separations(x, L, dtype, slice(i0, min(i0 + block, x.shape[0])))
    out.append(np.sqrt(np.sum(d * d, axis=2))[mask])
  return np.concatenate(out) if out else np.zeros(0, dtype=dtype)


def counts(frames, L, r_max, n_bins):
  """uint64 counts of unordered pairs over all frames: (n_frames, n, 3) or (n, 3)"""
  f = np.asarray(frames, dtype=np.float64)
  f = f.reshape(-1, f.shape[-2], 3) if f.ndim >= 2 else f.reshape(0, 0, 3)
  dr = float(r_max) / int(n_bins)
  h = np.zeros(int(n_bins), dtype=np.int64)
  for frame in f:
    r = pair_distances(frame, L)
    r = r[r < r_max]
    b = np.minimum((r / dr).astype(np.int64), int(n_bins) - 1)
    h += np.bincount(b, minlength=int(n_bins))
  return h.astype(np.uint64)


SCREEN = 1e-6      # float64 screen of edge_margin: q = r / dr is good to ~1e-11 there (q < 1e5), far inside this width


def edge_margin(frames, L, r_max, n_bins, allow_zero=False):
  """smallest |r / dr - nearest integer| over all pairs of all frames (inf without pairs).  Every pair is screened in float64;
  the pairs within SCREEN of an integer -- the only ones that can be within 1e-9 of one -- are evaluated again in long double,
  and theirs is the value returned when there are any.
  allow_zero: pairs at exactly r = 0 (coincident points, built on purpose) are left out."""
  f = np.asarray(frames, dtype=np.float64)
  f = f.reshape(-1, f.shape[-2], 3)
  m = np.inf
  for frame in f:
    n = frame.shape[0]
    for i0 in range(0, n, 128):
      rows = slice(i0, min(i0 + 128, n))
      d, mask = _separations(frame, L, np.float64, rows)
      q = np.sqrt(np.sum(d * d, axis=2)) / (float(r_max) / int(n_bins))
      off = np.abs(q - np.rint(q))
      if allow_zero:
        mask = mask & (q != 0)
      if not mask.any():
        continue
      near = mask & (off < SCREEN)
      if near.any():
        i, j = np.nonzero(near)
        de = frame[rows][i].astype(EXT) - frame[j].astype(EXT)
        for k in range(3):
          Lk = EXT(L[k])
          if Lk > 0:
            de[:, k] -= np.trunc(de[:, k] / Lk + EXT(0.5) * np.sign(de[:, k])) * Lk
        qe = np.sqrt(np.sum(de * de, axis=1)) / (EXT(r_max) / EXT(int(n_bins)))
        if allow_zero:
          qe = qe[qe != 0]
        if qe.size:
          m = min(m, float(np.min(np.abs(qe - np.rint(qe)))))
      m = min(m, float(off[mask & ~near].min()) if (mask & ~near).any() else np.inf)
  return m


MARGIN = 1e-9


def points_with_margin(make, L, r_max, n_bins, seed, allow_zero=False, tries=20):
  """make(rng) -> frames; the first seed from `seed` on whose frames satisfy the edge-margin precondition.  -> frames"""
  for s in range(seed, seed + tries):
    frames = make(np.random.RandomState(s))
    if edge_margin(frames, L, r_max, n_bins, allow_zero) > MARGIN:
      return frames
  raise AssertionError("no seed in %d ... %d keeps every pair %g away from a bin edge" % (seed, seed + tries - 1, MARGIN))


def g_pseudo2d(counts_, n_frames, n_points, lx, ly, r_max):
  """the program's normalisation, written as the program writes it"""
  c = np.asarray(counts_, dtype=np.float64)
  dr = r_max / c.size
  lo = np.arange(c.size) * dr
  up = lo + dr
  ideal = np.pi * (n_points / (lx * ly)) * (up ** 2 - lo ** 2)
  return 2.0 * c / (n_frames * n_points * ideal)


def config_text(frames, final_newline=True):
  """frames (n_frames, n, 3) in the .config format (unit quaternions); the reference program counts the last frame twice when
  the file ends in a newline, so the goldens are written without it"""
  lines = []
  for frame in np.asarray(frames, dtype=np.float64):
    lines.append("%d" % len(frame))
    lines += ["%.17g %.17g %.17g 1 0 0 0" % tuple(x) for x in frame]
  return "\n".join(lines) + ("\n" if final_newline else "")


def parse_gr(text):
  """the three columns `r g hist` -> (r, g, hist as int64)"""
  rows = [l.split() for l in text.splitlines() if l.strip()]
  a = np.array(rows, dtype=np.float64).reshape(-1, 3)
  return a[:, 0], a[:, 1], np.rint(a[:, 2]).astype(np.int64)
