"""numpy restatement of the cluster analysis (rmb_cluster_labels*, clusters.Clusters), shared by the host and GPU tests.

Per frame: the separation of every pair, its minimal image in every direction with a positive period (the formula of
_pair_hist_numpy), r^2 = dx^2 + dy^2 (+ dz^2 under plane "xyz"; under "xy" z and L_z are ignored) in plain float64; i and j are
bonded when r^2 < r_cut^2, strictly, and both are selected.  Components by a plain union-find; the label of a point is the
smallest index of its component, -1 when it is not selected; sizes[l] is the size of the cluster labelled l, 0 elsewhere.

bond_margin(): the precondition that makes exact equality of integers a fair demand -- in long double no pair has r^2 within
1e-9 r_cut^2 of r_cut^2, while the fp64 error of r^2 is ~1e-15 relative to the squared coordinates' differences."""
import numpy as np

from _pair_hist_numpy import EXT

MARGIN = 1e-9


def _frames(frames):
  f = np.asarray(frames, dtype=np.float64)
  return f.reshape(-1, f.shape[-2], 3)


def _r2(x, L, plane, dtype=np.float64, rows=slice(None)):
  """(rows, n) squared distances of one frame"""
  x = np.asarray(x, dtype=np.float64).astype(dtype)
  r2 = np.zeros((x[rows].shape[0], x.shape[0]), dtype=dtype)
  for k in range(2 if plane == "xy" else 3):
    d = x[rows, None, k] - x[None, :, k]
    Lk = dtype(L[k])
    if Lk > 0:
      d -= np.trunc(d / Lk + dtype(0.5) * np.sign(d)) * Lk
    r2 += d * d
  return r2


BLOCK = 512      # rows per block: a frame of a few thousand points stays within tens of megabytes


def bonds(frame, L, r_cut, plane="xyz", select=None):
  """(n, n) bool adjacency of one frame, diagonal False"""
  n = np.asarray(frame).shape[0]
  rc2 = np.float64(r_cut) * np.float64(r_cut)
  adj = np.concatenate([_r2(frame, L, plane, rows=slice(i0, i0 + BLOCK)) < rc2 for i0 in range(0, n, BLOCK)]) if n else np.zeros((0, 0), bool)
  adj[np.arange(n), np.arange(n)] = False
  if select is not None:
    s = np.asarray(select).astype(bool)
    adj &= s[:, None] & s[None, :]
  return adj


def components(adj, select=None):
  """labels (n,) int32 by a plain union-find over the adjacency: the smallest index of the component, -1 = unselected"""
  n = adj.shape[0]
  parent = list(range(n))

  def find(x):
    while parent[x] != x:
      parent[x] = parent[parent[x]]
      x = parent[x]
    return x
  for i, j in zip(*np.nonzero(np.triu(adj, 1))):
    a, b = find(int(i)), find(int(j))
    if a != b:
      parent[max(a, b)] = min(a, b)
  labels = np.array([find(i) for i in range(n)], dtype=np.int32).reshape(n)
  if select is not None:
    labels[~np.asarray(select).astype(bool)] = -1
  return labels


def sizes_of(labels):
  lab = np.asarray(labels)
  return np.bincount(lab[lab >= 0], minlength=lab.size).astype(np.int32)[:lab.size] if lab.size else np.zeros(0, dtype=np.int32)


def labels_sizes(frames, L, r_cut, plane="xyz", select=None):
  """(labels, sizes), int32 (n_frames, n) each"""
  f = _frames(frames)
  sel = None if select is None else np.asarray(select).reshape(f.shape[0], f.shape[1])
  labels = np.zeros(f.shape[:2], dtype=np.int32)
  sizes = np.zeros(f.shape[:2], dtype=np.int32)
  for k, frame in enumerate(f):
    s = None if sel is None else sel[k]
    labels[k] = components(bonds(frame, L, r_cut, plane, s), s)
    sizes[k] = sizes_of(labels[k])
  return labels, sizes


def closure_labels(adj, select=None):
  """the same labels by brute force, O(n^3): the transitive closure of the adjacency (Warshall)"""
  n = adj.shape[0]
  reach = adj | np.eye(n, dtype=bool)
  for k in range(n):
    reach |= reach[:, k:k + 1] & reach[k:k + 1, :]
  labels = np.array([int(np.nonzero(reach[i])[0][0]) for i in range(n)], dtype=np.int32).reshape(n)
  if select is not None:
    labels[~np.asarray(select).astype(bool)] = -1
  return labels


def statistics(labels, sizes):
  """What clusters.Clusters holds, from (labels, sizes) (n_frames, n): dict of n_selected, n_clusters, largest, sum_squares (int64
  per frame) and n_s (int64, n + 1 entries)."""
  labels, sizes = np.asarray(labels), np.asarray(sizes).astype(np.int64)
  n = labels.shape[1]
  n_s = np.bincount(sizes.reshape(-1), minlength=n + 1).astype(np.int64)
  n_s[0] = 0
  return dict(n_selected=np.count_nonzero(labels >= 0, axis=1).astype(np.int64), n_clusters=np.count_nonzero(sizes > 0, axis=1).astype(np.int64),
              largest=sizes.max(axis=1) if n else np.zeros(labels.shape[0], dtype=np.int64), sum_squares=(sizes * sizes).sum(axis=1), n_s=n_s)


def mean_size(n_s):
  s = np.arange(len(n_s), dtype=np.int64)
  return np.float64(int(np.sum(s * n_s))) / np.float64(int(np.sum(n_s)))


def weight_mean_size(n_s):
  s = np.arange(len(n_s), dtype=np.int64)
  return np.float64(int(np.sum(s * s * n_s))) / np.float64(int(np.sum(s * n_s)))


def format_lines(stats):
  """the command line's output, from statistics()"""
  out = []
  for f in range(len(stats["n_selected"])):
    ns, nc = np.float64(stats["n_selected"][f]), np.float64(stats["n_clusters"][f])
    with np.errstate(divide="ignore", invalid="ignore"):
      out.append("%d %d %d %d %.17g %.17g" % (f, stats["n_selected"][f], stats["n_clusters"][f], stats["largest"][f], ns / nc,
                                               np.float64(stats["sum_squares"][f]) / ns))
  out.extend("%d %d" % (s, stats["n_s"][s]) for s in np.nonzero(stats["n_s"])[0])
  return out


SCREEN = 1e-6      # float64 screen of bond_margin: r^2 / r_cut^2 is good to ~1e-12 there, far inside this width


def bond_margin(frames, L, r_cut, plane="xyz"):
  """min |r^2 - r_cut^2| / r_cut^2 over all pairs of all frames (inf without pairs).  Every pair is screened in float64; the
  pairs within SCREEN -- the only ones that can be within 1e-9 -- are evaluated again in np.longdouble, and theirs is the value
  returned when there are any."""
  rc2 = EXT(r_cut) * EXT(r_cut)
  m = np.inf
  for frame in _frames(frames):
    n = frame.shape[0]
    for i0 in range(0, n if n > 1 else 0, BLOCK):
      off = np.abs(_r2(frame, L, plane, rows=slice(i0, i0 + BLOCK)) / np.float64(rc2) - 1.0)
      off[np.arange(off.shape[0]), i0 + np.arange(off.shape[0])] = np.inf      # the point itself
      near = off < SCREEN
      if near.any():
        i, j = np.nonzero(near)
        pts = np.stack([frame[i0 + i], frame[j]], axis=1)      # (pairs, 2, 3)
        m = min([m] + [float(abs(_r2(p, L, plane, EXT)[0, 1] - rc2) / rc2) for p in pts])
        off[near] = np.inf
      m = min(m, float(off.min()))
  return m
