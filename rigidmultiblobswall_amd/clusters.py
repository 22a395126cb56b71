"""Cluster analysis of point trajectories on MI355X: which points belong together.

    python -m rigidmultiblobswall_amd.clusters run.config np lx ly lz --rcut R [--plane xy|xyz] [--every K] [--skip S]
                                               [--psi M,THRESH,RCUT_PSI] [--device N]

The positional arguments are those of rigidmultiblobswall_amd.correlation (a `.config` trajectory, the number of bodies, the
box); the points are the location columns.  It prints one line `frame n_selected n_clusters largest mean_size weight_mean_size`
per frame, then one line `s n_s` for every cluster size s that occurred.

Points i and j of a frame are bonded when d_ij < r_cut, strictly, in the minimal image of every direction with a positive period
(d the 3-D distance under plane="xyz", the in-plane distance under "xy"; coincident and, under "xy", stacked points are bonded).
A cluster is a connected component of the bond graph; its label is the smallest index in it.  With a selection only bonds
between two selected points exist and an unselected point belongs to no cluster: `--psi 6,0.7,1.5` selects the points with
|psi_6(i)| >= 0.7 (neighbour cutoff 1.5, MobilityContext.bond_order_frames_device), which gives the solid-like clusters.

Labels and sizes come from the HIP sweep rmb_cluster_labels_frames_device (a lock-free union-find under the pair-once frame);
they are integers that do not depend on the launch plan or the point order.  The statistics are exact integers per frame (number
of selected points, number of clusters, largest size, sum of squared sizes) and the accumulated size distribution n_s, so they do
not depend on how the trajectory is cut into add_frames calls either.  The reductions from (labels, sizes) to these numbers are
torch calls on the device.  There is no CPU fall-back.

Not here: percolation / spanning detection, per-cluster centre of mass and gyration (they need unwrapping along bonds), cluster
tracking in time, per-point radii as bond lengths, single precision, multi-device contexts.
"""
import argparse
import sys

import numpy as np

from ._lagged import UPLOAD_BYTES, ContextHolder, lengths as _lengths

PLANES = ("xy", "xyz")
MAX_POINTS_PER_CALL = 2 ** 31 - 1      # entries of the parent array of one call (int32 indices)


def number_mean(n_s):
  """sum s n_s / sum n_s (nan without clusters)"""
  n_s = np.asarray(n_s, dtype=np.int64)
  s = np.arange(n_s.size, dtype=np.int64)
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.float64(int(np.sum(s * n_s))) / np.float64(int(np.sum(n_s)))


def weight_mean(n_s):
  """sum s^2 n_s / sum s n_s (nan without clusters)"""
  n_s = np.asarray(n_s, dtype=np.int64)
  s = np.arange(n_s.size, dtype=np.int64)
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.float64(int(np.sum(s * s * n_s))) / np.float64(int(np.sum(s * n_s)))


def psi_select(ctx, frames, periodic_length, order, threshold, r_cut_psi, plane="xy"):
  """The selection |psi_m(i)| >= threshold of `frames`, a contiguous CUDA float64 tensor (k, n, 3): a CUDA bool tensor (k, n).
  psi_m = (neighbour sum) / N_i from ctx.bond_order_frames_device with the cutoff r_cut_psi, 0 where N_i = 0."""
  import torch
  out = ctx.bond_order_frames_device(frames, periodic_length, float(r_cut_psi), (int(order),), plane=plane)
  N = out[:, :, 0]
  safe = torch.where(N > 0, N, torch.ones_like(N))
  re, im = out[:, :, 1] / safe, out[:, :, 2] / safe
  return (N > 0) & (torch.sqrt(re * re + im * im) >= float(threshold))


class Clusters(ContextHolder):
  """Accumulates the cluster statistics of a trajectory of n_points points in the box periodic_length (<= 0: open direction) for
  the bond length r_cut.  add_frames(frames, select=None) takes frames (k, n_points, 3), numpy or CUDA float64 tensor, and an
  optional selection (k, n_points) (bool or uint8, numpy or CUDA), in any number of pieces; finish() ends the trajectory.
  n_selected(), n_clusters(), largest(), largest_fraction(), sum_squares(), size_distribution(), mean_size(),
  weight_mean_size(), labels_last(), format(), write(path).  ctx: a single-GPU MobilityContext (its resident configuration is
  left alone); None makes one on `device`, closed by close()."""
  entry, what = "cluster_labels_frames_device", "the cluster analysis runs"

  def __init__(self, n_points, periodic_length, r_cut, plane="xyz", device=0, ctx=None):
    self.n = self.n_points = int(n_points)
    self.n_frames, self._finished = 0, False
    if self.n < 0:
      raise ValueError("n_points must not be negative")
    if self.n > MAX_POINTS_PER_CALL:
      raise ValueError("n_points must not exceed 2^31 - 1, got %r" % (n_points,))
    if plane not in PLANES:
      raise ValueError("plane must be one of %s, got %r" % (PLANES, plane))
    self.plane = plane
    self.periodic_length = _lengths(periodic_length)
    if r_cut is None or not (float(r_cut) > 0.0 and np.isfinite(float(r_cut))):
      raise ValueError("r_cut must be positive and finite, got %r" % (r_cut,))
    self.r_cut = float(r_cut)
    self._open(device, ctx)
    self._per_frame = []      # int64 arrays (k, 4): n_selected, n_clusters, largest, sum of s^2
    self._n_s = np.zeros(self.n + 1, dtype=np.int64)
    self._labels_last = None

  def _per(self):
    """frames per call: the upload piece, and below 2^31 entries of the parent array"""
    return max(1, min(UPLOAD_BYTES // (8 * max(3 * self.n, 1)), MAX_POINTS_PER_CALL // max(self.n, 1)))

  def add_frames(self, frames, select=None):
    if self._finished:
      raise ValueError("add_frames() after finish()")
    torch = self._torch
    on_device = isinstance(frames, torch.Tensor)
    if on_device and not (frames.is_cuda and frames.dtype == torch.float64):
      raise ValueError("frames must be a numpy array or a CUDA float64 tensor")
    f = frames if on_device else np.ascontiguousarray(frames, dtype=np.float64)
    size, row = (f.numel() if on_device else f.size), 3 * self.n
    if row == 0 or size % row:
      raise ValueError("frames must hold whole frames of %s, got shape %r" % ("%d points x 3 coordinates" % self.n, tuple(f.shape)))
    f = f.reshape(-1, self.n, 3)
    s = None
    if select is not None:
      sel_dev = isinstance(select, torch.Tensor)
      s = select if sel_dev else np.ascontiguousarray(select)
      kind_ok = (s.dtype in (torch.bool, torch.uint8) and s.is_cuda) if sel_dev else (s.dtype == np.bool_ or s.dtype == np.uint8)
      if not kind_ok or (s.numel() if sel_dev else s.size) != f.shape[0] * self.n:
        raise ValueError("select must hold one bool or uint8 per point of every frame (numpy or CUDA), got %r of shape %r" %
                         (s.dtype, tuple(s.shape)))
      s = s.reshape(-1, self.n)
    per = self._per()
    for k in range(0, f.shape[0], per):
      piece, sel = f[k:k + per], None if s is None else s[k:k + per]
      if not on_device:      # torch refuses a read-only array
        piece = torch.from_numpy(piece if piece.flags.writeable else piece.copy()).to(self._dev)
      if sel is not None and not isinstance(sel, torch.Tensor):
        sel = torch.from_numpy(sel.astype(np.uint8)).to(self._dev)
      self._add_device(piece.contiguous(), None if sel is None else sel.contiguous())
    return self

  def _add_device(self, piece, sel=None):
    torch = self._torch
    k = int(piece.shape[0])
    with torch.cuda.device(self._dev):
      labels, sizes = self.ctx.cluster_labels_frames_device(piece, self.periodic_length, self.r_cut, plane=self.plane, select=sel)
      s64 = sizes.to(torch.int64)
      stats = torch.stack([torch.count_nonzero(labels >= 0, dim=1), torch.count_nonzero(sizes > 0, dim=1),
                           s64.amax(dim=1), (s64 * s64).sum(dim=1)], dim=1)
      n_s = torch.bincount(s64.reshape(-1), minlength=self.n + 1)
      self._per_frame.append(stats.cpu().numpy().astype(np.int64))
      n_s = n_s.cpu().numpy().astype(np.int64)
      n_s[0] = 0      # the entries of `sizes` that are nobody's label
      self._n_s += n_s
      if k:
        self._labels_last = labels[-1].clone()
    self.n_frames += k

  def finish(self):
    self._finished = True
    return self

  # ---- results -----------------------------------------------------------------------------------------------------
  def _stats(self):
    return np.concatenate(self._per_frame) if self._per_frame else np.zeros((0, 4), dtype=np.int64)

  def n_selected(self):
    """int64 (n_frames,): selected points per frame (all points without a selection)"""
    return self._stats()[:, 0].copy()

  def n_clusters(self):
    """int64 (n_frames,): clusters per frame, singletons included"""
    return self._stats()[:, 1].copy()

  def largest(self):
    """int64 (n_frames,): size of the largest cluster of every frame (0 where nothing is selected)"""
    return self._stats()[:, 2].copy()

  def sum_squares(self):
    """int64 (n_frames,): sum of s^2 over the clusters of every frame"""
    return self._stats()[:, 3].copy()

  def largest_fraction(self):
    """largest / n_selected per frame (nan where nothing is selected)"""
    st = self._stats()
    with np.errstate(divide="ignore", invalid="ignore"):
      return st[:, 2].astype(np.float64) / st[:, 0].astype(np.float64)

  def size_distribution(self):
    """int64 (n_points + 1,): entry s is the number of clusters of size s over all frames"""
    return self._n_s.copy()

  def mean_size(self):
    """the number average sum s n_s / sum n_s over all frames"""
    return number_mean(self._n_s)

  def weight_mean_size(self):
    """the weight average sum s^2 n_s / sum s n_s over all frames"""
    return weight_mean(self._n_s)

  def labels_last(self):
    """labels of the last frame: int32 (n_points,), -1 = unselected"""
    if self._labels_last is None:
      raise ValueError("no frame has been added")
    return self._labels_last.cpu().numpy()

  def format(self):
    """The command line's output: `frame n_selected n_clusters largest mean_size weight_mean_size` per frame (the two means of
    that frame alone, nan where it has no cluster, 17 significant digits), then `s n_s` for every s with n_s > 0."""
    st = self._stats()
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
      mean = st[:, 0].astype(np.float64) / st[:, 1].astype(np.float64)
      wmean = st[:, 3].astype(np.float64) / st[:, 0].astype(np.float64)
    for f in range(st.shape[0]):
      out.append("%d %d %d %d %.17g %.17g\n" % (f, st[f, 0], st[f, 1], st[f, 2], mean[f], wmean[f]))
    out.extend("%d %d\n" % (s, self._n_s[s]) for s in np.nonzero(self._n_s)[0])
    return "".join(out)

  def write(self, path):
    with open(path, "w") as f:
      f.write(self.format())


def parse_args(argv=None):
  """The command line's arguments, checked: (args, psi) with psi = None or (order, threshold, r_cut_psi)."""
  ap = argparse.ArgumentParser(prog="python -m rigidmultiblobswall_amd.clusters", description=__doc__.split("\n\n")[0])
  ap.add_argument("file", help="trajectory in the .config format")
  ap.add_argument("np", type=int, help="number of bodies per frame")
  ap.add_argument("lx", type=float)
  ap.add_argument("ly", type=float)
  ap.add_argument("lz", type=float)
  ap.add_argument("--rcut", type=float, required=True, help="bond length: points closer than this are bonded")
  ap.add_argument("--plane", choices=PLANES, default="xyz")
  ap.add_argument("--every", type=int, default=1, help="use every K-th frame")
  ap.add_argument("--skip", type=int, default=0, help="leave out the first S frames")
  ap.add_argument("--psi", default=None, metavar="M,THRESH,RCUT_PSI",
                  help="select the points with |psi_M| >= THRESH, psi_M over the neighbours within RCUT_PSI")
  ap.add_argument("--device", type=int, default=0)
  args = ap.parse_args(argv)
  if args.every < 1 or args.skip < 0 or args.np < 0:
    ap.error("--every must be at least 1; --skip and np must not be negative")
  if not (args.rcut > 0.0 and np.isfinite(args.rcut)):
    ap.error("--rcut must be positive and finite, got %r" % (args.rcut,))
  psi = None
  if args.psi is not None:
    tok = args.psi.split(",")
    try:
      psi = (int(tok[0]), float(tok[1]), float(tok[2]))
    except (ValueError, IndexError):
      psi = None
    if psi is None or len(tok) != 3 or not 1 <= psi[0] <= 16 or not np.isfinite(psi[1]) or not (psi[2] > 0.0 and np.isfinite(psi[2])):
      ap.error("--psi must be M,THRESH,RCUT_PSI with an order 1 ... 16, a finite threshold and a positive cutoff, got %r" % (args.psi,))
  return args, psi


def main(argv=None, out=None):
  from .correlation import load_trajectory
  args, psi = parse_args(argv)
  L = (args.lx, args.ly, args.lz)
  try:
    frames = load_trajectory(args.file, args.np, args.skip)[::args.every]
    acc = Clusters(args.np, L, args.rcut, plane=args.plane, device=args.device)
  except ValueError as exc:
    print("clusters: %s" % exc, file=sys.stderr)
    return 2
  try:
    import torch
    per = acc._per()
    for k in range(0, frames.shape[0], per):
      piece = torch.from_numpy(np.ascontiguousarray(frames[k:k + per])).to(acc._dev)
      with torch.cuda.device(acc._dev):
        sel = None if psi is None else psi_select(acc.ctx, piece, L, psi[0], psi[1], psi[2], plane=args.plane)
      acc.add_frames(piece, sel)
    acc.finish()
    (out or sys.stdout).write(acc.format())
  finally:
    acc.close()
  return 0


if __name__ == "__main__":
  sys.exit(main())
