"""Radial distribution function g(r) of point configurations -- multi_bodies/examples/Radial_Dist_Test on MI355X.

    python -m rigidmultiblobswall_amd.correlation file np lx ly lz [--bins 2000] [--rmax R] [--skip K]
                                                  [--normalisation pseudo2d|3d] [--device N]

The positional arguments are the reference program's (gr_pseudo2D_single_blob.cpp: a `.config` trajectory, the number of
bodies, the box), the output its three columns `r g hist`: bin centre, g, and the number of ORDERED pairs in the bin (the
reference adds 2 per pair i < j; everything in this package counts unordered pairs and doubles on output).

The counts come from the HIP pair-distance histogram (rmb_pair_histogram*): every unordered pair once, fp64, minimal image in
every direction with a positive period.  The reference program images x and y only; for its quasi-2D use (lz = 0, or a
layer much thinner than lz / 2) the two agree.  There is no CPU fall-back.

Normalisations:
  pseudo2d  the reference program's: distances in 3D, ideal-gas count of a 2D system,
            g = 2 counts / (n_frames N pi rho_2D (r_up^2 - r_low^2)),  rho_2D = N / (lx ly)
  3d        shell volumes: g = 2 counts / (n_frames N rho (4/3) pi (r_up^3 - r_low^3)),  rho = N / (lx ly lz); needs three
            positive periods
"""
import argparse
import sys

import numpy as np

NORMALISATIONS = ("pseudo2d", "3d")
BATCH_MAX_TILES = 32          # below: the batch entry (frames of few points); from here on: the resident, sorted and culled sweep
UPLOAD_BYTES = 64 << 20       # frames go to the device in chunks of at most this many bytes


def bin_edges(r_max, n_bins):
  dr = float(r_max) / int(n_bins)
  return dr * np.arange(int(n_bins) + 1)


def normalise(counts, n_frames, n_points, periodic_length, r_max, normalisation="pseudo2d"):
  """g per bin from the counts of unordered pairs summed over n_frames frames of n_points points."""
  if normalisation not in NORMALISATIONS:
    raise ValueError("normalisation must be one of %s, got %r" % (NORMALISATIONS, normalisation))
  L = np.asarray(periodic_length, dtype=np.float64).reshape(3)
  counts = np.asarray(counts, dtype=np.float64)
  e = bin_edges(r_max, counts.size)
  if normalisation == "pseudo2d":
    if not (L[0] > 0 and L[1] > 0):
      raise ValueError("normalisation 'pseudo2d' needs positive lx and ly, got %r" % (tuple(L),))
    ideal = np.pi * (n_points / (L[0] * L[1])) * (e[1:] ** 2 - e[:-1] ** 2)
  else:
    if not np.all(L > 0):
      raise ValueError("normalisation '3d' needs three positive periods, got %r" % (tuple(L),))
    ideal = 4.0 / 3.0 * np.pi * (n_points / (L[0] * L[1] * L[2])) * (e[1:] ** 3 - e[:-1] ** 3)
  with np.errstate(divide="ignore", invalid="ignore"):
    return 2.0 * counts / (float(n_frames) * n_points * ideal)


def format_gr(r, g, counts):
  """The reference program's three columns, one line per bin: r and g with %g (the program's six significant digits), the
  third -- 2 x the unordered count, an integer there too -- in full."""
  return "".join("%g %g %d\n" % (ri, gi, 2 * int(ci)) for ri, gi, ci in zip(r, g, counts))


def read_frames(path_or_paths, n_points, columns=3):
  """Frames of a trajectory as (n_frames, n_points, 3): a `.config` file (one count line, then `x y z q0 q1 q2 q3` per body,
  repeated for every saved step; a final newline or none), or a list of such files -- e.g. one `.clones` file per step.
  columns=7 keeps the quaternions too."""
  paths = [path_or_paths] if isinstance(path_or_paths, (str, bytes)) or hasattr(path_or_paths, "__fspath__") else list(path_or_paths)
  n_points = int(n_points)
  if n_points < 0:
    raise ValueError("n_points must not be negative")
  block = 1 + 7 * n_points
  out = []
  for path in paths:
    with open(path) as f:
      tok = np.array(f.read().split(), dtype=np.float64)
    if tok.size % block:
      raise ValueError("%s: %d numbers are not a whole number of frames of %d bodies (1 + 7 * %d numbers each)" % (path, tok.size, n_points, n_points))
    tok = tok.reshape(-1, block)
    if tok.size and np.any(tok[:, 0] != n_points):
      raise ValueError("%s: a frame announces %d bodies, expected %d" % (path, int(tok[tok[:, 0] != n_points][0, 0]), n_points))
    out.append(tok[:, 1:].reshape(-1, n_points, 7)[:, :, :columns])
  return np.ascontiguousarray(np.concatenate(out)) if out else np.zeros((0, n_points, columns))


def load_trajectory(path_or_paths, n_points, skip=0, columns=3):
  """read_frames without the first `skip` frames (the reference program's `skip`: they are neither counted nor normalised by)."""
  if int(skip) < 0:
    raise ValueError("skip must not be negative, got %r" % (skip,))
  frames = read_frames(path_or_paths, n_points, columns)[int(skip):]
  if frames.shape[0] < 1:
    raise ValueError("no frame left after skipping %d" % int(skip))
  return frames


class RadialDistribution(object):
  """Accumulates the pair-distance histogram of frames of n_points points in a box periodic_length (<= 0: open direction)
  and turns it into g(r).  r_max=None is lx / 2, as in the reference program.  add(frame) / add_frames(frames) take numpy
  arrays or CUDA float64 tensors; counts (numpy uint64, unordered pairs), n_frames, r (bin centres), g().  ctx: a
  MobilityContext to run on (its resident configuration is replaced for frames of 2048 points or more); None makes one on
  `device`, closed by close()."""

  def __init__(self, n_points, periodic_length, r_max=None, n_bins=2000, normalisation="pseudo2d", device=0, ctx=None):
    self.n_points = int(n_points)
    self.periodic_length = np.asarray(periodic_length, dtype=np.float64).reshape(3).copy()
    if r_max is None:
      r_max = 0.5 * self.periodic_length[0]
    self.r_max, self.n_bins = float(r_max), int(n_bins)
    if not self.r_max > 0.0:
      raise ValueError("r_max must be positive (r_max=None needs a positive lx), got %r" % (self.r_max,))
    if not 1 <= self.n_bins <= 8192:
      raise ValueError("n_bins must be 1 ... 8192, got %r" % (n_bins,))
    if self.n_points < 0:
      raise ValueError("n_points must not be negative")
    self.normalisation = normalisation
    normalise(np.zeros(1), 1, max(self.n_points, 1), self.periodic_length, self.r_max, normalisation)      # refuses what g() would
    self.n_frames = 0
    self._own_ctx = ctx is None
    if ctx is None:
      from .context import MobilityContext
      ctx = MobilityContext(int(device))
    if not hasattr(ctx, "pair_histogram_frames_device"):
      raise ValueError("the pair histogram runs on a single-GPU MobilityContext, got %r" % (type(ctx).__name__,))
    self.ctx = ctx
    import torch
    self._torch = torch
    self._dev = torch.device("cuda", ctx.device)
    self._hist = torch.zeros(self.n_bins, dtype=torch.int64, device=self._dev)

  def close(self):
    if self._own_ctx and self.ctx is not None:
      self.ctx.close()
    self.ctx = None

  @property
  def batch(self):
    """Whether frames go through the batch entry (fewer than 32 tiles of 64 points) or become the resident configuration."""
    return (self.n_points + 63) // 64 < BATCH_MAX_TILES

  def _add_device(self, frames):
    """frames: contiguous CUDA float64 tensor (k, n_points, 3)"""
    with self._torch.cuda.device(self._dev):
      if self.batch:
        self.ctx.pair_histogram_frames_device(frames, self.periodic_length, self.r_max, self.n_bins, out=self._hist)
      else:
        for k in range(frames.shape[0]):
          self.ctx.set_positions(frames[k], 1.0, self.periodic_length, wall=False)
          self.ctx.pair_histogram_device(self.r_max, self.n_bins, out=self._hist)
    self.n_frames += int(frames.shape[0])

  def add_frames(self, frames):
    torch = self._torch
    if isinstance(frames, torch.Tensor):
      if not (frames.is_cuda and frames.dtype == torch.float64):
        raise ValueError("frames must be a numpy array or a CUDA float64 tensor")
      f = frames.reshape(-1, self.n_points, 3).contiguous() if self.n_points else frames.reshape(-1, 0, 3)
      self._add_device(f)
      return self
    f = np.ascontiguousarray(frames, dtype=np.float64)
    if self.n_points == 0:
      self.n_frames += int(f.shape[0]) if f.ndim == 3 else 0
      return self
    if f.size % (3 * self.n_points):
      raise ValueError("frames must hold whole frames of %d points x 3 coordinates, got shape %r" % (self.n_points, f.shape))
    f = f.reshape(-1, self.n_points, 3)
    per = max(1, UPLOAD_BYTES // (24 * self.n_points))
    for k in range(0, f.shape[0], per):
      self._add_device(torch.from_numpy(f[k:k + per]).to(self._dev))
    return self

  def add(self, frame):
    torch = self._torch
    n = frame.numel() if isinstance(frame, torch.Tensor) else np.asarray(frame).size
    if n != 3 * self.n_points:
      raise ValueError("a frame holds %d points x 3 coordinates, got %d numbers" % (self.n_points, n))
    if self.n_points == 0:
      self.n_frames += 1
      return self
    return self.add_frames(frame.reshape(1, self.n_points, 3) if isinstance(frame, torch.Tensor) else np.asarray(frame).reshape(1, self.n_points, 3))

  @property
  def counts(self):
    return self._hist.cpu().numpy().astype(np.uint64)

  @property
  def r(self):
    return (np.arange(self.n_bins) + 0.5) * (self.r_max / self.n_bins)

  def g(self):
    if self.n_frames < 1:
      raise ValueError("g(): no frame was added")
    return normalise(self.counts, self.n_frames, self.n_points, self.periodic_length, self.r_max, self.normalisation)

  def write(self, path):
    """`r g hist` in the reference program's format (hist = ordered pairs)."""
    with open(path, "w") as f:
      f.write(format_gr(self.r, self.g(), self.counts))


def main(argv=None, out=None):
  ap = argparse.ArgumentParser(prog="python -m rigidmultiblobswall_amd.correlation", description=__doc__.split("\n\n")[0])
  ap.add_argument("file", help="trajectory in the .config format")
  ap.add_argument("np", type=int, help="number of bodies per frame")
  ap.add_argument("lx", type=float)
  ap.add_argument("ly", type=float)
  ap.add_argument("lz", type=float)
  ap.add_argument("--bins", type=int, default=2000)
  ap.add_argument("--rmax", type=float, default=None, help="default lx / 2")
  ap.add_argument("--skip", type=int, default=0, help="leave out the first K frames")
  ap.add_argument("--normalisation", choices=NORMALISATIONS, default="pseudo2d")
  ap.add_argument("--device", type=int, default=0)
  args = ap.parse_args(argv)
  try:
    frames = load_trajectory(args.file, args.np, args.skip)
  except ValueError as exc:
    ap.error(str(exc))
  rd = RadialDistribution(args.np, (args.lx, args.ly, args.lz), r_max=args.rmax, n_bins=args.bins, normalisation=args.normalisation,
                          device=args.device)
  try:
    rd.add_frames(frames)
    (out or sys.stdout).write(format_gr(rd.r, rd.g(), rd.counts))
  finally:
    rd.close()
  return 0


if __name__ == "__main__":
  sys.exit(main())
