"""6 x 6 translational-rotational mean-square displacement (MSD) of rigid-body trajectories on MI355X.

    python -m rigidmultiblobswall_amd.msd run.config n_bodies dt [--lags L] [--every K] [--skip S] [--origins window|all]
                                          [--offset x,y,z] [--device N]

prints one line per lag: `t n` and the 21 entries of the upper triangle of the averaged 6 x 6 matrix, row by row.

The definition is the reference's (general_application_utils.py: calc_total_msd_from_matrix_and_center): for a body with
location x, orientation q (scalar part first) and body-frame tracking offset p, the tracked point is c = x + R(q) p and the
displacement from origin frame o over a lag of l frames is

    Delta = [ c(o + l) - c(o) ;  u ],    u = 1/2 sum_i (R(q(o)) e_i) x (R(q(o + l)) e_i),

MSD[l] = < Delta Delta^T > over origins and bodies.  A body-frame offset covers the reference's calc_center_functions
(cross point, centre of hydrodynamic stress, tip).  Quaternions are used as they are and never renormalised.

The sums come from the HIP lag sweep (rmb_msd_frames_device: a lane owns a lag); there is no CPU fall-back.  Two origin
conventions: "window" (the reference's: only origins for which all n_lags lags exist, every lag has the same number of
terms) and "all" (lag l uses every origin o with o + l < n_frames).  reference_msd() adds the reference's own frame
selection and divisor around the same kernel.
"""
import argparse
import sys

import numpy as np

ORIGINS = ("window", "all")
UPLOAD_BYTES = 64 << 20       # frames go to the device in pieces of at most this many bytes (and at least n_lags frames)
TRIU = np.triu_indices(6)


def counts_per_lag(n_frames, n_bodies, n_lags, origins="window"):
  """Number of terms of every lag's sum, int64 (n_lags,): bodies x origins of the convention `origins`."""
  n_frames, n_bodies, n_lags = int(n_frames), int(n_bodies), int(n_lags)
  if n_lags < 1:
    raise ValueError("n_lags must be at least 1, got %r" % (n_lags,))
  if origins not in ORIGINS:
    raise ValueError("origins must be one of %s, got %r" % (ORIGINS, origins))
  if n_frames < 0 or n_bodies < 0:
    raise ValueError("n_frames and n_bodies must not be negative")
  if origins == "window":
    return np.full(n_lags, n_bodies * max(n_frames - n_lags + 1, 0), dtype=np.int64)
  return n_bodies * np.maximum(n_frames - np.arange(n_lags, dtype=np.int64), 0)


def reference_selection(n_steps, dt, end, burn_in=0, trajectory_length=100):
  """The reference's frame selection (calc_msd_data_from_trajectory): (kept, data_interval, origins, divisor).  kept: the
  indices k with k > burn_in and k % data_interval == 0, data_interval = int(end / dt / trajectory_length) + 1; origins: the
  kept-indices 1 .. K - trajectory_length that serve as origins, as range(1, K - trajectory_length + 1) -- the very first
  kept frame never is one; each origin contributes the lags 0 .. trajectory_length - 1; divisor: the float the reference
  divides the sums by, n_steps / data_interval - trajectory_length - burn_in / data_interval."""
  n_steps, trajectory_length = int(n_steps), int(trajectory_length)
  if trajectory_length < 1:
    raise ValueError("trajectory_length must be at least 1")
  data_interval = int(end / dt / trajectory_length) + 1
  if trajectory_length * data_interval > n_steps:
    raise ValueError("Trajectory length is longer than the total run. Perform a longer run, or choose a shorter end time.")
  k = np.arange(n_steps)
  kept = k[(k > burn_in) & (k % data_interval == 0)]
  origins = range(1, max(len(kept) - trajectory_length, 0) + 1)
  divisor = n_steps / data_interval - trajectory_length - burn_in / data_interval
  return kept, data_interval, origins, divisor


def _offsets(offsets, n_bodies):
  if offsets is None:
    return None
  p = np.asarray(offsets, dtype=np.float64)
  if p.size == 3:
    p = np.tile(p.reshape(1, 3), (n_bodies, 1))
  if p.size != 3 * n_bodies:
    raise ValueError("offsets must hold 3 values or (n_bodies, 3), got shape %r" % (p.shape,))
  return np.ascontiguousarray(p.reshape(n_bodies, 3))


class MeanSquareDisplacement(object):
  """Accumulates the MSD sums of a trajectory of n_bodies rigid bodies over n_lags lags (lag l = l frames = l dt).
  add_frames(frames) takes frames (k, n_bodies, 7) -- rows x y z s p1 p2 p3, numpy or CUDA float64 tensor -- in any
  number of pieces; only the frames of origins whose lags are not complete yet (at most n_lags - 1) stay on the device
  between calls, so a trajectory may be larger than device memory.  finish() ends the trajectory: with origins="all" it adds
  the origins whose later lags do not exist; with "window" nothing is left to add.  sums() (n_lags, 6, 6), counts()
  (n_lags,), msd() = sums / counts (nan where a lag has no term), times() = dt * lag, write(path).  offsets: body-frame
  tracking offsets, 3 values for all bodies or (n_bodies, 3).  Quaternions are used as they are, never renormalised.  ctx:
  a single-GPU MobilityContext (its resident configuration is left alone); None makes one on `device`, closed by close()."""

  def __init__(self, n_bodies, n_lags, dt=1.0, origins="window", offsets=None, device=0, ctx=None):
    self.n_bodies, self.n_lags, self.dt = int(n_bodies), int(n_lags), float(dt)
    if self.n_bodies < 0:
      raise ValueError("n_bodies must not be negative")
    counts_per_lag(0, self.n_bodies, self.n_lags, origins)      # refuses what the kernel entry would
    self.origins = origins
    off = _offsets(offsets, self.n_bodies)
    self.n_frames = 0
    self._finished = False
    self._own_ctx = ctx is None
    if ctx is None:
      from .context import MobilityContext
      ctx = MobilityContext(int(device))
    if not hasattr(ctx, "msd_frames_device"):
      if self._own_ctx:
        ctx.close()
      raise ValueError("the mean-square displacement runs on a single-GPU MobilityContext, got %r" % (type(ctx).__name__,))
    self.ctx = ctx
    import torch
    self._torch = torch
    self._dev = torch.device("cuda", ctx.device)
    self._sums = torch.zeros((self.n_lags, 6, 6), dtype=torch.float64, device=self._dev)
    self._counts = np.zeros(self.n_lags, dtype=np.int64)
    self._offsets = None if off is None else torch.from_numpy(off).to(self._dev)
    self._tail = None      # frames of the origins whose lags are not complete yet

  def close(self):
    if self._own_ctx and self.ctx is not None:
      self.ctx.close()
    self.ctx = None

  def _call(self, frames, origins):
    with self._torch.cuda.device(self._dev):
      _, n = self.ctx.msd_frames_device(frames, self.n_lags, offsets=self._offsets, origins=origins, out=self._sums)
    self._counts += n

  def _add_device(self, piece):
    """piece: CUDA float64 tensor (k, n_bodies, 7)"""
    torch = self._torch
    buf = piece.contiguous() if self._tail is None else torch.cat([self._tail, piece])
    complete = buf.shape[0] - self.n_lags + 1      # origins of the buffer that have every lag
    if complete > 0:
      self._call(buf, "window")
      buf = buf[complete:].clone()
    self._tail = buf if buf.shape[0] else None
    self.n_frames += int(piece.shape[0])

  def add_frames(self, frames):
    if self._finished:
      raise ValueError("add_frames() after finish()")
    torch = self._torch
    row = 7 * self.n_bodies
    per = max(self.n_lags, UPLOAD_BYTES // (8 * max(row, 1)))
    if isinstance(frames, torch.Tensor):
      if not (frames.is_cuda and frames.dtype == torch.float64):
        raise ValueError("frames must be a numpy array or a CUDA float64 tensor")
      if row == 0 or frames.numel() % row:
        raise ValueError("frames must hold whole frames of %d bodies x 7 numbers, got shape %r" % (self.n_bodies, tuple(frames.shape)))
      f = frames.reshape(-1, self.n_bodies, 7)
      for k in range(0, f.shape[0], per):
        self._add_device(f[k:k + per])
      return self
    f = np.ascontiguousarray(frames, dtype=np.float64)
    if row == 0 or f.size % row:
      raise ValueError("frames must hold whole frames of %d bodies x 7 numbers, got shape %r" % (self.n_bodies, f.shape))
    f = f.reshape(-1, self.n_bodies, 7)
    for k in range(0, f.shape[0], per):
      piece = f[k:k + per]
      self._add_device(torch.from_numpy(piece if piece.flags.writeable else piece.copy()).to(self._dev))
    return self

  def finish(self):
    """End of the trajectory.  origins="all": the frames still held are origins of the lags that exist for them."""
    if not self._finished:
      if self.origins == "all" and self._tail is not None:
        self._call(self._tail, "all")
      self._tail = None
      self._finished = True
    return self

  def sums(self):
    return self._sums.cpu().numpy()

  def counts(self):
    return self._counts.copy()

  def times(self):
    return self.dt * np.arange(self.n_lags)

  def msd(self):
    with np.errstate(divide="ignore", invalid="ignore"):
      return self.sums() / self._counts.astype(np.float64)[:, None, None]

  def write(self, path):
    """`t n` and the 21 upper-triangle entries per lag (format_msd)."""
    with open(path, "w") as f:
      f.write(format_msd(self.times(), self.counts(), self.msd()))


def format_msd(times, counts, msd):
  """One line per lag: t, the number of terms, and the upper triangle of the 6 x 6 matrix row by row (21 numbers), every
  float with 17 significant digits."""
  return "".join("%.17g %d %s\n" % (t, n, " ".join("%.17g" % v for v in m[TRIU])) for t, n, m in zip(times, counts, msd))


def reference_msd(locations, orientations, dt, end, burn_in=0, trajectory_length=100, offset=None, device=0, ctx=None):
  """The reference's calc_msd_data_from_trajectory for one body: locations (n_steps, 3), orientations (n_steps, 4) with the
  scalar part first (used as they are, never renormalised), offset: the body-frame point R(q) offset is added to the location
  (a calc_center_function; None: the location itself).  Frame selection and divisor are the reference's
  (reference_selection); the sums are the kernel's.  Returns (trajectory_length, 6, 6)."""
  loc = np.asarray(locations, dtype=np.float64).reshape(-1, 3)
  quat = np.asarray(orientations, dtype=np.float64).reshape(-1, 4)
  if loc.shape[0] != quat.shape[0]:
    raise ValueError("locations and orientations must have one row per step each")
  kept, _, origins, divisor = reference_selection(loc.shape[0], dt, end, burn_in, trajectory_length)
  # the first kept frame is never an origin, and no origin reaches back to it: window origins of the rest are the reference's
  frames = np.concatenate([loc[kept[1:]], quat[kept[1:]]], axis=1).reshape(-1, 1, 7)
  acc = MeanSquareDisplacement(1, trajectory_length, dt=dt, origins="window", offsets=offset, device=device, ctx=ctx)
  try:
    acc.add_frames(frames).finish()
    assert acc.counts()[0] == len(origins)
    return acc.sums() / divisor
  finally:
    acc.close()


def load_trajectory(path_or_paths, n_bodies, skip=0):
  """Frames of a `.config` trajectory as (n_frames, n_bodies, 7): one count line, then `x y z s p1 p2 p3` per body, repeated
  for every saved step; or a list of such files.  The first `skip` frames are left out."""
  if int(skip) < 0:
    raise ValueError("skip must not be negative, got %r" % (skip,))
  paths = [path_or_paths] if isinstance(path_or_paths, (str, bytes)) or hasattr(path_or_paths, "__fspath__") else list(path_or_paths)
  n_bodies = int(n_bodies)
  if n_bodies < 1:
    raise ValueError("n_bodies must be at least 1")
  block = 1 + 7 * n_bodies
  out = []
  for path in paths:
    with open(path) as f:
      tok = np.array(f.read().split(), dtype=np.float64)
    if tok.size % block:
      raise ValueError("%s: %d numbers are not a whole number of frames of %d bodies (1 + 7 * %d numbers each)" % (path, tok.size, n_bodies, n_bodies))
    tok = tok.reshape(-1, block)
    if tok.size and np.any(tok[:, 0] != n_bodies):
      raise ValueError("%s: a frame announces %d bodies, expected %d" % (path, int(tok[tok[:, 0] != n_bodies][0, 0]), n_bodies))
    out.append(tok[:, 1:].reshape(-1, n_bodies, 7))
  frames = np.ascontiguousarray(np.concatenate(out)) if out else np.zeros((0, n_bodies, 7))
  frames = frames[int(skip):]
  if frames.shape[0] < 1:
    raise ValueError("no frame left after skipping %d" % int(skip))
  return frames


def main(argv=None, out=None):
  ap = argparse.ArgumentParser(prog="python -m rigidmultiblobswall_amd.msd", description=__doc__.split("\n\n")[0])
  ap.add_argument("file", help="trajectory in the .config format")
  ap.add_argument("n_bodies", type=int, help="number of bodies per frame")
  ap.add_argument("dt", type=float, help="time between saved frames")
  ap.add_argument("--lags", type=int, default=100, help="number of lags, 0 .. L - 1 (at most the number of frames used)")
  ap.add_argument("--every", type=int, default=1, help="use every K-th frame (a lag is then K dt)")
  ap.add_argument("--skip", type=int, default=0, help="leave out the first S frames")
  ap.add_argument("--origins", choices=ORIGINS, default="window")
  ap.add_argument("--offset", default=None, help="body-frame tracking offset x,y,z of every body")
  ap.add_argument("--device", type=int, default=0)
  args = ap.parse_args(argv)
  if args.every < 1 or args.lags < 1:
    ap.error("--every and --lags must be at least 1")
  offset = None
  if args.offset is not None:
    try:
      offset = [float(v) for v in args.offset.split(",")]
    except ValueError:
      offset = []
    if len(offset) != 3:
      ap.error("--offset takes three numbers x,y,z")
  try:
    frames = load_trajectory(args.file, args.n_bodies, args.skip)[::args.every]
  except ValueError as exc:
    ap.error(str(exc))
  acc = MeanSquareDisplacement(args.n_bodies, min(args.lags, frames.shape[0]), dt=args.dt * args.every, origins=args.origins, offsets=offset,
                               device=args.device)
  try:
    acc.add_frames(frames).finish()
    (out or sys.stdout).write(format_msd(acc.times(), acc.counts(), acc.msd()))
  finally:
    acc.close()
  return 0


if __name__ == "__main__":
  sys.exit(main())
