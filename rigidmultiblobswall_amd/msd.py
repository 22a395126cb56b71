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

from ._lagged import ORIGINS, LagAccumulator, counts_per_lag      # ORIGINS and counts_per_lag are this module's names too

TRIU = np.triu_indices(6)


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


class MeanSquareDisplacement(LagAccumulator):
  """Accumulates the MSD sums of a trajectory of n_bodies rigid bodies over n_lags lags (lag l = l frames = l dt).
  add_frames(frames) takes frames (k, n_bodies, 7) -- rows x y z s p1 p2 p3, numpy or CUDA float64 tensor -- in any
  number of pieces; only the frames of origins whose lags are not complete yet (at most n_lags - 1) stay on the device
  between calls, so a trajectory may be larger than device memory.  finish() ends the trajectory: with origins="all" it adds
  the origins whose later lags do not exist; with "window" nothing is left to add.  sums() (n_lags, 6, 6), counts()
  (n_lags,), msd() = sums / counts (nan where a lag has no term), times() = dt * lag, write(path).  offsets: body-frame
  tracking offsets, 3 values for all bodies or (n_bodies, 3).  Quaternions are used as they are, never renormalised.  ctx:
  a single-GPU MobilityContext (its resident configuration is left alone); None makes one on `device`, closed by close()."""
  width, entry = 7, "msd_frames_device"
  what, row = "the mean-square displacement runs", ("n_bodies", "%d bodies x 7 numbers")

  def __init__(self, n_bodies, n_lags, dt=1.0, origins="window", offsets=None, device=0, ctx=None):
    LagAccumulator.__init__(self, n_bodies, n_lags, dt, origins)
    self.n_bodies = self.n
    off = _offsets(offsets, self.n_bodies)
    self._open(device, ctx)
    torch = self._torch
    self._sums = torch.zeros((self.n_lags, 6, 6), dtype=torch.float64, device=self._dev)
    self._counts = np.zeros(self.n_lags, dtype=np.int64)
    self._offsets = None if off is None else torch.from_numpy(off).to(self._dev)

  def _call(self, records, origins):
    with self._torch.cuda.device(self._dev):
      _, n = self.ctx.msd_frames_device(records[0], self.n_lags, offsets=self._offsets, origins=origins, out=self._sums)
    self._counts += n

  def sums(self):
    return self._sums.cpu().numpy()

  def counts(self):
    return self._counts.copy()

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
  for every saved step; or a list of such files.  The first `skip` frames are left out.  (correlation.load_trajectory with all
  seven columns.)"""
  from .correlation import load_trajectory as load
  if int(n_bodies) < 1:
    raise ValueError("n_bodies must be at least 1")
  return load(path_or_paths, n_bodies, skip, columns=7)


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
