"""Van Hove correlation functions G_s(r, t) and G_d(r, t) of point trajectories on MI355X.

    python -m rigidmultiblobswall_amd.vanhove run.config np lx ly lz --lags L [--dt DT] [--rmax R] [--bins B] [--self-rmax R]
                                              [--self-bins B] [--plane xy|xyz] [--every K] [--skip S] [--origins window|all]
                                              [--no-distinct] [--device N]

The positional arguments are those of rigidmultiblobswall_amd.correlation (a `.config` trajectory, the number of bodies, the
box); the points are the location columns.  It prints one block per lag: a line `# t T n_origins alpha2 msd`, then one line
`r Gs Hs Gd Hd` per bin (without the last two columns under --no-distinct).  Where the self grid (--self-rmax, --self-bins)
differs from the distinct one, the block holds the lines `r Gs Hs` of the self grid, a line `# distinct`, and the lines
`r Gd Hd` of the distinct grid.

With frames x_j(f), origins o and lags l (lag l = l frames = l dt),

    G_s(r, l): the distribution of the displacements |x_j(o + l) - x_j(o)| (as they are: trajectories are unwrapped, as for
               the MSD), normalised so that sum_b G_s shell_b is the fraction of displacements below self_r_max;
    G_d(r, l): the density of points i != j at distance r of where point j was l frames earlier, in units of the mean
               density: the minimal image of x_i(o + l) - x_j(o) in every periodic direction; G_d(r, 0) = g(r);
    msd(l) = < |D|^2 >,   alpha2(l) = d / (d + 2) < |D|^4 > / < |D|^2 >^2 - 1,   d = 3 (xyz) or 2 (xy),

the last two over ALL displacements, whatever self_r_max.  plane="xy" ignores the z component of every separation and
displacement.  F_s(k, t) of rigidmultiblobswall_amd.scattering is the Fourier transform of G_s, F(k, t) - F_s(k, t) that of G_d.

The counts come from the HIP sweeps rmb_van_hove_self_frames_device (a lane owns a point) and
rmb_van_hove_distinct_frames_device (ordered pairs, a workgroup owns a lag): integer counts, the same for every launch plan
and every way of cutting the trajectory into pieces.  There is no CPU fall-back.  Origins "window" and "all" are those of
rigidmultiblobswall_amd.msd.
"""
import argparse
import sys

import numpy as np

from .correlation import normalise
from ._lagged import ORIGINS, LagAccumulator, counts_per_lag, lengths as _lengths

PLANES = ("xy", "xyz")
NORMALISATIONS = ("3d", "2d", "pseudo2d")
MAX_BINS = 8192


def shell_volumes(r_max, n_bins, plane):
  """(4 pi / 3)(up^3 - lo^3) per bin for plane "xyz", pi (up^2 - lo^2) for "xy"."""
  e = (float(r_max) / int(n_bins)) * np.arange(int(n_bins) + 1)
  if plane == "xyz":
    return 4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3)
  return np.pi * (e[1:] ** 2 - e[:-1] ** 2)


def normalise_self(hist, counts, r_max, plane):
  """G_s (n_lags, n_bins) from the self counts and the number of terms per lag; nan where a lag has no term."""
  hist = np.asarray(hist, dtype=np.float64)
  with np.errstate(divide="ignore", invalid="ignore"):
    return hist / (np.asarray(counts, dtype=np.float64)[:, None] * shell_volumes(r_max, hist.shape[1], plane)[None, :])


def normalise_distinct(hist, n_origins, n_points, periodic_length, r_max, normalisation):
  """G_d (n_lags, n_bins) from the counts of ORDERED pairs and the origins per lag: hist / (n_origins N rho shell).  "3d": rho =
  N / (lx ly lz), shells of a sphere; "2d" and "pseudo2d": rho = N / (lx ly), rings -- for distances in the plane and, as
  correlation.normalise(..., "pseudo2d"), for distances in 3-D of a thin layer.  nan where a lag has no origin."""
  if normalisation not in NORMALISATIONS:
    raise ValueError("normalisation must be one of %s, got %r" % (NORMALISATIONS, normalisation))
  hist = np.asarray(hist, dtype=np.float64)
  form = "3d" if normalisation == "3d" else "pseudo2d"
  # half the ordered counts are correlation.py's unordered ones (exact in fp64): the same arithmetic as g(r)
  return np.stack([normalise(0.5 * hist[l], n_origins[l], n_points, periodic_length, r_max, form) for l in range(hist.shape[0])])


def alpha2_from_moments(moments, counts, plane):
  """(msd, alpha2) per lag from M[l] = (sum r^2, sum r^4) over counts[l] terms; nan where a lag has no term, alpha2 also where
  the msd is zero."""
  m = np.asarray(moments, dtype=np.float64)
  c = np.asarray(counts, dtype=np.float64)
  d = 3.0 if plane == "xyz" else 2.0
  with np.errstate(divide="ignore", invalid="ignore"):
    r2, r4 = m[:, 0] / c, m[:, 1] / c
    a2 = d / (d + 2.0) * r4 / (r2 * r2) - 1.0
  return r2, np.where(r2 > 0, a2, np.nan)


class VanHove(LagAccumulator):
  """Accumulates the van Hove counts of a trajectory of n_points points over n_lags lags (lag l = l frames = l dt) in the box
  periodic_length (<= 0: open direction).  Distinct part: n_bins bins up to r_max (None: half the smallest positive period of
  the plane); self part: self_n_bins bins up to self_r_max (None: the distinct values).  add_frames(frames) takes frames
  (k, n_points, 3), numpy or CUDA float64 tensor, in any number of pieces; between calls only the last n_lags - 1 frames stay
  on the device, and every (origin, lag) is counted exactly once however the trajectory is cut.  finish() ends the
  trajectory (origins="all": the frames still held are origins of the lags that exist for them).  n_origins(): origins per
  lag; counts(): terms per lag (msd.counts_per_lag); times(), r(), r_self(); self_counts(), distinct_counts(); Gs(), Gd(),
  msd(), alpha2(); write(path).  distinct=False leaves the O(N^2) part out.  ctx: a single-GPU MobilityContext (its
  resident configuration is left alone); None makes one on `device`, closed by close()."""
  width, entry = 3, "van_hove_self_frames_device"
  what, row = "the van Hove functions run", ("n_points", "%d points x 3 coordinates")

  def __init__(self, n_points, periodic_length, n_lags, dt=1.0, r_max=None, n_bins=1000, self_r_max=None, self_n_bins=None,
               origins="window", plane="xyz", distinct=True, device=0, ctx=None):
    LagAccumulator.__init__(self, n_points, n_lags, dt, origins)
    self.n_points = self.n
    if plane not in PLANES:
      raise ValueError("plane must be one of %s, got %r" % (PLANES, plane))
    self.plane, self.distinct = plane, bool(distinct)
    self.periodic_length = _lengths(periodic_length)
    if r_max is None:
      periods = self.periodic_length[:2 if plane == "xy" else 3]
      if not np.any(periods > 0):
        raise ValueError("r_max=None needs a positive period in the plane, got %r" % (tuple(self.periodic_length),))
      r_max = 0.5 * float(np.min(periods[periods > 0]))
    self.r_max, self.n_bins = float(r_max), int(n_bins)
    self.self_r_max = self.r_max if self_r_max is None else float(self_r_max)
    self.self_n_bins = self.n_bins if self_n_bins is None else int(self_n_bins)
    for name, r, b in (("r_max", self.r_max, self.n_bins), ("self_r_max", self.self_r_max, self.self_n_bins)):
      if not (r > 0.0 and np.isfinite(r)):
        raise ValueError("%s must be positive and finite, got %r" % (name, r))
      if not 1 <= b <= MAX_BINS:
        raise ValueError("the number of bins must be 1 ... %d, got %r" % (MAX_BINS, b))
    self._open(device, ctx)
    torch = self._torch
    self._Hs = torch.zeros((self.n_lags, self.self_n_bins), dtype=torch.int64, device=self._dev)
    self._M = torch.zeros((self.n_lags, 2), dtype=torch.float64, device=self._dev)
    self._Hd = torch.zeros((self.n_lags, self.n_bins), dtype=torch.int64, device=self._dev) if self.distinct else None
    self._origins = np.zeros(self.n_lags, dtype=np.int64)

  def _call(self, records, origins):
    frames, = records
    with self._torch.cuda.device(self._dev):
      self.ctx.van_hove_self_frames_device(frames, self.n_lags, self.self_r_max, self.self_n_bins, origins=origins, plane=self.plane,
                                           out=self._Hs, moments=self._M)
      if self.distinct:
        self.ctx.van_hove_distinct_frames_device(frames, self.periodic_length, self.n_lags, self.r_max, self.n_bins, origins=origins,
                                                 plane=self.plane, out=self._Hd)
    self._origins += counts_per_lag(int(frames.shape[0]), 1, self.n_lags, origins)

  def n_origins(self):
    return self._origins.copy()

  def counts(self):
    return self._origins * self.n_points

  def r(self):
    return (np.arange(self.n_bins) + 0.5) * (self.r_max / self.n_bins)

  def r_self(self):
    return (np.arange(self.self_n_bins) + 0.5) * (self.self_r_max / self.self_n_bins)

  def self_counts(self):
    return self._Hs.cpu().numpy()

  def moments(self):
    return self._M.cpu().numpy()

  def distinct_counts(self):
    if not self.distinct:
      raise ValueError("the distinct part was not asked for (distinct=True)")
    return self._Hd.cpu().numpy()

  def Gs(self):
    return normalise_self(self.self_counts(), self.counts(), self.self_r_max, self.plane)

  def Gd(self, normalisation=None):
    if normalisation is None:
      normalisation = "3d" if self.plane == "xyz" else "2d"
    return normalise_distinct(self.distinct_counts(), self._origins, self.n_points, self.periodic_length, self.r_max, normalisation)

  def msd(self):
    return alpha2_from_moments(self.moments(), self.counts(), self.plane)[0]

  def alpha2(self):
    return alpha2_from_moments(self.moments(), self.counts(), self.plane)[1]

  def format(self, normalisation=None):
    """The command line's output (see the module's docstring); every float with 17 significant digits."""
    d = dict(r=self.r(), Gd=self.Gd(normalisation), Hd=self.distinct_counts()) if self.distinct else {}
    return format_table(self.times(), self._origins, self.alpha2(), self.msd(), self.r_self(), self.Gs(), self.self_counts(), **d)

  def write(self, path, normalisation=None):
    with open(path, "w") as f:
      f.write(self.format(normalisation))


def format_table(times, n_origins, alpha2, msd, r_self, Gs, Hs, r=None, Gd=None, Hd=None):
  """One block per lag: `# t T n_origins alpha2 msd`, then `r Gs Hs Gd Hd` per bin where the two grids are the same one, else
  `r Gs Hs` per self bin, `# distinct`, `r Gd Hd` per distinct bin; without r / Gd / Hd the self lines only."""
  same = r is not None and len(r) == len(r_self) and np.array_equal(r, r_self)
  out = []
  for lag in range(len(times)):
    out.append("# t %.17g %d %.17g %.17g\n" % (times[lag], n_origins[lag], alpha2[lag], msd[lag]))
    if same:
      out.extend("%.17g %.17g %d %.17g %d\n" % (r[b], Gs[lag, b], Hs[lag, b], Gd[lag, b], Hd[lag, b]) for b in range(len(r)))
      continue
    out.extend("%.17g %.17g %d\n" % (r_self[b], Gs[lag, b], Hs[lag, b]) for b in range(len(r_self)))
    if r is not None:
      out.append("# distinct\n")
      out.extend("%.17g %.17g %d\n" % (r[b], Gd[lag, b], Hd[lag, b]) for b in range(len(r)))
  return "".join(out)


def parse(text):
  """What format() wrote, as a list of one dict per lag: t, n_origins, alpha2, msd, r_self, Gs, Hs and, where the distinct
  columns are there, r, Gd, Hd (numpy arrays; the counts int64)."""
  blocks, cur, part = [], None, None
  for line in text.splitlines():
    tok = line.split()
    if not tok:
      continue
    if tok[0] == "#" and len(tok) == 6 and tok[1] == "t":
      cur = {"t": float(tok[2]), "n_origins": int(tok[3]), "alpha2": float(tok[4]), "msd": float(tok[5]), "self": [], "distinct": []}
      blocks.append(cur)
      part = "self"
    elif tok[0] == "#" and tok[1:] == ["distinct"]:
      part = "distinct"
    elif cur is None or tok[0] == "#" or len(tok) not in (3, 5):
      raise ValueError("not a van Hove table: %r" % (line,))
    elif len(tok) == 5:
      cur["self"].append(tok[:3])
      cur["distinct"].append([tok[0]] + tok[3:])
    else:
      cur[part].append(tok)
  out = []
  for b in blocks:
    s = np.array(b.pop("self"), dtype=object).reshape(-1, 3)
    d = np.array(b.pop("distinct"), dtype=object).reshape(-1, 3)
    b.update(r_self=s[:, 0].astype(np.float64), Gs=s[:, 1].astype(np.float64), Hs=np.array([int(x) for x in s[:, 2]], dtype=np.int64))
    if d.shape[0]:
      b.update(r=d[:, 0].astype(np.float64), Gd=d[:, 1].astype(np.float64), Hd=np.array([int(x) for x in d[:, 2]], dtype=np.int64))
    out.append(b)
  return out


def main(argv=None, out=None):
  from .correlation import load_trajectory
  ap = argparse.ArgumentParser(prog="python -m rigidmultiblobswall_amd.vanhove", description=__doc__.split("\n\n")[0])
  ap.add_argument("file", help="trajectory in the .config format")
  ap.add_argument("np", type=int, help="number of bodies per frame")
  ap.add_argument("lx", type=float)
  ap.add_argument("ly", type=float)
  ap.add_argument("lz", type=float)
  ap.add_argument("--lags", type=int, required=True, help="number of lags, 0 .. L - 1 (at most the number of frames used)")
  ap.add_argument("--dt", type=float, default=1.0, help="time between saved frames")
  ap.add_argument("--rmax", type=float, default=None, help="default: half the smallest positive period of the plane")
  ap.add_argument("--bins", type=int, default=1000)
  ap.add_argument("--self-rmax", dest="self_rmax", type=float, default=None, help="default --rmax")
  ap.add_argument("--self-bins", dest="self_bins", type=int, default=None, help="default --bins")
  ap.add_argument("--plane", choices=PLANES, default="xyz")
  ap.add_argument("--every", type=int, default=1, help="use every K-th frame (a lag is then K dt)")
  ap.add_argument("--skip", type=int, default=0, help="leave out the first S frames")
  ap.add_argument("--origins", choices=ORIGINS, default="window")
  ap.add_argument("--no-distinct", dest="distinct", action="store_false", help="the self part only")
  ap.add_argument("--device", type=int, default=0)
  args = ap.parse_args(argv)
  if args.every < 1 or args.lags < 1:
    ap.error("--every and --lags must be at least 1")
  L = (args.lx, args.ly, args.lz)
  try:
    if not 1 <= args.bins <= MAX_BINS or not (args.self_bins is None or 1 <= args.self_bins <= MAX_BINS):
      raise ValueError("--bins and --self-bins must be 1 ... %d" % MAX_BINS)
    for name, r in (("--rmax", args.rmax), ("--self-rmax", args.self_rmax)):
      if r is not None and not (r > 0.0 and np.isfinite(r)):
        raise ValueError("%s must be positive and finite, got %r" % (name, r))
    if args.rmax is None and not any(x > 0 for x in (L[:2] if args.plane == "xy" else L)):
      raise ValueError("--rmax is needed: the box has no positive period in the plane")
    if args.distinct:      # refuses the box that Gd() would
      normalise_distinct(np.zeros((1, 1)), np.ones(1), max(args.np, 1), _lengths(L), 1.0, "3d" if args.plane == "xyz" else "2d")
    frames = load_trajectory(args.file, args.np, args.skip)[::args.every]
    acc = VanHove(args.np, L, min(args.lags, frames.shape[0]), dt=args.dt * args.every, r_max=args.rmax, n_bins=args.bins,
                  self_r_max=args.self_rmax, self_n_bins=args.self_bins, origins=args.origins, plane=args.plane, distinct=args.distinct,
                  device=args.device)
  except ValueError as exc:
    ap.error(str(exc))
  try:
    acc.add_frames(frames).finish()
    (out or sys.stdout).write(acc.format())
  finally:
    acc.close()
  return 0


if __name__ == "__main__":
  sys.exit(main())
