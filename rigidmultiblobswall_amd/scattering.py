"""Structure factor S(k), intermediate scattering function F(k, t) and its self part F_s(k, t) of point trajectories on MI355X.

    python -m rigidmultiblobswall_amd.scattering run.config np lx ly lz [--nmax M | --kmax KM] [--plane xy|xyz] [--lags L]
                                                 [--dt DT] [--every K] [--skip S] [--origins window|all] [--self]
                                                 [--shells B] [--device N]

The positional arguments are those of rigidmultiblobswall_amd.correlation (a `.config` trajectory, the number of bodies, the
box); the points are the location columns.  With --lags 1 (the default) it prints `kx ky kz |k| S` per wavevector, with
--shells B `k n_k S` per shell of |k|; with --lags L > 1 one block per lag: a line `# t T n_origins`, then the same lines with
F(k, t) in place of S, and F_s(k, t) as one more column with --self.

Direct Fourier sums, no grid (the reference handed positions to the external HydroGrid library, which bins them on a grid):
with wavevectors k = 2 pi (n_x / L_x, n_y / L_y, n_z / L_z), integer n,

    rho_k(f)  = sum_j exp(-i k . x_j(f)),
    S(k)      = < |rho_k|^2 > / N,
    F(k, l)   = < Re rho_k(o + l) conj rho_k(o) > / N,
    F_s(k, l) = < cos k . (x_j(o + l) - x_j(o)) >  over origins o and points j.

The sums come from the HIP sweeps (rmb_density_modes_frames_device: a lane owns a wavevector; rmb_scattering_lags_device and
rmb_self_scattering_frames_device: a lane owns a lag); there is no CPU fall-back.  The phase is reduced in turns before it is
multiplied by 2 pi, so unwrapped trajectories that have drifted many periods keep their accuracy.  Origins "window" and "all"
are those of rigidmultiblobswall_amd.msd.
"""
import argparse
import sys

import numpy as np

from ._lagged import ORIGINS, UPLOAD_BYTES, LagAccumulator, lengths as _lengths

PLANES = ("xy", "xyz")
MAX_WAVEVECTORS = 16384       # per call of the kernel entries
MAX_INDEX = 32768


def k_vectors(periodic_length, wavevectors):
  """k = 2 pi n_d / L_d as float64 (K, 3); a component with n_d = 0 is 0 whatever L_d."""
  L = _lengths(periodic_length)
  n = np.asarray(wavevectors).reshape(-1, 3)
  if np.any((n != 0) & ~(L > 0)[None, :]):
    raise ValueError("a nonzero n_d needs a positive length L_d")
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.where(n != 0, 2.0 * np.pi * n / L[None, :], 0.0)


def wavevectors(periodic_length, n_max=None, k_max=None, plane="xy"):
  """Integer triples n (int32, (K, 3)) of the wavevectors k = 2 pi n_d / L_d with |n_d| <= n_max and / or |k| <= k_max (at least
  one of the two): one of every +-n pair (the one whose first nonzero component is positive), never n = 0.  plane="xy":
  n_z = 0, the monolayer; "xyz": all three.  A direction with L_d <= 0 gets n_d = 0.  Order: by |k|, then lexicographically
  in (n_x, n_y, n_z); |k|^2 is compared to 40 bits, so that vectors of one shell that differ in the last bit still tie."""
  L = _lengths(periodic_length)
  if plane not in PLANES:
    raise ValueError("plane must be one of %s, got %r" % (PLANES, plane))
  if n_max is None and k_max is None:
    raise ValueError("wavevectors() needs n_max or k_max")
  if n_max is not None and (int(n_max) != n_max or int(n_max) < 0):
    raise ValueError("n_max must be a non-negative integer, got %r" % (n_max,))
  if k_max is not None and not float(k_max) >= 0.0:
    raise ValueError("k_max must not be negative, got %r" % (k_max,))
  axes = []
  for d in range(3):
    m = 0
    if L[d] > 0 and (d < 2 or plane == "xyz"):
      m = MAX_INDEX if n_max is None else int(n_max)
      if k_max is not None:
        m = min(m, int(np.floor(float(k_max) * L[d] / (2.0 * np.pi) * (1.0 + 1e-12))))
    if m > MAX_INDEX:
      raise ValueError("|n_d| must be at most %d" % MAX_INDEX)
    axes.append(np.arange(-m, m + 1, dtype=np.int64))
  if float(len(axes[0])) * len(axes[1]) * len(axes[2]) > 5.0e7:
    raise ValueError("too many candidate wavevectors; lower n_max or k_max")
  n = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
  first = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
  n = n[first > 0]
  k2 = np.sum(k_vectors(L, n) ** 2, axis=1)
  if k_max is not None:
    n, k2 = n[k2 <= float(k_max) ** 2 * (1.0 + 1e-12)], k2[k2 <= float(k_max) ** 2 * (1.0 + 1e-12)]
  mant, expo = np.frexp(k2)
  key = np.ldexp(np.round(mant * 2.0 ** 40), expo - 40)
  order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], key))
  return np.ascontiguousarray(n[order], dtype=np.int32)


def _check_wavevectors(periodic_length, wv):
  k = np.asarray(wv)
  if k.dtype.kind not in "iu" or k.ndim != 2 or k.shape[1] != 3:
    raise ValueError("wavevectors must be an integer array of shape (K, 3), got %r" % (getattr(k, "shape", None),))
  if k.shape[0] > MAX_WAVEVECTORS:
    raise ValueError("at most %d wavevectors, got %d" % (MAX_WAVEVECTORS, k.shape[0]))
  if np.any(np.abs(k.astype(np.int64)) > MAX_INDEX):
    raise ValueError("|n_d| must be at most %d" % MAX_INDEX)
  k_vectors(periodic_length, k)      # refuses a nonzero n_d along a direction without a length
  return np.ascontiguousarray(k, dtype=np.int32)


class IntermediateScattering(LagAccumulator):
  """Accumulates the lag sums of a trajectory of n_points points over n_lags lags (lag l = l frames = l dt) for the
  integer wavevectors `wavevectors` (K, 3) in the box periodic_length.  add_frames(frames) takes frames (k, n_points, 3),
  numpy or CUDA float64 tensor, in any number of pieces; between calls only the density modes of the last n_lags - 1 frames
  stay on the device (with self_part=True those frames too), so a trajectory may be larger than device memory.  finish()
  ends the trajectory (origins="all": the frames still held are origins of the lags that exist for them).  counts():
  origins per lag, msd.counts_per_lag for one body; times() = dt * lag; S() (K,), F() and Fs() (n_lags, K), nan where a lag
  has no origin; shells(n_bins) averages over shells of |k|; write(path).  n_lags=1 is the plain structure factor.  ctx: a
  single-GPU MobilityContext (its resident configuration is left alone); None makes one on `device`, closed by close()."""
  width, entry = 3, "density_modes_frames_device"
  what, row = "the scattering functions run", ("n_points", "%d points x 3 coordinates")

  def __init__(self, n_points, periodic_length, wavevectors, n_lags=1, dt=1.0, origins="window", self_part=False, device=0, ctx=None):
    LagAccumulator.__init__(self, n_points, n_lags, dt, origins)
    self.n_points, self.self_part = self.n, bool(self_part)
    self.periodic_length = _lengths(periodic_length)
    self.wavevectors = _check_wavevectors(self.periodic_length, wavevectors)
    self.K = int(self.wavevectors.shape[0])
    self.k = k_vectors(self.periodic_length, self.wavevectors)
    self.k_norm = np.sqrt(np.sum(self.k ** 2, axis=1))
    self._open(device, ctx)
    torch = self._torch
    self._C = torch.zeros((self.n_lags, self.K), dtype=torch.float64, device=self._dev)
    self._Sf = torch.zeros((self.n_lags, self.K), dtype=torch.float64, device=self._dev) if self.self_part else None
    self._counts = np.zeros(self.n_lags, dtype=np.int64)

  def _per(self):
    return max(self.n_lags, min(UPLOAD_BYTES // (8 * max(3 * self.n_points, 1)), (4 * UPLOAD_BYTES) // (16 * max(self.K, 1))))

  def _records(self, piece):
    """the modes of every frame, and the frames themselves for the self part"""
    with self._torch.cuda.device(self._dev):
      modes = self.ctx.density_modes_frames_device(piece, self.periodic_length, self.wavevectors)
    return (modes, piece) if self.self_part else (modes,)

  def _call(self, records, origins):
    with self._torch.cuda.device(self._dev):
      _, n = self.ctx.scattering_lags_device(records[0], self.n_lags, origins=origins, out=self._C)
      if self.self_part:
        self.ctx.self_scattering_frames_device(records[1], self.periodic_length, self.wavevectors, self.n_lags, origins=origins, out=self._Sf)
    self._counts += n

  def collective_sums(self):
    return self._C.cpu().numpy()

  def self_sums(self):
    if not self.self_part:
      raise ValueError("the self part was not asked for (self_part=True)")
    return self._Sf.cpu().numpy()

  def counts(self):
    return self._counts.copy()

  def _normalised(self, sums):
    with np.errstate(divide="ignore", invalid="ignore"):
      return sums / (float(self.n_points) * self._counts.astype(np.float64))[:, None]

  def F(self):
    return self._normalised(self.collective_sums())

  def Fs(self):
    return self._normalised(self.self_sums())

  def S(self):
    return self.F()[0]

  def shells(self, n_bins, values=None):
    """Average over n_bins shells of equal width in |k| on (0, max |k|]: (k_mean, n_k, values) with k_mean (n_bins,) the mean
    |k| of a shell's wavevectors, n_k their number and values (..., n_bins) the average of `values` (..., K) -- S() when
    None -- over them; nan where a shell is empty."""
    n_bins = int(n_bins)
    if n_bins < 1:
      raise ValueError("n_bins must be at least 1, got %r" % (n_bins,))
    v = self.S() if values is None else np.asarray(values, dtype=np.float64)
    if v.shape[-1] != self.K:
      raise ValueError("values must have one entry per wavevector along the last axis")
    return shell_average(self.k_norm, v, n_bins)

  def write(self, path, shells=None):
    with open(path, "w") as f:
      f.write(self.format(shells))

  def format(self, shells=None):
    """The command line's output (see the module's docstring); every float with 17 significant digits."""
    cols = [self.F()] + ([self.Fs()] if self.self_part else [])
    out = []
    for lag in range(self.n_lags):
      if self.n_lags > 1:
        out.append("# t %.17g %d\n" % (self.dt * lag, self._counts[lag]))
      if shells:
        k_mean, n_k, v = self.shells(shells, np.stack([c[lag] for c in cols]))
        out.extend("%.17g %d %s\n" % (k_mean[b], n_k[b], " ".join("%.17g" % x for x in v[:, b])) for b in range(len(n_k)))
      else:
        out.extend("%.17g %.17g %.17g %.17g %s\n" % (self.k[i, 0], self.k[i, 1], self.k[i, 2], self.k_norm[i],
                                                    " ".join("%.17g" % c[lag, i] for c in cols)) for i in range(self.K))
    return "".join(out)


def shell_average(k_norm, values, n_bins):
  k_norm = np.asarray(k_norm, dtype=np.float64)
  top = k_norm.max() if k_norm.size else 1.0
  idx = np.minimum((k_norm / top * n_bins).astype(np.int64), n_bins - 1) if top > 0 else np.zeros(k_norm.size, dtype=np.int64)
  n_k = np.bincount(idx, minlength=n_bins)
  with np.errstate(divide="ignore", invalid="ignore"):
    k_mean = np.bincount(idx, weights=k_norm, minlength=n_bins) / n_k
    flat = values.reshape(-1, k_norm.size)
    avg = np.stack([np.bincount(idx, weights=row, minlength=n_bins) / n_k for row in flat]).reshape(values.shape[:-1] + (n_bins,))
  return k_mean, n_k, avg


def main(argv=None, out=None):
  from .correlation import load_trajectory
  ap = argparse.ArgumentParser(prog="python -m rigidmultiblobswall_amd.scattering", description=__doc__.split("\n\n")[0])
  ap.add_argument("file", help="trajectory in the .config format")
  ap.add_argument("np", type=int, help="number of bodies per frame")
  ap.add_argument("lx", type=float)
  ap.add_argument("ly", type=float)
  ap.add_argument("lz", type=float)
  ap.add_argument("--nmax", type=int, default=None, help="|n_d| <= M (default 8 when --kmax is not given)")
  ap.add_argument("--kmax", type=float, default=None, help="|k| <= KM")
  ap.add_argument("--plane", choices=PLANES, default="xy")
  ap.add_argument("--lags", type=int, default=1, help="number of lags, 0 .. L - 1 (at most the number of frames used); 1: S(k) only")
  ap.add_argument("--dt", type=float, default=1.0, help="time between saved frames")
  ap.add_argument("--every", type=int, default=1, help="use every K-th frame (a lag is then K dt)")
  ap.add_argument("--skip", type=int, default=0, help="leave out the first S frames")
  ap.add_argument("--origins", choices=ORIGINS, default="window")
  ap.add_argument("--self", dest="self_part", action="store_true", help="also the self part F_s")
  ap.add_argument("--shells", type=int, default=0, help="average over B shells of |k|")
  ap.add_argument("--device", type=int, default=0)
  args = ap.parse_args(argv)
  if args.every < 1 or args.lags < 1 or args.shells < 0:
    ap.error("--every and --lags must be at least 1, --shells must not be negative")
  L = (args.lx, args.ly, args.lz)
  try:
    wv = wavevectors(L, n_max=8 if args.nmax is None and args.kmax is None else args.nmax, k_max=args.kmax, plane=args.plane)
    if wv.shape[0] < 1:
      raise ValueError("no wavevector selected: the box needs a positive lx or ly (or lz with --plane xyz)")
    frames = load_trajectory(args.file, args.np, args.skip)[::args.every]
    acc = IntermediateScattering(args.np, L, wv, n_lags=min(args.lags, frames.shape[0]), dt=args.dt * args.every, origins=args.origins,
                                 self_part=args.self_part, device=args.device)
  except ValueError as exc:
    ap.error(str(exc))
  try:
    acc.add_frames(frames).finish()
    (out or sys.stdout).write(acc.format(args.shells))
  finally:
    acc.close()
  return 0


if __name__ == "__main__":
  sys.exit(main())
