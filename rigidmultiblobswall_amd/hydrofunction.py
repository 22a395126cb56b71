"""Hydrodynamic function H(k) of point trajectories on MI355X: the short-time collective diffusion D(k) = D0 H(k) / S(k).

    python -m rigidmultiblobswall_amd.hydrofunction run.config np lx ly lz --radius A --eta ETA [--nmax M | --kmax KM]
                                                    [--plane xy|xyz] [--polarisation longitudinal|transverse|vertical]
                                                    [--no-wall] [--open] [--every K] [--skip S] [--shells B] [--with-S]
                                                    [--device N]

The positional arguments and the frame reader are those of rigidmultiblobswall_amd.scattering (a `.config` trajectory, the
number of bodies, the box); the points are the location columns, every point a blob of radius A in a fluid of viscosity ETA.
It prints `kx ky kz |k| H_s H_d H stderr` per wavevector (with --shells B `k n_k H_s H_d H stderr` per shell of |k|), and
with --with-S two more columns `S H/S`, S from the density-mode sweep on the same frames.

    H(k; e) = (1 / (N mu0)) < sum_i sum_j  e^T M_ij e  cos(k . (x_i - x_j)) >,     mu0 = 1 / (6 pi eta a),

averaged over the frames: H_s is the part i = j (the short-time self diffusion in units of D0, the k -> infinity limit of H),
H_d the part i != j, stderr the standard error of the mean of H over the frames.  M is the translational mobility this
engine uses everywhere: the RPY block (overlap patch included), above the wall z = 0 the single-wall block with heights
clamped to a and blobs below a damped by z / a (--no-wall: unbounded), summed over the 3 x 3 periodic images in x and y
(--open: no images).  e is the polarisation: "longitudinal" (k / |k|, what scattering sees), "transverse" (z x k / |k_xy|) or
"vertical" (z).  Wavevectors k = 2 pi n_d / L_d as in rigidmultiblobswall_amd.scattering.

The sums come from one HIP sweep (rmb_hydro_function_frames_device): the pair block is built once per pair and contracted
with eight wavevectors at a time; there is no CPU fall-back.
"""
import argparse
import sys

import numpy as np

from ._lagged import UPLOAD_BYTES, ContextHolder, lengths as _lengths
from .scattering import PLANES, _check_wavevectors, k_vectors, shell_average, wavevectors as _wavevectors

POLARISATIONS = ("longitudinal", "transverse", "vertical")


def polarisations(periodic_length, wavevectors, polarisation="longitudinal"):
  """Unit polarisation vectors (K, 3) float64 of the integer wavevectors (K, 3), formed in long double and rounded once:
  "longitudinal" k / |k| (refused for n = 0, which has no direction), "transverse" z x k / |k_xy| = (-k_y, k_x, 0) / |k_xy|
  (refused where k_x = k_y = 0), "vertical" z; a (K, 3) array is returned as float64, as it is."""
  n = np.asarray(wavevectors).reshape(-1, 3)
  if not isinstance(polarisation, str):
    e = np.ascontiguousarray(polarisation, dtype=np.float64)
    if e.shape != n.shape or not np.all(np.isfinite(e)):
      raise ValueError("a polarisation array must hold one finite vector per wavevector, shape (K, 3), got %r" % (e.shape,))
    return e
  if polarisation not in POLARISATIONS:
    raise ValueError("polarisation must be one of %s or a (K, 3) array, got %r" % (POLARISATIONS, polarisation))
  k_vectors(periodic_length, n)      # refuses a nonzero n_d along a direction without a length
  L = _lengths(periodic_length).astype(np.longdouble)
  safe = np.where(L > 0, L, np.longdouble(1))
  k = np.where(n != 0, n.astype(np.longdouble) / safe[None, :], np.longdouble(0))      # k / (2 pi)
  e = np.zeros(n.shape, dtype=np.longdouble)
  if polarisation == "vertical":
    e[:, 2] = 1
  elif polarisation == "longitudinal":
    norm = np.sqrt(np.sum(k * k, axis=1))
    if np.any(norm == 0):
      raise ValueError("the longitudinal polarisation of n = 0 does not exist: pass the polarisation as a (K, 3) array")
    e = k / norm[:, None]
  else:
    norm = np.sqrt(k[:, 0] * k[:, 0] + k[:, 1] * k[:, 1])
    if np.any(norm == 0):
      raise ValueError("the transverse polarisation needs k_xy != 0")
    e[:, 0], e[:, 1] = -k[:, 1] / norm, k[:, 0] / norm
  return np.ascontiguousarray(e, dtype=np.float64)


class HydroSums(object):
  """The host side of the hydrodynamic function: per-wavevector sums and sums of squares over frames of H_s, H_d and H, and
  everything derived from them.  add_values(values) takes (k, K, 2) per-frame (H_s, H_d), frame by frame in order, so the
  sums do not depend on how a trajectory was cut.  HydrodynamicFunction fills it from the GPU."""

  def __init__(self, periodic_length, wavevectors):
    self.periodic_length = _lengths(periodic_length)
    self.wavevectors = _check_wavevectors(self.periodic_length, wavevectors)
    self.K = int(self.wavevectors.shape[0])
    self.k = k_vectors(self.periodic_length, self.wavevectors)
    self.k_norm = np.sqrt(np.sum(self.k ** 2, axis=1))
    self.n_frames = 0
    self._sum = np.zeros((3, self.K))       # H_s, H_d, H
    self._sum2 = np.zeros((3, self.K))

  def add_values(self, values):
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 3 or v.shape[1:] != (self.K, 2):
      raise ValueError("values must have shape (frames, K, 2), got %r" % (v.shape,))
    for row in v:
      cols = np.stack([row[:, 0], row[:, 1], row[:, 0] + row[:, 1]])
      self._sum += cols
      self._sum2 += cols * cols
    self.n_frames += int(v.shape[0])
    return self

  def _mean(self, c):
    with np.errstate(divide="ignore", invalid="ignore"):
      return self._sum[c] / np.float64(self.n_frames)

  def H_self(self):
    return self._mean(0)

  def H_distinct(self):
    return self._mean(1)

  def H(self):
    return self._mean(2)

  def stderr(self):
    """standard error of the mean of H over the frames (nan with fewer than two)"""
    F = np.float64(self.n_frames)
    with np.errstate(divide="ignore", invalid="ignore"):
      var = (self._sum2[2] - self._sum[2] * self._sum[2] / F) / (F - 1.0)
      return np.sqrt(np.maximum(var, 0.0) / F) if self.n_frames >= 2 else np.full(self.K, np.nan)

  def D_short(self, S):
    """H / S: the short-time collective diffusion coefficient in units of D0"""
    S = np.asarray(S, dtype=np.float64)
    if S.shape != (self.K,):
      raise ValueError("S must hold one value per wavevector")
    with np.errstate(divide="ignore", invalid="ignore"):
      return self.H() / S

  def _columns(self, S=None):
    cols = [self.H_self(), self.H_distinct(), self.H(), self.stderr()]
    if S is not None:
      cols += [np.asarray(S, dtype=np.float64), self.D_short(S)]
    return np.stack(cols)

  def shells(self, n_bins, values=None):
    """Average over n_bins shells of equal width in |k| on (0, max |k|]: (k_mean, n_k, values), values (..., n_bins) the average
    of `values` (..., K) -- H() when None -- over a shell's wavevectors; nan where a shell is empty."""
    n_bins = int(n_bins)
    if n_bins < 1:
      raise ValueError("n_bins must be at least 1, got %r" % (n_bins,))
    v = self.H() if values is None else np.asarray(values, dtype=np.float64)
    if v.shape[-1] != self.K:
      raise ValueError("values must have one entry per wavevector along the last axis")
    return shell_average(self.k_norm, v, n_bins)

  def format(self, shells=None, S=None):
    """The command line's output (see the module's docstring); every float with 17 significant digits."""
    cols = self._columns(S)
    if shells:
      k_mean, n_k, v = self.shells(shells, cols)
      return "".join("%.17g %d %s\n" % (k_mean[b], n_k[b], " ".join("%.17g" % x for x in v[:, b])) for b in range(len(n_k)))
    return "".join("%.17g %.17g %.17g %.17g %s\n" % (self.k[i, 0], self.k[i, 1], self.k[i, 2], self.k_norm[i],
                                                    " ".join("%.17g" % x for x in cols[:, i])) for i in range(self.K))

  def write(self, path, shells=None, S=None):
    with open(path, "w") as f:
      f.write(self.format(shells, S))


class HydrodynamicFunction(HydroSums, ContextHolder):
  """Accumulates the hydrodynamic function of a trajectory of n_points blobs of radius `a` in a fluid of viscosity `eta` for the
  integer wavevectors `wavevectors` (K, 3) of the box L.  wall: the no-slip wall at z = 0 (True) or none; periodic: the
  mobility sums the 3 x 3 images in x and y with the periods L[0], L[1] (True) or takes the open form; polarisation: see
  polarisations().  add_frames(frames) takes frames (k, n_points, 3), numpy or CUDA float64 tensor, in any number of pieces;
  finish() closes the stream.  H(), H_self(), H_distinct() (K,): means over the frames; stderr(); D_short(S) = H / S;
  shells(n_bins); format(), write(path).  ctx: a single-GPU MobilityContext (its resident configuration is left alone); None
  makes one on `device`, closed by close()."""
  entry, what = "hydrodynamic_function_frames_device", "the hydrodynamic function runs"

  def __init__(self, n_points, L, wavevectors, a, eta, wall=True, periodic=True, polarisation="longitudinal", ctx=None, device=0):
    HydroSums.__init__(self, L, wavevectors)
    self.n = self.n_points = int(n_points)
    if self.n < 1:
      raise ValueError("n_points must be at least 1, got %r" % (n_points,))
    if np.ndim(a) != 0:
      raise ValueError("the hydrodynamic function takes one radius, not per-blob radii")
    self.a, self.eta = float(a), float(eta)
    if not (self.a > 0.0 and np.isfinite(self.a)) or not (self.eta > 0.0 and np.isfinite(self.eta)):
      raise ValueError("the radius and eta must be positive and finite, got %r and %r" % (a, eta))
    if isinstance(wall, str):
      raise ValueError("wall must be True (no-slip wall at z = 0) or False, got %r: no free surface" % (wall,))
    self.wall, self.periodic = bool(wall), bool(periodic)
    if self.periodic and not (self.periodic_length[0] > 0 and self.periodic_length[1] > 0):
      raise ValueError("a periodic mobility needs positive lengths in x and y (periodic=False: the open form)")
    self.mobility_periodic_length = np.array([self.periodic_length[0], self.periodic_length[1], 0.0]) if self.periodic else np.zeros(3)
    self.polarisation = polarisations(self.periodic_length, self.wavevectors, polarisation)
    self._finished = False
    self._open(device, ctx)

  def _per(self):
    """frames per call: the upload piece, and at most 64 MB of results"""
    return max(1, min(UPLOAD_BYTES // (8 * 3 * self.n), UPLOAD_BYTES // (16 * max(self.K, 1))))

  def add_frames(self, frames):
    if self._finished:
      raise ValueError("add_frames() after finish()")
    torch = self._torch
    on_device = isinstance(frames, torch.Tensor)
    if on_device and not (frames.is_cuda and frames.dtype == torch.float64):
      raise ValueError("frames must be a numpy array or a CUDA float64 tensor")
    f = frames if on_device else np.ascontiguousarray(frames, dtype=np.float64)
    size, row = (f.numel() if on_device else f.size), 3 * self.n
    if size % row:
      raise ValueError("frames must hold whole frames of %d points x 3 coordinates, got shape %r" % (self.n, tuple(f.shape)))
    f = f.reshape(-1, self.n, 3)
    scale = 6.0 * np.pi * self.eta * self.a / self.n      # 1 / (N mu0)
    per = self._per()
    for k in range(0, f.shape[0], per):
      piece = f[k:k + per]
      if not on_device:      # torch refuses a read-only array
        piece = torch.from_numpy(piece if piece.flags.writeable else piece.copy()).to(self._dev)
      with torch.cuda.device(self._dev):
        sums = self.ctx.hydrodynamic_function_frames_device(piece.contiguous(), self.a, self.eta, self.periodic_length, self.wavevectors,
                                                            self.polarisation, wall=self.wall,
                                                            mobility_periodic_length=self.mobility_periodic_length)
      self.add_values(sums.cpu().numpy() * scale)
    return self

  def finish(self):
    self._finished = True
    return self


def parse_args(argv=None):
  """The command line's arguments, checked."""
  ap = argparse.ArgumentParser(prog="python -m rigidmultiblobswall_amd.hydrofunction", description=__doc__.split("\n\n")[0])
  ap.add_argument("file", help="trajectory in the .config format")
  ap.add_argument("np", type=int, help="number of bodies per frame")
  ap.add_argument("lx", type=float)
  ap.add_argument("ly", type=float)
  ap.add_argument("lz", type=float)
  ap.add_argument("--radius", type=float, required=True, help="blob radius a")
  ap.add_argument("--eta", type=float, required=True, help="viscosity")
  ap.add_argument("--nmax", type=int, default=None, help="|n_d| <= M (default 8 when --kmax is not given)")
  ap.add_argument("--kmax", type=float, default=None, help="|k| <= KM")
  ap.add_argument("--plane", choices=PLANES, default="xy")
  ap.add_argument("--polarisation", choices=POLARISATIONS, default="longitudinal")
  ap.add_argument("--no-wall", dest="wall", action="store_false", help="unbounded mobility instead of the wall at z = 0")
  ap.add_argument("--open", dest="periodic", action="store_false", help="no periodic images of the mobility")
  ap.add_argument("--every", type=int, default=1, help="use every K-th frame")
  ap.add_argument("--skip", type=int, default=0, help="leave out the first S frames")
  ap.add_argument("--shells", type=int, default=0, help="average over B shells of |k|")
  ap.add_argument("--with-S", dest="with_S", action="store_true", help="also the structure factor S and H / S")
  ap.add_argument("--device", type=int, default=0)
  args = ap.parse_args(argv)
  if args.every < 1 or args.skip < 0 or args.shells < 0 or args.np < 1:
    ap.error("--every and np must be at least 1; --skip and --shells must not be negative")
  if not (args.radius > 0.0 and np.isfinite(args.radius)) or not (args.eta > 0.0 and np.isfinite(args.eta)):
    ap.error("--radius and --eta must be positive and finite")
  return args


def main(argv=None, out=None):
  from .correlation import load_trajectory
  from .scattering import IntermediateScattering
  args = parse_args(argv)
  L = (args.lx, args.ly, args.lz)
  try:
    wv = _wavevectors(L, n_max=8 if args.nmax is None and args.kmax is None else args.nmax, k_max=args.kmax, plane=args.plane)
    if wv.shape[0] < 1:
      raise ValueError("no wavevector selected: the box needs a positive lx or ly (or lz with --plane xyz)")
    frames = load_trajectory(args.file, args.np, args.skip)[::args.every]
    acc = HydrodynamicFunction(args.np, L, wv, args.radius, args.eta, wall=args.wall, periodic=args.periodic,
                               polarisation=args.polarisation, device=args.device)
  except ValueError as exc:
    print("hydrofunction: %s" % exc, file=sys.stderr)
    return 2
  try:
    acc.add_frames(frames).finish()
    S = None
    if args.with_S:
      sk = IntermediateScattering(args.np, L, wv, n_lags=1, ctx=acc.ctx)
      S = sk.add_frames(frames).finish().S()
    (out or sys.stdout).write(acc.format(args.shells, S))
  finally:
    acc.close()
  return 0


if __name__ == "__main__":
  sys.exit(main())
