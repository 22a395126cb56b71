"""Bond-orientational order of point trajectories on MI355X: psi_m(i), its pair correlation g_m(r) and its time correlation C_m(t).

    python -m rigidmultiblobswall_amd.bondorder run.config np lx ly lz --orders 4,6 --rcut R [--rmax R --bins B] [--lags L --dt DT]
                                                [--plane xy|xyz] [--every K] [--skip S] [--origins window|all] [--device N]

The positional arguments are those of rigidmultiblobswall_amd.correlation (a `.config` trajectory, the number of bodies, the
box); the points are the location columns.  It prints what BondOrder.format() writes (below).

With frames x_i(f), orders m and a cutoff r_cut,

    psi_m(i)  = N_i^-1 sum_j z_ij^m over the N_i neighbours j of i: d_ij < r_cut in the minimal image of every periodic
                direction and rho_ij > 0, z_ij = (dx + i dy) / rho_ij, rho the in-plane distance; 0 where N_i = 0.  plane="xy":
                d = rho; "xyz": d is the 3-D distance (the bond angle stays the in-plane one);
    g_m(r)    = < Re psi_m(i) psi_m*(j) > over the unordered pairs of a frame at distance r (plane as above);
    C_m(l)    = sum_o sum_i Re psi_m(i, o + l) psi_m*(i, o), printed as (C_m(l) / n_origins(l)) / (C_m(0) / n_origins(0)).

The neighbour sums come from the HIP sweep rmb_bond_order_frames_device (fixed-order fp64 sums, no trigonometric function).
g_m(r) is accumulated in INTEGERS by rmb_pair_field_frames_device on the field quantise(psi) = rint(psi 2^30): a bin's mean is
within (sqrt(2) + 1/2) 2^-30 of the unquantised one, and counts and sums are the same bits however the trajectory is cut and the points are
ordered.  C_m is the lag sweep rmb_scattering_lags_device over the series (Re psi, Im psi) of every point, in blocks of
ORIGIN_BLOCK origins counted from the first frame, so its bits do not depend on the cut either.  The means < |psi_m| > and
< |N^-1 sum_i psi_m(i)| > are sums of rint(. 2^30) as well.  There is no CPU fall-back.

Not here: neighbour lists (every pair of a frame is met), Voronoi neighbours, single precision, multi-device contexts.
"""
import argparse
import sys

import numpy as np

from ._lagged import ORIGINS, LagAccumulator, counts_per_lag, lengths as _lengths

PLANES = ("xy", "xyz")
MAX_BINS = 4096
MAX_ORDERS, MAX_ORDER = 4, 16
FIELD_SCALE = 2 ** 30
COUNT_LIMIT = 2 ** 32       # a bin's accumulated count: |sums| <= count (2^30 + 1) stays far inside int64
ORIGIN_BLOCK = 256          # origins per call of the lag sweep, counted from the first frame of the trajectory
MAX_SERIES = 16384          # series per call of the lag sweep (rmb_scattering_lags_device)
SOURCE_CHUNK = 8192         # sources per chunk of the neighbour sweep: fixed, so psi's bits do not depend on the frames per call


def check_orders(orders):
  m = np.asarray(orders).reshape(-1)
  if m.dtype.kind not in "iu" or not 1 <= m.size <= MAX_ORDERS or np.any(m < 1) or np.any(m > MAX_ORDER):
    raise ValueError("orders must be 1 ... %d integers in 1 ... %d, got %r" % (MAX_ORDERS, MAX_ORDER, orders))
  return tuple(int(x) for x in m)


def quantise(psi):
  """The int32 field (..., 2) of (a, b) = rint(psi 2^30): psi a complex numpy array (...), a real numpy array (..., 2) of
  (Re, Im), or a torch float64 tensor (..., 2) (then a torch int32 tensor on its device).  Halves round to even.  Refuses a
  component beyond 1 in magnitude after rounding (|a|, |b| <= 2^30 is what the sweep's capacity rests on)."""
  try:
    import torch
    is_tensor = isinstance(psi, torch.Tensor)
  except ImportError:
    is_tensor = False
  if is_tensor:
    if psi.dtype != torch.float64 or psi.dim() < 1 or psi.shape[-1] != 2:
      raise ValueError("psi must be a float64 tensor of shape (..., 2)")
    q = torch.round(psi * float(FIELD_SCALE))
    if q.numel() and not bool((q.abs() <= float(FIELD_SCALE)).all()):      # NaN fails too
      raise ValueError("psi must lie in the unit square: |Re|, |Im| <= 1")
    return q.to(torch.int32)
  p = np.asarray(psi)
  if np.iscomplexobj(p):
    p = np.stack([p.real, p.imag], axis=-1)
  p = np.asarray(p, dtype=np.float64)
  if p.ndim < 1 or p.shape[-1] != 2:
    raise ValueError("psi must be complex (...) or real (..., 2)")
  q = np.rint(p * float(FIELD_SCALE))
  if q.size and not np.all(np.abs(q) <= float(FIELD_SCALE)):
    raise ValueError("psi must lie in the unit square: |Re|, |Im| <= 1")
  return q.astype(np.int32)


def g_from_sums(sums, counts):
  """g = sums / (2^30 counts) per bin; nan where a bin is empty."""
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.asarray(sums, dtype=np.float64) / (float(FIELD_SCALE) * np.asarray(counts, dtype=np.float64))


class BondOrder(LagAccumulator):
  """Accumulates the bond-orientational order of a trajectory of n_points points in the box periodic_length (<= 0: open
  direction) for the orders `orders` (1 ... 4 values in 1 ... 16) and the neighbour cutoff r_cut (keep it below half the
  smallest positive period).  n_bins > 0: also g_m(r) on n_bins <= 4096 bins up to r_max (None: half the smallest positive
  period of the plane).  n_lags > 0: also C_m over n_lags lags (lag l = l frames = l dt; origins as msd).  add_frames(frames)
  takes frames (k, n_points, 3), numpy or CUDA float64 tensor, in any number of pieces; finish() ends the trajectory.
  psi_last(), mean_abs_psi(), global_order(), neighbour_counts(), g_n(), C_n(), format(), write(path).  ctx: a single-GPU
  MobilityContext (its resident configuration is left alone); None makes one on `device`, closed by close()."""
  width, entry = 3, "bond_order_frames_device"
  what, row = "the bond-orientational order runs", ("n_points", "%d points x 3 coordinates")

  def __init__(self, n_points, periodic_length, orders=(6,), r_cut=None, plane="xy", r_max=None, n_bins=0, n_lags=0, dt=1.0,
               origins="window", device=0, ctx=None):
    self.lags = int(n_lags)
    if self.lags < 0:
      raise ValueError("n_lags must not be negative, got %r" % (n_lags,))
    LagAccumulator.__init__(self, n_points, max(self.lags, 1), dt, origins)
    self.n_points = self.n
    self.orders = check_orders(orders)
    if plane not in PLANES:
      raise ValueError("plane must be one of %s, got %r" % (PLANES, plane))
    self.plane = plane
    self.periodic_length = _lengths(periodic_length)
    if r_cut is None or not (float(r_cut) > 0.0 and np.isfinite(float(r_cut))):
      raise ValueError("r_cut must be positive and finite, got %r" % (r_cut,))
    self.r_cut, self.n_bins = float(r_cut), int(n_bins)
    if not 0 <= self.n_bins <= MAX_BINS:
      raise ValueError("n_bins must be 0 (no g_n) ... %d, got %r" % (MAX_BINS, n_bins))
    self.r_max = None
    if self.n_bins:
      if r_max is None:
        periods = self.periodic_length[:2 if plane == "xy" else 3]
        if not np.any(periods > 0):
          raise ValueError("r_max=None needs a positive period in the plane, got %r" % (tuple(self.periodic_length),))
        r_max = 0.5 * float(np.min(periods[periods > 0]))
      self.r_max = float(r_max)
      if not (self.r_max > 0.0 and np.isfinite(self.r_max)):
        raise ValueError("r_max must be positive and finite, got %r" % (r_max,))
    self._open(device, ctx)
    torch = self._torch
    K = len(self.orders)
    self._psi_last = None
    self._abs_q = torch.zeros(K, dtype=torch.int64, device=self._dev)      # sum over frames and points of rint(|psi| 2^30)
    self._glob_q = torch.zeros(K, dtype=torch.int64, device=self._dev)     # sum over frames of rint(|N^-1 sum_i psi| 2^30)
    self._nc = np.zeros(1, dtype=np.int64)
    self._counts = torch.zeros((K, self.n_bins), dtype=torch.int64, device=self._dev)
    self._sums = torch.zeros((K, self.n_bins), dtype=torch.int64, device=self._dev)
    self._blocks = [(p, min(p + MAX_SERIES, self.n)) for p in range(0, self.n, MAX_SERIES)] if self.lags else []
    self._C = [[torch.zeros((self.lags, p1 - p0), dtype=torch.float64, device=self._dev) for p0, p1 in self._blocks] for _ in range(K)]
    self._origins = np.zeros(self.lags, dtype=np.int64)

  # ---- per piece: pass 1, the means, pass 2; the records of the lag sweep -----------------------------------------
  def _records(self, piece):
    torch = self._torch
    K, k = len(self.orders), int(piece.shape[0])
    with torch.cuda.device(self._dev):
      out = self.ctx.bond_order_frames_device(piece, self.periodic_length, self.r_cut, self.orders, plane=self.plane, source_chunk=SOURCE_CHUNK)
      N = out[:, :, :1]
      psi = torch.where(N > 0, out[:, :, 1:] / N, torch.zeros_like(out[:, :, 1:])).reshape(k, self.n, K, 2)
      field = torch.round(psi * float(FIELD_SCALE)).to(torch.int32)      # |sum| / N <= 1 up to a few units of roundoff: inside 2^30
      self._abs_q += torch.round(torch.sqrt(psi[..., 0] * psi[..., 0] + psi[..., 1] * psi[..., 1]) * float(FIELD_SCALE)).to(torch.int64).sum(dim=(0, 1))
      tot = field.to(torch.int64).sum(dim=1).to(torch.float64)            # (k, K, 2): exact integers
      glob = torch.sqrt(tot[..., 0] * tot[..., 0] + tot[..., 1] * tot[..., 1]) / (float(FIELD_SCALE) * max(self.n, 1))
      self._glob_q += torch.round(glob * float(FIELD_SCALE)).to(torch.int64).sum(dim=0)
      nc = torch.bincount(N.reshape(-1).to(torch.int64)).cpu().numpy()
      if nc.size > self._nc.size:
        self._nc = np.concatenate([self._nc, np.zeros(nc.size - self._nc.size, dtype=np.int64)])
      self._nc[:nc.size] += nc
      if k:
        self._psi_last = psi[-1].clone()
      if self.n_bins:
        for j in range(K):
          self.ctx.pair_field_correlation_frames_device(piece, field[:, :, j, :].contiguous(), self.periodic_length, self.r_max, self.n_bins,
                                                        plane=self.plane, counts=self._counts[j], sums=self._sums[j])
        self._check_capacity()
      if not self.lags:
        return (piece.new_empty((k, 0)),)
      return tuple(psi[:, :, j, :].contiguous() for j in range(K))

  def _check_capacity(self):
    if self.n_bins and int(self._counts.max()) >= COUNT_LIMIT:
      raise OverflowError("a bin of g_n has counted 2^32 pairs: use more bins or accumulate in several BondOrder objects")

  # ---- the lag sweep in blocks of ORIGIN_BLOCK origins counted from the first frame -----------------------------------
  def _add_device(self, piece):
    rec = self._records(piece)
    self.n_frames += int(piece.shape[0])
    if not self.lags:
      return
    if self._tail is not None:
      rec = tuple(self._torch.cat([t, r]) for t, r in zip(self._tail, rec))
    complete = max(rec[0].shape[0] - self.n_lags + 1, 0)
    complete -= complete % ORIGIN_BLOCK
    for b in range(0, complete, ORIGIN_BLOCK):
      self._call(tuple(r[b:b + ORIGIN_BLOCK + self.n_lags - 1] for r in rec), "window")
    if complete:
      rec = tuple(r[complete:].clone() for r in rec)
    self._tail = rec if rec[0].shape[0] else None

  def finish(self):
    """End of the trajectory: the origins of the last, partial block (origins="all": every frame still held is an origin of the
    lags that exist for it)."""
    if not self._finished:
      if self.lags and self._tail is not None and (self.origins == "all" or self._tail[0].shape[0] >= self.n_lags):
        self._call(self._tail, self.origins)
      self._tail = None
      self._finished = True
    return self

  def _call(self, records, origins):
    with self._torch.cuda.device(self._dev):
      for j, rec in enumerate(records):
        for b, (p0, p1) in enumerate(self._blocks):
          modes = rec if len(self._blocks) == 1 else rec[:, p0:p1].contiguous()
          self.ctx.scattering_lags_device(modes, self.lags, origins=origins, out=self._C[j][b])
    self._origins += counts_per_lag(int(records[0].shape[0]), 1, self.lags, origins)

  # ---- results -----------------------------------------------------------------------------------------------------
  def psi_last(self):
    """psi of the last frame: complex (n_points, K)"""
    if self._psi_last is None:
      raise ValueError("no frame has been added")
    p = self._psi_last.cpu().numpy()
    return p[..., 0] + 1j * p[..., 1]

  def mean_abs_psi(self):
    """< |psi_m| > over frames and points, per order (nan without frames)"""
    with np.errstate(divide="ignore", invalid="ignore"):
      return self._abs_q.cpu().numpy() / (float(FIELD_SCALE) * np.float64(self.n_frames * self.n))

  def global_order(self):
    """< |N^-1 sum_i psi_m(i)| > over frames, per order (nan without frames)"""
    with np.errstate(divide="ignore", invalid="ignore"):
      return self._glob_q.cpu().numpy() / (float(FIELD_SCALE) * np.float64(self.n_frames if self.n else 0))

  def neighbour_counts(self):
    """int64 array: entry c is the number of (frame, point) with exactly c neighbours"""
    return self._nc.copy()

  def r(self):
    return (np.arange(self.n_bins) + 0.5) * (self.r_max / self.n_bins)

  def pair_counts(self):
    return self._counts.cpu().numpy()

  def pair_sums(self):
    return self._sums.cpu().numpy()

  def g_n(self):
    """(r, g, counts): bin centres, g_m(r) as (K, n_bins) (nan in an empty bin), pair counts per bin"""
    if not self.n_bins:
      raise ValueError("g_n was not asked for (n_bins > 0)")
    counts = self.pair_counts()
    return self.r(), g_from_sums(self.pair_sums(), counts), counts[0]

  def n_origins(self):
    return self._origins.copy()

  def lag_sums(self):
    """C_m(l) = sum_o sum_i Re psi_m(i, o + l) psi_m*(i, o): float64 (K, n_lags)"""
    if not self.lags:
      raise ValueError("C_n was not asked for (n_lags > 0)")
    out = np.zeros((len(self.orders), self.lags))
    for j, blocks in enumerate(self._C):
      for c in blocks:
        out[j] += c.sum(dim=1).cpu().numpy()
    return out

  def C_n(self):
    """(t, C): lag times and (C_m(l) / n_origins(l)) / (C_m(0) / n_origins(0)) as (K, n_lags); nan where a lag has no origin"""
    C = self.lag_sums()
    with np.errstate(divide="ignore", invalid="ignore"):
      per = C / self._origins[None, :].astype(np.float64)
      return self.dt * np.arange(self.lags), per / per[:, :1]

  def format(self):
    """The command line's output: `# orders m1 ...`, `# frames F points N plane P r_cut R`, `# mean_abs_psi ...`, `# global_order
    ...`, `# neighbours c0 c1 ...`; with g_n a line `# g_n` and one line `r counts g_m1 ...` per bin; with C_n a line `# C_n` and
    one line `t n_origins C_m1 ...` per lag.  Every float with 17 significant digits."""
    fl = lambda v: " ".join("%.17g" % x for x in v)      # noqa: E731
    out = ["# orders %s\n" % " ".join("%d" % m for m in self.orders),
           "# frames %d points %d plane %s r_cut %.17g\n" % (self.n_frames, self.n, self.plane, self.r_cut),
           "# mean_abs_psi %s\n" % fl(self.mean_abs_psi()), "# global_order %s\n" % fl(self.global_order()),
           "# neighbours %s\n" % " ".join("%d" % c for c in self._nc)]
    if self.n_bins:
      r, g, counts = self.g_n()
      out.append("# g_n\n")
      out.extend("%.17g %d %s\n" % (r[b], counts[b], fl(g[:, b])) for b in range(self.n_bins))
    if self.lags:
      t, C = self.C_n()
      out.append("# C_n\n")
      out.extend("%.17g %d %s\n" % (t[l], self._origins[l], fl(C[:, l])) for l in range(self.lags))
    return "".join(out)

  def write(self, path):
    with open(path, "w") as f:
      f.write(self.format())


def parse(text):
  """What format() wrote, as a dict: orders, n_frames, n_points, plane, r_cut, mean_abs_psi, global_order, neighbours and, where
  present, r, counts, g (K, n_bins) and t, n_origins, C (K, n_lags)."""
  d, part, rows = {}, None, {"g_n": [], "C_n": []}
  for line in text.splitlines():
    tok = line.split()
    if not tok:
      continue
    if tok[0] == "#":
      if len(tok) == 2 and tok[1] in rows:
        part = tok[1]
      elif tok[1] == "orders":
        d["orders"] = tuple(int(x) for x in tok[2:])
      elif tok[1] == "frames" and len(tok) == 9:
        d.update(n_frames=int(tok[2]), n_points=int(tok[4]), plane=tok[6], r_cut=float(tok[8]))
      elif tok[1] in ("mean_abs_psi", "global_order"):
        d[tok[1]] = np.array([float(x) for x in tok[2:]])
      elif tok[1] == "neighbours":
        d["neighbours"] = np.array([int(x) for x in tok[2:]], dtype=np.int64)
      else:
        raise ValueError("not a bond-order table: %r" % (line,))
    elif part is None or "orders" not in d or len(tok) != 2 + len(d["orders"]):
      raise ValueError("not a bond-order table: %r" % (line,))
    else:
      rows[part].append(tok)
  for name, keys in (("g_n", ("r", "counts", "g")), ("C_n", ("t", "n_origins", "C"))):
    if rows[name]:
      a = np.array(rows[name], dtype=object)
      d[keys[0]] = a[:, 0].astype(np.float64)
      d[keys[1]] = np.array([int(x) for x in a[:, 1]], dtype=np.int64)
      d[keys[2]] = a[:, 2:].astype(np.float64).T
  return d


def main(argv=None, out=None):
  from .correlation import load_trajectory
  ap = argparse.ArgumentParser(prog="python -m rigidmultiblobswall_amd.bondorder", description=__doc__.split("\n\n")[0])
  ap.add_argument("file", help="trajectory in the .config format")
  ap.add_argument("np", type=int, help="number of bodies per frame")
  ap.add_argument("lx", type=float)
  ap.add_argument("ly", type=float)
  ap.add_argument("lz", type=float)
  ap.add_argument("--orders", default="6", help="comma-separated orders m, 1 ... 4 values in 1 ... 16")
  ap.add_argument("--rcut", type=float, required=True, help="neighbour cutoff")
  ap.add_argument("--rmax", type=float, default=None, help="reach of g_n; default: half the smallest positive period of the plane")
  ap.add_argument("--bins", type=int, default=0, help="bins of g_n (0: no g_n)")
  ap.add_argument("--lags", type=int, default=0, help="number of lags of C_n, 0 .. L - 1 (0: no C_n)")
  ap.add_argument("--dt", type=float, default=1.0, help="time between saved frames")
  ap.add_argument("--plane", choices=PLANES, default="xy")
  ap.add_argument("--every", type=int, default=1, help="use every K-th frame (a lag is then K dt)")
  ap.add_argument("--skip", type=int, default=0, help="leave out the first S frames")
  ap.add_argument("--origins", choices=ORIGINS, default="window")
  ap.add_argument("--device", type=int, default=0)
  args = ap.parse_args(argv)
  if args.every < 1 or args.lags < 0:
    ap.error("--every must be at least 1 and --lags must not be negative")
  L = (args.lx, args.ly, args.lz)
  try:
    try:
      orders = tuple(int(x) for x in args.orders.split(","))
    except ValueError:
      raise ValueError("--orders must be comma-separated integers, got %r" % (args.orders,))
    check_orders(orders)
    if not (args.rcut > 0.0 and np.isfinite(args.rcut)):
      raise ValueError("--rcut must be positive and finite, got %r" % (args.rcut,))
    if not 0 <= args.bins <= MAX_BINS:
      raise ValueError("--bins must be 0 ... %d" % MAX_BINS)
    if args.rmax is not None and not (args.rmax > 0.0 and np.isfinite(args.rmax)):
      raise ValueError("--rmax must be positive and finite, got %r" % (args.rmax,))
    if args.bins and args.rmax is None and not any(x > 0 for x in (L[:2] if args.plane == "xy" else L)):
      raise ValueError("--rmax is needed: the box has no positive period in the plane")
    frames = load_trajectory(args.file, args.np, args.skip)[::args.every]
    acc = BondOrder(args.np, L, orders=orders, r_cut=args.rcut, plane=args.plane, r_max=args.rmax, n_bins=args.bins,
                    n_lags=min(args.lags, frames.shape[0]), dt=args.dt * args.every, origins=args.origins, device=args.device)
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
