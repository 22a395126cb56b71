"""A radial pair law U(r) given as a table -- the user-defined interaction of the HIP pair sweeps.

The reference's examples replace the pair interaction by editing Python / CUDA source (user_defined_functions.py,
forces_*_user_defined.py, potential_pycuda_user_defined.py).  Here the law is DATA: K uniform intervals of width h from r0
with one cubic each, K x 4 fp64 coefficients c[k] = (c0, c1, c2, c3); r_cut = r0 + K h.

  r0 <= r < r_cut:  x = (r - r0)/h, k = min(floor(x), K - 1), t = x - k
                    U(r)  = c0 + t (c1 + t (c2 + t c3))
                    U'(r) = (c1 + t (2 c2 + 3 t c3)) / h
  r < r0:           U = c[0][0] + (c[0][1]/h)(r - r0),  U' = c[0][1]/h     (linear core: constant force magnitude)
  r >= r_cut:       U = U' = 0

The force on blob i is (U'(r)/r)(r_j - r_i): the exact derivative of the interpolant whose value is the energy, so force
sweep (MobilityContext.pair_table_force), energy sweep (blob_potential(..., pair_table=T)), sampler and steppers are
consistent by construction.  The four coefficients DEFINE the law; the constructors below only produce them:

  PairTable.from_knots(r0, h, u, du)       cubic Hermite interpolant of K + 1 knot values and slopes
  PairTable.from_function(U, dU, r0, r_cut, K, shift="none"|"energy"|"force")
  PairTable.load(path) / .save(path)       text, `#` comments, three columns  r  U  dU/dr  on a uniform grid (2..1025 rows)

Out of scope (refused where a caller could ask): per-blob radii or species-dependent tables, precision = 32, pair shards
and MultiContext, single-body MCMC moves, body-body tables, non-radial laws.
"""
import numpy as np

K_MAX = 1024
_LD = np.longdouble


class PairTable(object):
  """r0 >= 0, h > 0, coeff (K, 4) fp64 with 1 <= K <= 1024."""

  def __init__(self, r0, h, coeff):
    r0, h = float(r0), float(h)
    c = np.array(coeff, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 4:
      raise ValueError("PairTable: coeff must have shape (K, 4), got %r" % (c.shape,))
    if not 1 <= c.shape[0] <= K_MAX:
      raise ValueError("PairTable: the number of intervals K must be 1..%d, got %d" % (K_MAX, c.shape[0]))
    if not (np.isfinite(h) and h > 0.0):
      raise ValueError("PairTable: the interval width h must be finite and positive, got %r" % (h,))
    if not (np.isfinite(r0) and r0 >= 0.0):
      raise ValueError("PairTable: r0 must be finite and not negative, got %r" % (r0,))
    if not np.all(np.isfinite(c)):
      raise ValueError("PairTable: the coefficients must be finite")
    self.r0, self.h = r0, h
    self.coeff = np.ascontiguousarray(c)
    self.coeff.setflags(write=False)

  @property
  def K(self):
    return self.coeff.shape[0]

  @property
  def r_cut(self):
    return self.r0 + self.K * self.h

  def __repr__(self):
    return "PairTable(r0=%r, h=%r, K=%d, r_cut=%r)" % (self.r0, self.h, self.K, self.r_cut)

  # ---- constructors -----------------------------------------------------------------------------------------------
  @classmethod
  def from_knots(cls, r0, h, u, du):
    """Cubic Hermite interpolant of the K + 1 knot values u and slopes du (dU/dr) at r0 + k h:
      c0 = u_k, c1 = h d_k, c2 = 3 (u_{k+1} - u_k) - h (2 d_k + d_{k+1}), c3 = 2 (u_k - u_{k+1}) + h (d_k + d_{k+1}),
    formed in np.longdouble and rounded once: in fp64 the differences in c2 and c3 lose |u| / (h |U'|) units on a fine table."""
    u = np.asarray(u, dtype=_LD).reshape(-1)
    d = np.asarray(du, dtype=_LD).reshape(-1)
    if u.size != d.size or u.size < 2:
      raise ValueError("PairTable.from_knots: u and du must have the same length K + 1 >= 2, got %d and %d" % (u.size, d.size))
    hl = _LD(h)
    c = np.empty((u.size - 1, 4), dtype=_LD)
    c[:, 0] = u[:-1]
    c[:, 1] = hl * d[:-1]
    c[:, 2] = _LD(3) * (u[1:] - u[:-1]) - hl * (_LD(2) * d[:-1] + d[1:])
    c[:, 3] = _LD(2) * (u[:-1] - u[1:]) + hl * (d[:-1] + d[1:])
    return cls(r0, h, c.astype(np.float64))

  @classmethod
  def from_function(cls, U, dU, r0, r_cut, K, shift="none"):
    """Samples the callables U(r), dU(r) (which take and return np.longdouble arrays) at the K + 1 knots.
    shift="energy" subtracts U(r_cut); shift="force" subtracts U(r_cut) + (r - r_cut) U'(r_cut), so the table ends at
    u_K = d_K = 0 and both energy and force are continuous at r_cut."""
    if shift not in ("none", "energy", "force"):
      raise ValueError("PairTable.from_function: shift must be 'none', 'energy' or 'force', got %r" % (shift,))
    K = int(K)
    if not 1 <= K <= K_MAX:
      raise ValueError("PairTable.from_function: K must be 1..%d, got %d" % (K_MAX, K))
    if not float(r_cut) > float(r0):
      raise ValueError("PairTable.from_function: r_cut must exceed r0")
    h = (float(r_cut) - float(r0)) / K        # the fp64 numbers the table keeps; the knots are r0 + k h of exactly these
    r = _LD(float(r0)) + np.arange(K + 1, dtype=_LD) * _LD(h)
    u = np.asarray(U(r), dtype=_LD).reshape(-1)
    d = np.asarray(dU(r), dtype=_LD).reshape(-1)
    if shift == "energy":
      u = u - u[-1]
    elif shift == "force":
      u = u - (u[-1] + (r - r[-1]) * d[-1])
      d = d - d[-1]
    return cls.from_knots(float(r0), h, u, d)

  # ---- files ------------------------------------------------------------------------------------------------------
  @classmethod
  def load(cls, path):
    """Text file, `#` comments, rows `r U dU/dr` on a uniform grid (2 to 1025 rows)."""
    rows = []
    with open(path) as fh:
      for n, line in enumerate(fh, 1):
        line = line.split("#", 1)[0].strip()
        if not line:
          continue
        parts = line.split()
        if len(parts) != 3:
          raise ValueError("%s:%d: a pair table row is `r U dU/dr`, got %d columns" % (path, n, len(parts)))
        try:
          rows.append([_LD(p) for p in parts])
        except ValueError:
          raise ValueError("%s:%d: not a number in %r" % (path, n, line))
    if not 2 <= len(rows) <= K_MAX + 1:
      raise ValueError("%s: a pair table file holds 2 to %d rows, got %d" % (path, K_MAX + 1, len(rows)))
    a = np.array(rows, dtype=_LD)
    r = a[:, 0]
    K = len(rows) - 1
    h = (r[-1] - r[0]) / _LD(K)
    if not h > 0:
      raise ValueError("%s: the r column must increase" % (path,))
    # uniform within the precision a decimal fp64 column carries
    dev = np.max(np.abs(r - (r[0] + np.arange(K + 1, dtype=_LD) * h)))
    if dev > _LD(4) * _LD(np.finfo(np.float64).eps) * np.max(np.abs(r)) + _LD(1e-12) * h:
      raise ValueError("%s: the r column is not uniformly spaced (largest deviation %.3g of a spacing %.6g); a pair table "
                       "needs a uniform grid" % (path, float(dev), float(h)))
    return cls.from_knots(float(r[0]), float(h), a[:, 1], a[:, 2])

  def save(self, path):
    """The K + 1 knots r, U, dU/dr of the table (17 significant digits; load() gives the Hermite table of these knots)."""
    r, u, d = self.knots()
    with open(path, "w") as fh:
      fh.write("# pair table: r  U  dU/dr  (uniform grid, K = %d intervals, r_cut = %.17g)\n" % (self.K, self.r_cut))
      for k in range(self.K + 1):
        fh.write("%.17g %.17g %.17g\n" % (r[k], u[k], d[k]))

  def knots(self):
    """(r, U, dU/dr) at the K + 1 knots, fp64; the last knot from interval K - 1 at t = 1."""
    c = self.coeff.astype(_LD)
    r = _LD(self.r0) + np.arange(self.K + 1, dtype=_LD) * _LD(self.h)
    u = np.append(c[:, 0], c[-1].sum())
    d = np.append(c[:, 1], c[-1, 1] + 2 * c[-1, 2] + 3 * c[-1, 3]) / _LD(self.h)
    return r.astype(np.float64), u.astype(np.float64), d.astype(np.float64)

  # ---- evaluation (numpy, fp64): the definition above ----------------------------------------------------------------
  def _locate(self, r):
    r = np.asarray(r, dtype=np.float64)
    x = (r - self.r0) * (1.0 / self.h)
    xc = np.clip(np.where(np.isnan(x), 0.0, x), 0.0, float(self.K))
    k = np.minimum(np.floor(xc), self.K - 1).astype(np.int64)
    t = xc - k
    return r, x, k, t

  def U(self, r):
    r, x, k, t = self._locate(r)
    c = self.coeff[k]
    lead = np.where(x < 0.0, x, t)
    u = c[..., 0] + lead * (c[..., 1] + t * (c[..., 2] + t * c[..., 3]))
    return np.where(r < self.r_cut, u, 0.0)

  def dU(self, r):
    r, x, k, t = self._locate(r)
    c = self.coeff[k]
    du = (c[..., 1] + t * (2.0 * c[..., 2] + 3.0 * t * c[..., 3])) * (1.0 / self.h)
    return np.where(r < self.r_cut, du, 0.0)


def lennard_jones(eps=1.0, sigma=1.0):
  """(U, dU) callables of 4 eps ((sigma/r)^12 - (sigma/r)^6) in the precision of their argument."""
  def U(r):
    s6 = (sigma / r) ** 6
    return 4 * eps * (s6 * s6 - s6)

  def dU(r):
    s6 = (sigma / r) ** 6
    return -24 * eps * (2 * s6 * s6 - s6) / r
  return U, dU


def yukawa(eps=1.0, b=1.0):
  """(U, dU) callables of eps exp(-r/b) / r in the precision of their argument."""
  def U(r):
    return eps * np.exp(-r / b) / r

  def dU(r):
    return -eps * np.exp(-r / b) * (1 / b + 1 / r) / r
  return U, dU
