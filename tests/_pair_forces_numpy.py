"""Extended-precision restatement of the pair LAWS (blob-blob contact force with uniform and per-blob radii, body-body
Yukawa force, the blob and body pair energies), the per-blob scale their rounding bounds are stated against, and the
designed clouds -- TEST infrastructure, written from DESIGN 3.6 / 3.6.1 / 3.9 and forces.py.

  contact:  F_i = sum_j f0 d,  d = r_j - r_i,  f0 = -(eps/b) exp(-(r - c)/b)/r for r > c, else -(eps/b)/max(r, 1e-25),
            c = 2a (law "contact") or a_i + a_j (law "radii")
  yukawa:   f0 = -(eps/b + eps/r) exp(-r/b)/r^2                       (tests/_body_forces_numpy.forces is the same law)
  energies: soft   u2 = r < 2a ? eps + eps (2a - r)/b : eps exp(-(r - 2a)/b)       (minimal image in x and y, all z > 0)
            yukawa u2 = eps exp(-r/b)/r                                            (the same images)
            body   u2 = eps exp(-r/b)/r                                            (minimal image in every direction)
  minimal image d - trunc(d/L + sign(d)/2) L in every direction with L > 0, as the kernels and the oracle do it.

With dtype = EXT (np.longdouble, 64-bit mantissa) the separations of the float64 positions are exact and long double does
not underflow in the range of the laws: every sum is good to ~2^-64 of its scale.

The metric.  Every existing check of these laws is a norm over the whole array, and the laws decay like exp(-(r - c)/b):
a norm sees the pairs within ~27 b of contact and nothing else.  Here every blob is measured against ITS OWN scale

    S_ik = sum_j |f0_ij| (|d_ij,k| w_ij + |n L|_ij,k),        w_ij = 1 + rho_ij / b,

rho_ij = r_ij in open space and the Euclidean norm of the raw separation (before the image is taken) in a box.  w is the
conditioning of the law: one rounding of r, or of d - n L, moves the exponent by rho/b units.  A blob whose every
neighbour is 100 b away is held to 2^-53 of a force of e^-100, not of the largest force of the cloud.  |n L|_k = |raw_k -
d_k| is the part of the raw separation the image removes (0 in open space): the raw difference x_j - x_i is rounded once in
fp64, at the size of raw_k, and that ABSOLUTE error stays on d_k however small d_k is -- beside an axis-aligned neighbour in
contact, periods away, it is the whole error of the component across the axis, and no multiple of |d_k| covers it.  (The
fp64 oracle undoes a shift x + k L bit by bit, because it rounds the product k L as the shift did; an fma does not.)  The
weight w, without that term, per term for the energies (S = sum |u2| w): they depend on r alone.  An absolute floor of one
result-denormal per pair goes on top:

    floor_ik = sum_j (eps/b) tiny |d_k| / r,       tiny = 2^-1074 (2^-126 for the fp32 kernel)

(the kernel's exponential rounds into the denormals and clamps at -750, the hardware exp2 of the fp32 kernel may flush;
long double does neither: design, not error).  The floor only covers a pair whose separation has components that are
exact zeros or not small against r (the product f0 d_k is rounded to the denormal grid once more, which no multiple of
|d_k|/r covers when it is tiny): the designed clouds keep every pair of a blob that has no near neighbour in 695 < x < 752
axis-aligned, and the coverage function asserts it.  Energies: floor = sum_pairs tiny (eps m + 1), m = 1 (soft) or 1/r
(the exponential is rounded to the denormal grid, and so is the product).

    |got - EXT| <= MARGIN * C[law, periodic] * eps_prec * S + floor            MARGIN = _mobility_numpy.MARGIN = 4

C (C32): the worst ratio of the fp64 oracle (of a float32 numpy restatement of the reference's float formula) on these
clouds, measured on the CPU by tests/test_pair_forces_host.py, which asserts measured <= stored <= 2 measured + 1.
Regenerate with    python -m pytest tests/test_pair_forces_host.py -k yardstick -s
They come from the reference side only, never from a kernel."""
import numpy as np

import _body_forces_numpy as bfn
import _potential_numpy as pn
from _mobility_numpy import EXT, LONG_DOUBLE, MARGIN

assert EXT is pn.EXT
A, B, EPS = 0.5, 0.05, 3.92          # a = 1/2: r = 2a is the representable number 1; eps/b = 78.4
EPS_PREC = {64: 2.0 ** -53, 32: 2.0 ** -24}
TINY = {64: EXT(2.0) ** -1074, 32: EXT(2.0) ** -126}
REACH = {64: 750.0, 32: 110.0}       # the culling reach of the kernels in units of b beyond contact
FORCE_LAWS = ("contact", "radii", "yukawa")
ENERGY_FORMS = ("soft", "yukawa", "body")

# (law, periodic) -> worst |oracle_fp64 - EXT| / (2^-53 S) beyond the floor over the designed clouds, rounded up.
# Measured on x86-64 (80-bit long double), gcc -O2 oracle / numpy float64.
C = {
    ("contact", False): 3.0, ("contact", True): 2.0,                  # measured 2.43, 1.50
    ("radii", False): 2.0, ("radii", True): 2.0,                      # 1.96, 1.29
    ("yukawa", False): 3.0, ("yukawa", True): 2.0,                    # 2.54, 1.58
    # energies: the weight 1 + rho/b of a slab pair is 1e3 .. 2e6 (b = 1e-4, 1e-3), the fp64 sum sits far inside it
    ("soft", False): 1.0, ("soft", True): 1.0,                        # 0.012, 0.226
    ("yukawa_energy", False): 1.0, ("yukawa_energy", True): 1.0,      # 0.207, 0.251
    ("body", False): 1.0, ("body", True): 1.0,                        # 0.207, 0.197
}
# float32 restatement in units of 2^-24 S (open boundaries: in a box the option falls back to fp64)
C32 = {"contact": 3.0, "radii": 3.0}                                  # 2.68, 2.04
# the measured values behind the tables, for the record (tools/pair_forces_report.py prints them; the host test measures
# them again and holds the tables to measured <= stored <= 2 measured + 1)
C_MEASURED = {("contact", False): 2.432, ("contact", True): 1.501, ("radii", False): 1.964, ("radii", True): 1.289,
              ("yukawa", False): 2.544, ("yukawa", True): 1.576, ("soft", False): 0.012, ("soft", True): 0.226,
              ("yukawa_energy", False): 0.207, ("yukawa_energy", True): 0.251, ("body", False): 0.207, ("body", True): 0.197,
              ("contact", 32): 2.681, ("radii", 32): 2.036}


# ---------------------------------------------------------------------------------------------------------------------
# laws
# ---------------------------------------------------------------------------------------------------------------------
def _period(L):
  return np.zeros(3) if L is None else np.asarray(L, dtype=np.float64).reshape(3)


def _image(d, L, dtype, dims=(0, 1, 2)):
  for k in dims:
    if L[k] > 0:
      Lk = dtype(L[k])
      d[..., k] = d[..., k] - np.trunc(d[..., k] / Lk + dtype(0.5) * np.sign(d[..., k])) * Lk
  return d


def _rows(x, L, lo, hi, dtype, dims=(0, 1, 2)):
  """d[i, j] = r_j - r_i (minimal image), r, rho (norm of the raw separation) of rows lo..hi; self pairs at r = rho = inf."""
  if dtype == np.float32:       # the fp32 kernels: separations taken exactly from the float64 positions, then float
    raw = x[None, :, :] - x[lo:hi, None, :]
  else:
    raw = (x[None, :, :] - x[lo:hi, None, :]).astype(dtype)
  d = _image(raw.copy(), L, raw.dtype.type, dims).astype(dtype)
  r = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
  rho = np.sqrt(np.sum(raw.astype(EXT) ** 2, axis=-1))
  own = (np.arange(hi - lo), np.arange(lo, hi))
  r[own] = np.inf
  rho[own] = np.inf
  return d, r, rho, raw


def _f0(law, r, c, eps, b, T):
  with np.errstate(all="ignore"):
    if law == "yukawa":
      return -((eps / b) + (eps / r)) * np.exp(-r / b) / (r * r)
    return np.where(r > c, -((eps / b) * np.exp(-(r - c) / b) / r), -((eps / b) / np.maximum(r, T(1e-25))))


def _contact(law, a, radii, lo, hi, dtype, mutant):
  if law == "yukawa":
    return dtype(0)
  if law == "contact":
    return dtype(2) * dtype(a)
  rad = np.asarray(radii, dtype=np.float64).astype(dtype)
  if mutant and mutant.get("two_a_i"):
    return (rad[lo:hi, None] + rad[lo:hi, None]) + dtype(0) * rad[None, :]
  return rad[lo:hi, None] + rad[None, :]


def forces(law, r, L=None, eps=EPS, b=B, a=A, radii=None, dtype=EXT, mutant=None, scale=False, precision=64, block=128):
  """(N, 3) forces of `law` in `dtype` arithmetic; scale=True: (F, S, floor) with S and floor evaluated in EXT.
  mutant (of the law, for the host tests): {"reach": x} drops the pairs beyond (r - c)/b = x, {"drop": (i, j)} one ordered
  pair, {"two_a_i": 1} contacts at 2 a_i, {"no_z_image": 1} takes no image in z."""
  assert law in FORCE_LAWS
  L = _period(L)
  xs = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  x = xs.astype(EXT if dtype == np.float32 else dtype)
  T = dtype
  n = len(x)
  dims = (0, 1) if mutant and mutant.get("no_z_image") else (0, 1, 2)
  F = np.zeros((n, 3), dtype=dtype)
  S = np.zeros((n, 3), dtype=EXT)
  floor = np.zeros((n, 3), dtype=EXT)
  for lo in range(0, n, block):
    hi = min(n, lo + block)
    d, rr, rho, raw = _rows(x, L, lo, hi, dtype, dims)
    c = _contact(law, a, radii, lo, hi, dtype, mutant)
    f0 = _f0(law, rr, c, T(eps), T(b), T)
    f0[np.isinf(rr)] = 0
    if mutant and "reach" in mutant:
      f0 = np.where((rr - c) / T(b) > mutant["reach"], T(0), f0)
    if mutant and "drop" in mutant and lo <= mutant["drop"][0] < hi:
      f0[mutant["drop"][0] - lo, mutant["drop"][1]] = 0
    F[lo:hi] = np.sum(f0[..., None] * d, axis=1)
    if scale:
      assert dtype == EXT
      with np.errstate(invalid="ignore"):
        w = np.where(np.isinf(rr), EXT(0), EXT(1) + rho / EXT(b))
        S[lo:hi] = np.sum((np.abs(f0) * w)[..., None] * np.abs(d) + np.abs(f0)[..., None] * np.abs(raw - d), axis=1)
        floor[lo:hi] = np.sum(np.abs(d) / rr[..., None], axis=1) * (EXT(eps) / EXT(b)) * TINY[precision]
  return (F, S, floor) if scale else F


def pair_x(law, r, L=None, b=B, a=A, radii=None, block=256):
  """x_ij = (r_ij - c_ij)/b (float64, from EXT; +inf on the diagonal) and the components' ratio |d_k|/r (N, N, 3)."""
  L = _period(L)
  x = np.asarray(r, dtype=np.float64).reshape(-1, 3).astype(EXT)
  n = len(x)
  X = np.empty((n, n))
  R = np.empty((n, n))
  U = np.empty((n, n, 3))
  for lo in range(0, n, block):
    hi = min(n, lo + block)
    d, rr, _, _ = _rows(x, L, lo, hi, EXT)
    X[lo:hi] = ((rr - _contact(law, a, radii, lo, hi, EXT, None)) / EXT(b)).astype(np.float64)
    R[lo:hi] = rr.astype(np.float64)
    U[lo:hi] = (np.abs(d) / rr[..., None]).astype(np.float64)
  return X, R, U


def energy(form, r, L=None, eps=EPS, b=B, a=A, dtype=EXT, mutant=None, block=128):
  """(U, S, floor, n_terms) of the pair energy `form` in `dtype`; S = sum |u2| (1 + rho/b) and the floor in EXT.
  mutant: {"reach": x} as above, {"drop": (i, j)} the unordered pair i < j."""
  assert form in ENERGY_FORMS
  L = _period(L)
  x = np.asarray(r, dtype=np.float64).reshape(-1, 3).astype(dtype)
  assert form == "body" or np.all(x[:, 2] > 0)
  T = dtype
  eps_, b_ = T(eps), T(b)
  c = T(2) * T(a) if form == "soft" else T(0)
  n = len(x)
  dims = (0, 1, 2) if form == "body" else (0, 1)
  x64 = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  U, S, floor, count = T(0), EXT(0), EXT(0), 0
  for lo in range(0, n, block):
    hi = min(n, lo + block)
    # float64 first pass: a pair beyond x = 900 is below 2^-1298 of eps in long double, far under the floor; the
    # extended-precision terms are evaluated for the others only
    r64 = np.sqrt(np.sum(_image(x64[None, :, :] - x64[lo:hi, None, :], L, np.float64, dims) ** 2, axis=-1))
    keep = np.arange(n)[None, :] > np.arange(lo, hi)[:, None]
    with np.errstate(divide="ignore"):
      floor = floor + np.where(keep, eps * (1.0 if form == "soft" else 1.0 / r64) + 1.0, 0.0).sum() * TINY[64]
    count += int(keep.sum())
    ii, jj = np.nonzero(keep & ((r64 - float(c)) / b < 900.0))
    if mutant and "drop" in mutant:
      sel = ~((ii + lo == mutant["drop"][0]) & (jj == mutant["drop"][1]))
      ii, jj = ii[sel], jj[sel]
    if not len(ii):
      continue
    raw = x[jj] - x[ii + lo]
    d = _image(raw.copy(), L, T, dims)
    rr = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    rho = np.sqrt(np.sum(raw.astype(EXT) ** 2, axis=-1))
    with np.errstate(all="ignore"):
      if form == "soft":
        t = np.where(rr < c, eps_ + eps_ * (c - rr) / b_, eps_ * np.exp(-np.maximum(rr - c, 0) / b_))
      else:
        t = eps_ * np.exp(-rr / b_) / rr
      if mutant and "reach" in mutant:
        t = np.where((rr - c) / b_ > mutant["reach"], T(0), t)
      U = U + t.sum(dtype=dtype)
      S = S + (np.abs(t).astype(EXT) * (EXT(1) + rho / EXT(b))).sum(dtype=EXT)
  return U, S, floor, count


def yukawa_float64(r, L=None, eps=EPS, b=B):
  """The Yukawa law's fp64 yardstick: tests/_body_forces_numpy.forces in float64 (the body law has no compiled oracle)."""
  return bfn.forces(r, L, eps, b, dtype=np.float64)


def wall_term(z, eps_w, b_w, a, form):
  """u1 of one blob without weight (EXT): the one-blob wall term of tests/_potential_numpy.one_blob_terms."""
  return pn.one_blob_terms(np.atleast_1d(z), EXT(eps_w), EXT(b_w), EXT(0), EXT(a), "soft" if form == "soft" else "yukawa")


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
import contextlib      # noqa: E402
import ctypes          # noqa: E402
import ctypes.util     # noqa: E402


@contextlib.contextmanager
def ieee_denormals():
  """The calling thread in the default floating-point environment (gradual underflow) for the duration.  The -ffast-math
  flavour of the oracle (liboracle_mobility_fast.so) switches the thread that loads it to flush-to-zero / denormals-are-
  zero for the rest of the process; float64 arithmetic and comparisons on denormal results -- half of what these tests are
  about -- would then depend on which test ran before.  The previous environment is put back."""
  libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
  saved = ctypes.create_string_buffer(256)
  libm.fegetenv(saved)
  libm.fesetenv(ctypes.c_void_p(-1))          # FE_DFL_ENV
  try:
    assert float(np.float64(1e-310) * np.float64(1.0)) != 0.0, "float64 denormals are flushed in this thread"
    yield
  finally:
    libm.fesetenv(saved)


def is_positive_zero(x):
  """Bitwise +0.0 (a comparison would call a denormal zero under denormals-are-zero)."""
  return not np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64).any()


def ratios(got, F, S, floor, c, precision=64):
  """(|got - EXT| - floor)+ / (c eps_prec S) per entry (float64); inf where S = 0 and the error exceeds the floor."""
  err = np.maximum(np.abs(np.asarray(got).astype(EXT) - F) - floor, EXT(0))
  den = EXT(c) * EXT(EPS_PREC[precision]) * S
  with np.errstate(divide="ignore", invalid="ignore"):
    q = np.where(err == 0, EXT(0), np.where(den > 0, err / den, EXT(np.inf)))
  return q.astype(np.float64)


def worst(got, F, S, floor, c, precision=64):
  """(worst ratio, blob, component)."""
  q = ratios(got, F, S, floor, c, precision)
  i, k = np.unravel_index(int(np.argmax(q)), q.shape)
  return float(q[i, k]), int(i), int(k)


def rel_err(x, y):
  x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
  return float(np.linalg.norm((x - y).ravel()) / np.linalg.norm(y.ravel()))


# ---------------------------------------------------------------------------------------------------------------------
# designed force clouds
# ---------------------------------------------------------------------------------------------------------------------
CLASSES = ("r<a", "a<=r<2a", "r==2a", "0<x<1", "1..30", "30..110", "110..700", "700..745", "745..750", ">750")
N_CLOUD, N_SUB, N_BIG = 200, 72, 2120
N_EXTRA = 33          # 8 specials + 8 near tails + 4 of the denormal chain + 5 loners + 8 far tails
TARGET_RANGE = (61, 137)


def _lattice(shape, count, spacing, jitter, rng, z0=0.0):
  g = np.stack(np.meshgrid(*[np.arange(m) for m in shape], indexing="ij"), -1).reshape(-1, 3).astype(float)
  g = g[rng.permutation(len(g))[:count]] * spacing
  g += jitter * (2.0 * rng.rand(count, 3) - 1.0)
  g[:, 2] += z0
  return g


def _extras(core, a, b):
  """The designed blobs around a core in x, y, z >= 0 (a = 1/2, b = 0.05 numbers in the comments):
  specials (8): pairs at r < a, a <= r < 2a, r = 2a exactly (integers: exact at 1e6 a and in a power-of-two box), 0 < x < 1
  near tails (8): a 2 x 2 x 2 grid 2.7 apart and 2.7 beyond the core: every neighbour at x > 30
  chain (4) along x, 45 beyond the core in y: neighbours at x = 720 (denormal results), 747.5 and 751.5
  loners (5) at x = -50, 45 apart: every neighbour at x > 750
  far tails (8): a 2 x 2 x 2 grid 7 apart, 7 beyond the near tails: every neighbour at x > 110"""
  s = a / 0.5
  u = b / 0.05
  hi = core.max(axis=0)
  specials = s * np.array([[-4.0, -4.0, 0.0], [-3.0, -4.0, 0.0], [-4.0, -6.0, 0.0], [-3.7, -6.0, 0.1],
                           [-6.0, -4.0, 0.0], [-5.5, -4.0, 0.55], [-8.0, -4.0, 0.0], [-6.98, -4.0, 0.0]])
  grid = np.stack(np.meshgrid([0.0, 1.0], [0.0, 1.0], [0.0, 1.0], indexing="ij"), -1).reshape(-1, 3)
  near = np.array([hi[0] + 2.7 * s, 0.3 * s, 0.0]) + 2.7 * s * grid
  far = np.array([near[:, 0].max() + 7.2 * s, 0.2 * s, 0.0]) + 7.0 * s * grid
  y_chain = max(hi[1], far[:, 1].max()) + 45.0 * s
  steps = np.array([0.0, 2 * a + 720.0 * b, 2 * a + 747.5 * b, 2 * a + 751.5 * b])
  chain = np.zeros((4, 3))
  chain[:, 0] = np.cumsum(steps)
  chain[:, 1] = y_chain
  loners = np.zeros((5, 3))
  loners[:, 0] = -50.0 * s * max(1.0, u)
  loners[:, 1] = 45.0 * s * max(1.0, u) * np.arange(5)
  return specials, near, chain, loners, far


def _shifted(r, L, rng, groups, per_tile):
  """Blobs moved by random whole periods (-2..2) in every periodic direction: one draw per blob, or per 64-blob tile
  (the tile boxes stay compact and the tile gap meets images).  `groups`: index sets that move together in y and z (the
  axis-aligned chain)."""
  n = len(r)
  k = rng.randint(-2, 3, size=(n, 3))
  if per_tile:
    k = rng.randint(-2, 3, size=((n + 63) // 64, 3))[np.arange(n) // 64]
  for g in groups:
    k[g, 1:] = k[g[0], 1:]
  return r + k * L[None, :]


VARIANTS = {
    # name: (periods: 0 open / 2 = x, y / 3 = all, power of two, offset, per-tile moves, classes that cannot exist)
    "open": (0, False, 0.0, False, ()),
    "offset": (0, False, 1.0e6 * A, False, ()),
    "box": (2, False, 0.0, False, ("r==2a",)),          # d - n L is not exact in a non-power-of-two box
    "pow2": (3, True, 0.0, True, ()),
    "box3": (3, False, 0.0, False, ("r==2a",)),
}
_cache = {}


def _build(size, variant, a=A, b=B):
  periods, pow2, offset, per_tile, _ = VARIANTS[variant]
  rng = np.random.RandomState(2500 + size)
  if size == N_BIG:         # a monolayer, listed at random
    core = _lattice((46, 46, 1), N_BIG - N_EXTRA, 1.15 * a / 0.5, 0.1 * a / 0.5, rng, z0=0.6 * a / 0.5)
  else:
    core = _lattice((6, 6, 5), N_CLOUD - N_EXTRA, 1.15 * a / 0.5, 0.1 * a / 0.5, rng)
  core -= core.min(axis=0)
  specials, near, chain, loners, far = _extras(core, a, b)
  if size == N_BIG:
    r = np.concatenate([core, specials, near, chain, loners, far])
    order = rng.permutation(len(r))
    r = r[order]
    chain_at = np.argsort(order)[len(core) + 16 + np.arange(4)]        # argsort(order)[k] = new index of blob k
  else:
    # tiles 0 and 1: core; tile 2: specials, near tails, chain, loners and core; tile 3 (8 blobs): the far tails, a compact
    # tile 7 .. 21 from the core tiles -- inside 2a + 750 b, beyond 2a + 110 b
    r = np.concatenate([core[:128], specials, near, chain, loners, core[128:], far])
    chain_at = 128 + 16 + np.arange(4)
    if size == N_SUB:
      r = r[128:]
      chain_at = chain_at - 128
  r = r + np.array([offset, offset, 0.0])
  L = None
  if periods:
    ext = r.max(axis=0) - r.min(axis=0)
    if pow2:
      L = 2.0 ** np.ceil(np.log2(ext + 45.0 * a / 0.5))
    else:
      L = ext + np.array([47.3, 49.7, 51.1]) * a / 0.5
    if periods == 2:
      L[2] = 0.0
    r = _shifted(r, L, np.random.RandomState(77 + size), [chain_at], per_tile)
  return np.ascontiguousarray(r), L, chain_at


def cloud(size=N_CLOUD, variant="open"):
  """(r, L) of a designed cloud, its coverage asserted once."""
  key = ("cloud", size, variant)
  if key not in _cache:
    r, L, _ = _build(size, variant)
    assert_coverage(coverage("contact", r, L), VARIANTS[variant][4])
    _cache[key] = (r, L)
  return _cache[key]


def radii_of(size):
  """Per-blob radii from [0.5 a, 1.5 a] (the radii law's clouds)."""
  return A * (0.5 + np.random.RandomState(31 + size).rand(size))


def coverage(law, r, L=None, b=B, a=A, radii=None):
  """Pair counts per class of x = (r - c)/b (ordered pairs), the tail blobs (every neighbour at x > 30), the far tails
  (> 110), the loners (> 750; `loners32`: > 110, exact zeros of the fp32 kernel), coincident pairs, and `oblique`: the pairs
  in 695 < x < 752 of a blob without a neighbour below x = 600 that have a component neither exactly zero nor at least
  r / 10 (see the floor in the module docstring)."""
  X, R, U = pair_x(law, r, L, b, a, radii)
  nearest = X.min(axis=1)
  c2 = 2 * a if law == "contact" else None
  cnt = lambda m: int(np.count_nonzero(m))      # noqa: E731
  c = {"0<x<1": cnt((X > 0) & (X < 1)), "1..30": cnt((X >= 1) & (X < 30)), "30..110": cnt((X >= 30) & (X < 110)),
       "110..700": cnt((X >= 110) & (X < 700)), "700..745": cnt((X >= 700) & (X < 745)), "745..750": cnt((X >= 745) & (X < 750)),
       ">750": cnt((X > 750) & np.isfinite(X)), "x<=0": cnt(X <= 0),
       "tail": cnt(nearest > 30), "far_tail": cnt((nearest > 110) & (nearest < 700)), "loner": cnt(nearest > 750), "loner32": cnt(nearest > 110),
       "coincident": cnt(R == 0)}
  if c2 is not None:
    c.update({"r<a": cnt(R < a), "a<=r<2a": cnt((R >= a) & (R < c2)), "r==2a": cnt(R == c2)})
  lonely = nearest > 600
  zone = (X > 695) & (X < 752) & lonely[:, None]
  c["oblique"] = cnt(zone[..., None] & (U != 0) & (U < 0.1))
  return c


def assert_coverage(c, absent=(), tails=8, loners=4):
  missing = [k for k in CLASSES if k not in absent and k in c and c[k] < 1]
  assert not missing, (missing, c)
  assert c["tail"] - c["loner"] >= tails and c["far_tail"] >= 4 and c["loner"] >= loners and c["coincident"] == 0 and c["oblique"] == 0, c


def loners(law, r, L=None, b=B, a=A, radii=None, precision=64):
  """Indices of the blobs whose every neighbour lies beyond the culling reach: exact zeros of the kernel."""
  X, _, _ = pair_x(law, r, L, b, a, radii)
  return np.nonzero(X.min(axis=1) > REACH[precision])[0]


def reference(law, size, variant, precision=64):
  """(F, S, floor) in EXT of a designed cloud, once per process."""
  key = ("ref", law, size, variant, precision)
  if key not in _cache:
    r, L = cloud(size, variant)
    _cache[key] = forces(law, r, L, radii=radii_of(size) if law == "radii" else None, scale=True, precision=precision)
  return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# N = 2 ladder
# ---------------------------------------------------------------------------------------------------------------------
LADDER = (-1.0, 0.0, 0.5, 30.5, 109.0, 111.0, 700.0, 744.0, 751.0)
LADDER_RADII = (0.375, 0.625)          # a_i + a_j = 1 = 2a exactly
LADDER_BOX = np.array([128.0, 128.0, 0.0])


def ladder_pair(x, contact=2 * A, b=B, box=False):
  """Two blobs along the x axis at (r - contact)/b = x, above z = 0 (x = 0: r = contact exactly); box: LADDER_BOX, the
  second blob two periods further in x and one back in y (exact: powers of two)."""
  r = np.array([[0.0, 0.0, 1.0], [contact + x * b, 0.0, 1.0]])
  if box:
    r[1, 0] += 2 * LADDER_BOX[0]
    r[1, 1] -= LADDER_BOX[1]
  return r


def ladder(law_or_form):
  """The rungs that exist for a law: the Yukawa forms have no contact distance (x = r/b > 0)."""
  return tuple(x for x in LADDER if x > 0) if law_or_form in ("yukawa", "body") else LADDER


# ---------------------------------------------------------------------------------------------------------------------
# energy clouds: slab pairs
# ---------------------------------------------------------------------------------------------------------------------
BANDS = ((1, 20), (90, 110), (400, 420), (700, 740), (752, 760))
SLAB = dict(a=0.5, spacing=1.2, eps=1.7, b={"soft": 1.0e-4, "yukawa": 1.0e-3, "body": 1.0e-3})
N_SLAB, N_SLAB_BIG = 136, 2176
SLAB_BOX = np.array([211.3, 197.9, 167.3])


def _slab_pair(band, form, rng):
  """Tile A: a 4 x 4 x 4 lattice (every internal pair beyond the reach: 0.2 = 2000 b soft, 1.2 = 1200 b yukawa); tile B: A
  shifted along x so that the 16 blobs of A's +x face meet the 16 of B's -x face at x = band centre -2 .. +2 (jitter in x)."""
  b = SLAB["b"][form]
  c = 2 * SLAB["a"] if form == "soft" else 0.0
  g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3) * SLAB["spacing"]
  mid = 0.5 * (band[0] + band[1])
  Bt = g + np.array([3 * SLAB["spacing"] + c, 0.0, 0.0])
  Bt[:, 0] += (mid - 2.0 + 4.0 * rng.rand(64)) * b
  return g, Bt


def slab_cloud(band, form, big=False, box=False):
  """(r, L): one slab pair and 8 loners (136 blobs), or 17 slab pairs 20 apart with 8 blobs of the last tile B's far face
  made loners (2176 blobs: the sorted path), all z > 0.  box: SLAB_BOX (z period for the body form only), every tile B a whole
  number of periods further."""
  key = ("slab", band, form, big, box)
  if key in _cache:
    return _cache[key]
  rng = np.random.RandomState(900 + 7 * BANDS.index(band) + (3 if big else 0))
  L = None
  if box:
    L = SLAB_BOX.copy()
    if form != "body":
      L[2] = 0.0
  parts = []
  for p in range(17 if big else 1):
    At, Bt = _slab_pair(band, form, rng)
    origin = np.array([20.0 * (p % 5), 20.0 * (p // 5), 0.0])
    if box:
      Bt = Bt + L * np.array([1 + p % 2, -(p % 3), 1 if form == "body" else 0])
    parts += [At + origin, Bt + origin]
  if big:
    far_face = np.argsort(-(parts[-1][:, 0]))[:8]
    parts[-1] = np.delete(parts[-1], far_face, axis=0)
  lon = np.zeros((8, 3))
  lon[:, 0] = -30.0
  lon[:, 1] = 12.0 * np.arange(8)
  r = np.concatenate(parts + [lon])
  r[:, 2] += 0.75
  if big:
    r = r[rng.permutation(len(r))]
  assert len(r) == (N_SLAB_BIG if big else N_SLAB)
  _cache[key] = (np.ascontiguousarray(r), L)
  return _cache[key]


def slab_coverage(band, form, big=False, box=False):
  """Asserts the design of a slab cloud: 16 facing pairs per slab pair inside the band and within e^-21 of each other, every
  other pair beyond x = 750.  Returns the list of facing pairs (i < j)."""
  r, L = slab_cloud(band, form, big, box)
  b = SLAB["b"][form]
  x = np.asarray(r).astype(EXT)
  n = len(x)
  facing = []
  dims = (0, 1, 2) if form == "body" else (0, 1)
  c = 2 * SLAB["a"] if form == "soft" else 0.0
  x64 = np.asarray(r, dtype=np.float64)
  for lo in range(0, n, 256):
    hi = min(n, lo + 256)
    r64 = np.sqrt(np.sum(_image(x64[None, :, :] - x64[lo:hi, None, :], _period(L), np.float64, dims) ** 2, axis=-1))
    r64[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
    ii, jj = np.nonzero((r64 - c) / b < 800.0)          # float64 first pass; the classes from long double
    if not len(ii):
      continue
    d = _image(x[jj] - x[ii + lo], _period(L), EXT, dims)
    X = ((np.sqrt(np.sum(d * d, axis=-1)) - EXT(c)) / EXT(b)).astype(np.float64)
    near = X <= 750.0
    assert np.all((X[near] > band[0]) & (X[near] < band[1])) and (band[0] < 750 or not near.any()), (band, form, X.min(), X.max())
    facing += [(int(i + lo), int(j), float(v)) for i, j, v in zip(ii[near], jj[near], X[near]) if i + lo < j]
  pairs = 17 if big else 1
  if band[0] > 750:
    assert not facing
    return []
  assert len(facing) == 16 * pairs, (band, form, len(facing))
  xs = np.array([f[2] for f in facing])
  assert xs.max() - xs.min() < 20.0 and band[1] - band[0] <= 40
  return facing


def slab_reference(band, form, big=False, box=False):
  """(U, S, floor) in EXT, once per process."""
  key = ("slab_ref", band, form, big, box)
  if key not in _cache:
    r, L = slab_cloud(band, form, big, box)
    _cache[key] = energy(form, r, L, SLAB["eps"], SLAB["b"][form], SLAB["a"])[:3]
  return _cache[key]


def energy_ratio(got, U, S, floor, c):
  err = max(abs(EXT(got) - U) - floor, EXT(0))
  if err == 0:
    return 0.0
  return float(err / (EXT(c) * EXT(EPS_PREC[64]) * S)) if S > 0 else float("inf")
