"""Bond-orientational order without a GPU: the numpy restatement on lattices (_bond_order_numpy.py), the fp64 restatement inside
the derived bound, quantise, the argument checks of the two C entries with a null context, the Python and command-line argument
errors, the table's write / parse round trip, and the agreement of header, library and ctypes table on the two new names."""
import ctypes
import os
import re

import numpy as np
import pytest

import _bond_order_numpy as bo
import _pair_hist_numpy as phnp
from rigidmultiblobswall_amd import bondorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (4, 6, 12)


def _lattice_tol(pts, a, m):
  """the lattice's own coordinates are rounded: a bond vector is off by at most 4 u max|x|, its angle by that over a, z^m by m times"""
  return m * 4 * bo.U * np.abs(pts).max() / a * 2


def test_triangular_and_square_lattices():
  pts, L = bo.triangular_lattice(8, 8, 1.25)
  assert bo.cut_margin(pts, L, 1.3 * 1.25) > 0.1
  N, S, _ = bo.neighbour_sums(pts, L, 1.3 * 1.25, ORDERS)
  psi = bo.psi_of(N, S)[0]
  assert np.all(N == 6)
  assert np.all(np.abs(psi[:, 0]) <= _lattice_tol(pts, 1.25, 4))
  assert np.all(np.abs(np.abs(psi[:, 1]) - 1) <= _lattice_tol(pts, 1.25, 6)) and np.all(np.abs(np.abs(psi[:, 2]) - 1) <= _lattice_tol(pts, 1.25, 12))
  pts, L = bo.square_lattice(7, 9, 0.75)
  N, S, _ = bo.neighbour_sums(pts, L, 1.2 * 0.75, ORDERS)
  psi = bo.psi_of(N, S)[0]
  assert np.all(N == 4) and np.all(np.abs(psi[:, 1]) <= 1e-15)
  assert np.allclose(psi[:, 0], 1.0, rtol=0, atol=1e-15) and np.allclose(psi[:, 2], 1.0, rtol=0, atol=1e-15)
  # a rotation of the lattice by alpha turns psi_m by exp(i m alpha) and leaves |psi_m| alone (open box: the rotated one has no period)
  alpha = 0.3
  R = np.array([[np.cos(alpha), -np.sin(alpha), 0], [np.sin(alpha), np.cos(alpha), 0], [0, 0, 1]])
  big, _ = bo.square_lattice(5, 5, 1.0)
  N0, S0, _ = bo.neighbour_sums(big, np.zeros(3), 1.2, (4,))
  N1, S1, _ = bo.neighbour_sums(big @ R.T, np.zeros(3), 1.2, (4,))
  assert np.array_equal(N0, N1) and N0[0, 12] == 4 and N0[0, 0] == 2
  assert np.allclose(bo.psi_of(N1, S1), bo.psi_of(N0, S0) * np.exp(4j * alpha), rtol=0, atol=1e-14)


def test_stacked_points_planes_and_images():
  L = np.array([4.0, 4.0, 0.0])
  # two stacked points and a third: the stacked pair has no angle under either plane
  pts = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.5], [1.75, 1.0, 0.0]])
  for plane in ("xy", "xyz"):      # under xyz the stacked pair is 0.5 apart, inside the cutoff, and still left out: rho = 0
    N, S, _ = bo.neighbour_sums(pts, L, 1.0, (1,), plane)
    assert N.tolist() == [[1, 1, 2]] and np.allclose(S[0, 0, 0].astype(float), [-1.0, 0.0], rtol=0, atol=1e-18)      # sin(pi) in long double
  N, S, _ = bo.neighbour_sums(pts, L, 0.8, (1,), "xyz")      # |(0.75, 0, 0.5)| = 0.90 > 0.8: the raised point loses its neighbour
  assert N.tolist() == [[1, 0, 1]]
  # a pair across the box edge, any number of periods away
  pts = np.array([[0.125, 2.0, 0.0], [3.875 + 3 * 4.0, 2.0 - 5 * 4.0, 0.0]])
  N, S, ratio = bo.neighbour_sums(pts, L, 0.5, (1, 2), "xy")
  assert N.tolist() == [[1, 1]] and np.allclose(S[0, 0, :, 0].astype(float), [1.0, 1.0]) and np.allclose(S[0, 1, :, 0].astype(float), [-1.0, 1.0])
  assert ratio[0, 0] == 20.0 / 0.25
  assert bo.neighbour_sums(pts, np.zeros(3), 0.5, (1,), "xy")[0].tolist() == [[0, 0]]


def test_fp64_numpy_sits_inside_the_bound():
  """the bound the GPU test demands is reachable: the kernel's arithmetic in fp64 numpy against long double with true trigonometry"""
  worst = 0.0
  L = np.array([7.0, 5.0, 3.0])
  for n, seed, shift in ((65, 1, 0.0), (130, 2, 0.0), (130, 3, 1000.0)):
    make = lambda rng: rng.uniform(0, 1, (2, n, 3)) * L + shift * L * rng.randint(-1, 2, (2, n, 3))      # noqa: E731
    for plane in ("xy", "xyz"):
      frames = bo.frames_with_margin(make, L, 1.1, plane, seed=seed)
      orders = (1, 4, 6, 16)
      N, S, ratio = bo.neighbour_sums(frames, L, 1.1, orders, plane)
      N64, S64 = bo.neighbour_sums_fp64(frames, L, 1.1, orders, plane)
      bound = bo.sum_bound(N, ratio, orders)
      assert np.array_equal(N, N64) and N.max() >= 3
      err = np.abs(S64.astype(bo.EXT) - S).max(axis=-1).astype(np.float64)
      assert np.all(err <= bound)
      worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
  assert 0.0 < worst < 1.0


def test_quantise():
  q = bondorder.quantise(np.array([1.0 + 0j, -1j, 0.5 - 0.25j, 0j]))
  assert q.dtype == np.int32 and q.tolist() == [[2 ** 30, 0], [0, -2 ** 30], [2 ** 29, -2 ** 28], [0, 0]]
  assert bondorder.quantise(np.array([[1.5 * 2.0 ** -30, 2.5 * 2.0 ** -30]])).tolist() == [[2, 2]]      # halves to even
  assert bondorder.quantise(np.array([[1.0 + 2.0 ** -52, -1.0]])).tolist() == [[2 ** 30, -2 ** 30]]      # a unit of roundoff past 1
  assert bondorder.quantise(np.zeros((0, 2))).shape == (0, 2)
  for bad in (np.array([1.0 + 1e-9 + 0j]), np.array([[0.0, np.nan]])):
    with pytest.raises(ValueError, match="unit square"):
      bondorder.quantise(bad)
  with pytest.raises(ValueError, match="complex"):
    bondorder.quantise(np.zeros((3, 3)))
  # a quantised term is within (sqrt(2) + 1/2) 2^-30 of the unquantised one, and so is every bin mean: each psi moves by at most
  # sqrt(2) 2^-31 against a factor of at most 1, and the shift rounds to half a unit of 2^-30
  rng = np.random.RandomState(0)
  psi = (rng.uniform(-1, 1, 400) + 1j * rng.uniform(-1, 1, 400)) / np.sqrt(2)
  f = bondorder.quantise(psi).astype(np.int64)
  i, j = np.triu_indices(400, 1)
  term = (f[i, 0] * f[j, 0] + f[i, 1] * f[j, 1] + (1 << 29)) >> 30
  exact = (psi[i] * np.conj(psi[j])).real
  assert np.max(np.abs(term / 2.0 ** 30 - exact)) <= (np.sqrt(2.0) + 0.5) * 2.0 ** -30
  assert bondorder.g_from_sums([term.sum(), 0], [term.size, 0])[0] == term.sum() / (2.0 ** 30 * term.size)
  assert np.isnan(bondorder.g_from_sums([0], [0])[0])


def test_pair_field_restatement():
  rng = np.random.RandomState(5)
  L = np.array([6.0, 5.0, 0.0])
  frames = rng.uniform(0, 1, (3, 40, 3)) * np.array([6.0, 5.0, 2.0])
  for plane in ("xy", "xyz"):
    ones = np.zeros((3, 40, 2), dtype=np.int32)
    ones[..., 0] = 2 ** 30
    counts, sums = bo.pair_field(frames, ones, L, 2.0, 16, plane)
    assert np.array_equal(sums, counts * 2 ** 30) and counts.sum() > 0
    f3, L3 = bo._in_plane(frames, L, plane)
    assert np.array_equal(counts, phnp.counts(f3, L3, 2.0, 16).astype(np.int64))
    fld = bo.random_field(rng, (3, 40))
    assert np.abs(fld).max() == 2 ** 30 and (fld == 0).any()
    c1, s1 = bo.pair_field(frames, fld, L, 2.0, 16, plane)
    perm = rng.permutation(40)
    c2, s2 = bo.pair_field(frames[:, perm], fld[:, perm], L, 2.0, 16, plane)
    assert np.array_equal(c1, c2) and np.array_equal(s1, s2) and np.array_equal(c1, counts)
  # (-2^30)^2 + (-2^30)^2 = 2^61: the term 2^31 fits
  two = np.array([[[0.0, 0, 0], [1.0, 0, 0]]])
  assert bo.pair_field(two, np.full((1, 2, 2), -2 ** 30, dtype=np.int32), np.zeros(3), 2.0, 1)[1].tolist() == [2 ** 31]
  assert bo.pair_field(two, np.array([[[3, 0], [-1, 0]]], dtype=np.int32), np.zeros(3), 2.0, 1)[1].tolist() == [0]      # (-3 + 2^29) >> 30


def _declared():
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rmb_mobility.h")).read(), flags=re.S)
  return sorted(set(re.findall(r"\b(rmb_[a-z0-9_]+)\s*\(", src)))


def test_header_library_and_ctypes_table_agree():
  from rigidmultiblobswall_amd import _lib
  names = _declared()
  lib = ctypes.CDLL(_lib.LIB_PATH)
  assert len(names) == len(_lib.SYMBOLS) == sum(hasattr(lib, n) for n in names)
  for name in ("rmb_bond_order_frames_device", "rmb_pair_field_frames_device"):
    assert name in names and name in _lib.SYMBOLS and hasattr(lib, name)


def test_c_entries_refuse_bad_arguments_without_a_device():
  """Every argument check comes before the context is looked at."""
  from rigidmultiblobswall_amd import _lib
  lib, ARG = _lib.load(), -1      # RMB_ERR_ARG
  buf, L = np.zeros(3 * 2 * 3), np.array([4.0, 3.0, 0.0])
  orders, out = np.array([4, 6], dtype=np.int32), np.zeros(3 * 2 * 5)
  field, counts, sums = np.zeros(3 * 2 * 2, dtype=np.int32), np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.int64)
  p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
  good = dict(frames=p(buf), n_frames=3, n=2, L=p(L), r_cut=1.5, plane=1, orders=p(orders), n_orders=2, chunk=0, out=p(out),
              field=p(field), r_max=1.5, n_bins=16, counts=p(counts), sums=p(sums))
  shared = [(dict(n_frames=-1), "negative size"), (dict(n=-1), "negative size"), (dict(frames=None), "null frames"),
            (dict(L=None), "null periodic_length"), (dict(plane=2), "plane must be"), (dict(plane=-1), "plane must be")]
  bad_r = lambda k, msg: [(dict([(k, v)]), msg) for v in (0.0, -1.0, float("inf"), float("nan"))]      # noqa: E731
  calls = {
      "rmb_bond_order_frames_device": (lambda a: (a["frames"], a["n_frames"], a["n"], a["L"], a["r_cut"], a["plane"], a["orders"], a["n_orders"],
                                                  a["chunk"], a["out"]),
                                       shared + bad_r("r_cut", "r_cut must be positive and finite") +
                                       [(dict(orders=None), "null orders"), (dict(n_orders=0), "n_orders must be 1 ... 4"),
                                        (dict(n_orders=5), "n_orders must be 1 ... 4"), (dict(chunk=-1), "source_chunk must not be negative"),
                                        (dict(out=None), "null output"), (dict(orders=p(np.array([4, 17], dtype=np.int32))), "every order must be 1 ... 16"),
                                        (dict(orders=p(np.array([0, 6], dtype=np.int32))), "every order must be 1 ... 16")]),
      "rmb_pair_field_frames_device": (lambda a: (a["frames"], a["field"], a["n_frames"], a["n"], a["L"], a["plane"], a["r_max"], a["n_bins"],
                                                  a["counts"], a["sums"]),
                                       shared + bad_r("r_max", "r_max must be positive and finite") +
                                       [(dict(field=None), "null field"), (dict(counts=None), "null counts or sums"), (dict(sums=None), "null counts or sums"),
                                        (dict(n_bins=0), "n_bins must be 1 ... 4096"), (dict(n_bins=4097), "n_bins must be 1 ... 4096"),
                                        (dict(n_frames=2 ** 34, n=2 ** 19), "too many pairs for one launch")]),
  }
  header = open(os.path.join(ROOT, "include", "rmb_mobility.h")).read()
  for name, (args, cases) in calls.items():
    assert ("int %s(" % name) in header
    fn = getattr(lib, name)
    for change, message in cases + [(dict(), "null context")]:
      rc = fn(None, *args(dict(good, **change)))
      assert rc == ARG, (name, change)
      assert message in lib.rmb_last_error().decode(), (name, change, lib.rmb_last_error())
  assert not out.any() and not counts.any() and not sums.any()


def test_python_argument_errors():
  L = (4.0, 3.0, 0.0)
  B = bondorder.BondOrder
  cases = [(dict(r_cut=None), "r_cut must be positive"), (dict(r_cut=-1.0), "r_cut must be positive"), (dict(r_cut=float("inf")), "r_cut must be positive"),
           (dict(orders=()), "orders must be"), (dict(orders=(1, 2, 3, 4, 5)), "orders must be"), (dict(orders=(17,)), "orders must be"),
           (dict(orders=(0,)), "orders must be"), (dict(orders=(6.5,)), "orders must be"), (dict(plane="xz"), "plane must be"),
           (dict(n_bins=4097), "n_bins must be"), (dict(n_bins=-1), "n_bins must be"), (dict(n_bins=4, r_max=0.0), "r_max must be positive"),
           (dict(n_lags=-1), "n_lags must not be negative"), (dict(origins="some"), "origins must be"), (dict(ctx=object()), "single-GPU MobilityContext")]
  for kw, message in cases:
    with pytest.raises(ValueError, match=message):
      B(3, L, **dict(dict(r_cut=1.0), **kw))
  with pytest.raises(ValueError, match="n_points"):
    B(-1, L, r_cut=1.0)
  with pytest.raises(ValueError, match="three lengths"):
    B(3, (4.0, 3.0), r_cut=1.0)
  with pytest.raises(ValueError, match="positive period in the plane"):
    B(3, (0.0, 0.0, 5.0), r_cut=1.0, n_bins=4)


def test_command_line_argument_errors(tmp_path, capsys):
  traj = tmp_path / "run.config"
  traj.write_text(phnp.config_text(np.zeros((3, 2, 3))))
  base = [str(traj), "2", "4.0", "3.0", "0.0"]
  cases = [(base, "--rcut"), (base + ["--rcut", "0"], "--rcut must be positive"), (base + ["--rcut", "1", "--orders", "4,x"], "comma-separated integers"),
           (base + ["--rcut", "1", "--orders", "4,17"], "orders must be"), (base + ["--rcut", "1", "--orders", "1,2,3,4,5"], "orders must be"),
           (base + ["--rcut", "1", "--plane", "xz"], "invalid choice"), (base + ["--rcut", "1", "--origins", "some"], "invalid choice"),
           (base + ["--rcut", "1", "--bins", "5000"], "0 ... 4096"), (base + ["--rcut", "1", "--bins", "4", "--rmax", "-1"], "--rmax must be positive"),
           (base + ["--rcut", "1", "--every", "0"], "at least 1"), (base + ["--rcut", "1", "--lags", "-1"], "must not be negative"),
           ([str(traj), "2", "0.0", "0.0", "0.0", "--rcut", "1", "--bins", "4"], "--rmax is needed"),
           ([str(traj), "3", "4.0", "3.0", "0.0", "--rcut", "1"], "whole number of frames"), (base + ["--rcut", "1", "--skip", "3"], "no frame left")]
  for argv, message in cases:
    with pytest.raises(SystemExit) as exc:
      bondorder.main(argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err, argv


class _Table(bondorder.BondOrder):
  """format() on hand-made results: no context"""

  def __init__(self, orders, n_bins, lags):      # noqa: super().__init__ would open a device
    rng = np.random.RandomState(2)
    K = len(orders)
    self.orders, self.n_bins, self.lags, self.n_lags = orders, n_bins, lags, max(lags, 1)
    self.n_frames, self.n, self.plane, self.r_cut, self.r_max, self.dt = 7, 11, "xy", 1.3, 2.5, 0.25
    self._nc = np.array([0, 3, 10, 64], dtype=np.int64)
    self.vals = dict(mean=rng.uniform(0, 1, K), glob=rng.uniform(0, 1, K), counts=rng.randint(0, 2 ** 40, (K, n_bins)),
                     g=rng.uniform(-1, 1, (K, n_bins)), C=rng.uniform(-1, 1, (K, lags)))
    self._origins = np.arange(lags, 0, -1).astype(np.int64)

  def mean_abs_psi(self):
    return self.vals["mean"]

  def global_order(self):
    return self.vals["glob"]

  def g_n(self):
    return self.r(), self.vals["g"], self.vals["counts"][0]

  def C_n(self):
    return self.dt * np.arange(self.lags), self.vals["C"]


@pytest.mark.parametrize("orders,n_bins,lags", [((6,), 0, 0), ((4, 6), 5, 0), ((4, 6, 12), 0, 3), ((1, 4, 6, 16), 4, 2)])
def test_table_round_trip(tmp_path, orders, n_bins, lags):
  acc = _Table(orders, n_bins, lags)
  path = tmp_path / "bo.dat"
  acc.write(str(path))
  d = bondorder.parse(path.read_text())
  assert d["orders"] == orders and d["n_frames"] == 7 and d["n_points"] == 11 and d["plane"] == "xy" and d["r_cut"] == 1.3
  assert np.array_equal(d["mean_abs_psi"], acc.vals["mean"]) and np.array_equal(d["global_order"], acc.vals["glob"])
  assert np.array_equal(d["neighbours"], [0, 3, 10, 64])
  if n_bins:
    assert np.array_equal(d["r"], acc.r()) and np.array_equal(d["counts"], acc.vals["counts"][0]) and np.array_equal(d["g"], acc.vals["g"])
  else:
    assert "g" not in d
  if lags:
    assert np.array_equal(d["t"], 0.25 * np.arange(lags)) and np.array_equal(d["n_origins"], acc._origins) and np.array_equal(d["C"], acc.vals["C"])
  else:
    assert "C" not in d
  with pytest.raises(ValueError, match="not a bond-order table"):
    bondorder.parse("1 2 3\n")
