"""The HIP cluster sweep (rmb_cluster_labels_frames_device, rmb_cluster_labels_device, cluster_kernels.h) against the numpy
restatement (_clusters_numpy.py).

Every comparison is EXACT equality of integers: labels and sizes.  That is a fair demand because every random input satisfies,
and every case asserts, the precondition: in long double no pair has r^2 within 1e-9 r_cut^2 of r_cut^2 (bond_margin), while
the fp64 error of r^2 is ~1e-15 relative.  The designed ties sit on dyadic coordinates, where r^2 is exact in any evaluation
order.  Inputs and references are computed once and shared."""
import numpy as np
import pytest
import torch

import _clusters_numpy as cn
from rigidmultiblobswall_amd._lib import RmbError

pytestmark = pytest.mark.gpu

BOX = np.array([9.0, 7.0, 5.0])
MODES = {"open": (0, 0, 0), "xy": (1, 1, 0), "xyz": (1, 1, 1)}
PLANES = ("xy", "xyz")
SIZES = (1, 2, 63, 64, 65, 129, 200)
CHUNK_STEPS = (0, 4, 28, 1024)
OVERSUB = (1, 8)
DEFAULTS = {"sym_chunk_steps": 1024, "sym_oversub": 8}
_CASES, _REFS = {}, {}


def cloud_r_cut(n, plane):
  """Bond length for n uniform points in BOX that gives a broad size distribution: a mean of 1.8 bonds per point in the plane
  (continuum percolation sets in at 4.5) and of 1.3 in 3-D (2.7).  The same for n < 63, where the points are drawn close together."""
  n = max(n, 63)
  if plane == "xy":
    return float(np.sqrt(1.8 * BOX[0] * BOX[1] / (np.pi * n)))
  return float(np.cbrt(1.3 * BOX.prod() * 3.0 / (4.0 * np.pi * n)))


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  assert {k: c.get_option(k) for k in DEFAULTS} == DEFAULTS
  yield c
  c.close()


class _plan:
  """the two plan options for the length of a with block (as test_gpu_pair_once_schedule.py)"""

  def __init__(self, ctx, chunk_steps, oversub):
    self.ctx, self.values = ctx, {"sym_chunk_steps": chunk_steps, "sym_oversub": oversub}

  def __enter__(self):
    for k, v in self.values.items():
      self.ctx.set_option(k, v)

  def __exit__(self, *exc):
    for k, v in DEFAULTS.items():
      self.ctx.set_option(k, v)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _margin_ok(frames, L, cuts):
  return all(cn.bond_margin(frames, L, r, p) > cn.MARGIN for p, r in cuts.items())


def _cloud(n, mode, F=1):
  """frames (F, n, 3), L: uniform points in BOX, every point moved by -2 ... 2 periods in the periodic directions (five periods
  in x and y); n <= 2: drawn within (0.5, 0.5, 0.3) so that the two points are bonded.  The margin holds for both planes' r_cut."""
  if (n, mode, F) not in _CASES:
    L = BOX * np.asarray(MODES[mode], dtype=np.float64)
    span = BOX if n > 2 else np.array([0.5, 0.5, 0.3])
    cuts = {p: cloud_r_cut(n, p) for p in PLANES}
    for seed in range(1000 * n + F, 1000 * n + F + 20):
      rng = np.random.RandomState(seed)
      frames = rng.uniform(0, 1, (F, n, 3)) * span + rng.randint(-2, 3, (F, n, 3)) * L
      if _margin_ok(frames, L, cuts):
        break
    else:
      pytest.fail("no seed keeps every pair off the bond length")
    assert _margin_ok(frames, L, cuts)
    _CASES[(n, mode, F)] = (frames, L)
  return _CASES[(n, mode, F)]


def _ref(key, frames, L, r_cut, plane, select=None):
  if (key, plane) not in _REFS:
    _REFS[(key, plane)] = cn.labels_sizes(frames, L, r_cut, plane, select)
  return _REFS[(key, plane)]


def _run(ctx, frames, L, r_cut, plane, select=None):
  f = np.asarray(frames, dtype=np.float64)
  f = f.reshape(-1, f.shape[-2], 3)
  sel = None if select is None else torch.from_numpy(np.ascontiguousarray(select).reshape(f.shape[:2])).cuda()
  labels, sizes = ctx.cluster_labels_frames_device(_dev(f), L, r_cut, plane=plane, select=sel)
  for t in (labels, sizes):
    assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == f.shape[:2]
  return labels.cpu().numpy(), sizes.cpu().numpy()


def _same(got, ref):
  assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", SIZES)
def test_clouds_against_the_restatement(ctx, n, mode):
  frames, L = _cloud(n, mode)
  for plane in PLANES:
    r_cut = cloud_r_cut(n, plane)
    ref = _ref(("cloud", n, mode), frames, L, r_cut, plane)
    _same(_run(ctx, frames, L, r_cut, plane), ref)
    if n >= 63:      # a broad distribution: the case is not one blob and not a gas
      assert np.count_nonzero(ref[1] >= 3) >= 3 and np.count_nonzero(ref[1] == 1) >= 3
    elif n == 2:
      assert ref[0].tolist() == [[0, 0]] and ref[1].tolist() == [[2, 0]]
    else:
      assert ref[0].tolist() == [[0]] and ref[1].tolist() == [[1]]


def _chain_positions():
  """200 points one apart along x: with r_cut 1.25 only consecutive members are bonded (the next-nearest are 2 apart)"""
  x = np.zeros((200, 3))
  x[:, 0] = np.arange(200.0)
  x[:, 1:] = (1.5, 0.25)
  return x


CHAIN_R_CUT = 1.25
CHAIN_L = {"open": np.zeros(3), "xy": np.array([512.0, 512.0, 0.0]), "xyz": np.array([512.0, 512.0, 512.0])}


def _chain_orders():
  return {"in_order": np.arange(200), "reverse": np.arange(200)[::-1].copy(), "random": np.random.RandomState(5).permutation(200)}


def _indexed(pos, idx):
  """chain member c gets index idx[c]"""
  out = np.empty_like(pos)
  out[idx] = pos
  return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("order", ["in_order", "reverse", "random"])
def test_chains(ctx, order, mode):
  """deep trees, hooks between roots owned by different workgroups: one cluster of 200, label 0"""
  x, L = _indexed(_chain_positions(), _chain_orders()[order]), CHAIN_L[mode]
  for plane in PLANES:
    assert cn.bond_margin(x, L, CHAIN_R_CUT, plane) > 0.3
    ref = _ref(("chain", order, mode), x, L, CHAIN_R_CUT, plane)
    assert np.all(ref[0] == 0) and ref[1][0, 0] == 200 and cn.bonds(x, L, CHAIN_R_CUT, plane).sum() == 2 * 199
    _same(_run(ctx, x, L, CHAIN_R_CUT, plane), ref)


@pytest.mark.parametrize("order", ["in_order", "random"])
def test_two_chains_joined_only_across_the_periodic_boundary(ctx, order):
  """not a closed ring: two chains of 100, 1.5 apart, whose far ends meet only through the image (0.75 apart across Lx = 200.25): one cluster in
  the periodic box, two in the open one"""
  x = _chain_positions()
  x[100:, 0] += 0.5
  x = _indexed(x, _chain_orders()[order])
  for mode, n_clusters in (("open", 2), ("xy", 1), ("xyz", 1)):
    L = np.array([200.25, 64.0, 64.0]) * np.asarray(MODES[mode], dtype=np.float64)
    for plane in PLANES:
      assert cn.bond_margin(x, L, CHAIN_R_CUT, plane) > 0.3
      ref = _ref(("image_joined", order, mode), x, L, CHAIN_R_CUT, plane)
      assert np.count_nonzero(ref[1]) == n_clusters
      _same(_run(ctx, x, L, CHAIN_R_CUT, plane), ref)


@pytest.mark.parametrize("order", ["in_order", "random"])
def test_ring_closed_only_across_the_periodic_boundary(ctx, order):
  """the chain of 200 in a box of Lx = 200: members 199 and 0 are 1 apart through the image, which closes the chain to a ring of
  200 bonds; in the open box it stays a chain of 199"""
  x = _indexed(_chain_positions(), _chain_orders()[order])
  for mode, n_bonds in (("open", 199), ("xy", 200), ("xyz", 200)):
    L = np.array([200.0, 64.0, 64.0]) * np.asarray(MODES[mode], dtype=np.float64)
    for plane in PLANES:
      assert cn.bond_margin(x, L, CHAIN_R_CUT, plane) > 0.3 and cn.bonds(x, L, CHAIN_R_CUT, plane).sum() == 2 * n_bonds
      ref = _ref(("ring", order, mode), x, L, CHAIN_R_CUT, plane)
      assert np.all(ref[0] == 0)
      _same(_run(ctx, x, L, CHAIN_R_CUT, plane), ref)


@pytest.mark.parametrize("mode", list(MODES))
def test_two_chains_joined_at_their_largest_indices(ctx, mode):
  """chain A (indices 0 ... 99) along x, chain B (100 ... 199) up in y from A's end; the one bond between them joins index 99 and
  index 199, the largest of either chain: the last hook goes between two roots far below both"""
  x = np.zeros((200, 3))
  x[:100, 0] = np.arange(100.0)
  k = np.arange(100)
  idx = np.where(k == 0, 199, 99 + k)
  x[idx, 0] = 99.0
  x[idx, 1] = 1.0 + k
  L = CHAIN_L[mode]
  for plane in PLANES:
    adj = cn.bonds(x, L, CHAIN_R_CUT, plane)
    assert adj.sum() == 2 * 199 and adj[99, 199] and not adj[:100, 100:199].any()
    ref = _ref(("joined", mode), x, L, CHAIN_R_CUT, plane)
    assert np.all(ref[0] == 0)
    _same(_run(ctx, x, L, CHAIN_R_CUT, plane), ref)


@pytest.mark.parametrize("n", [64, 257, 1024])
def test_complete_graphs(ctx, n):
  """every point within r_cut of every other: every union contends for the same roots"""
  x = np.random.RandomState(n).uniform(0, 0.5, (n, 3))      # diameter sqrt(0.75) < 1
  for mode in MODES:
    L = BOX * np.asarray(MODES[mode], dtype=np.float64)
    for plane in PLANES:
      assert cn.bond_margin(x, L, 1.0, plane) > 0.2
      labels, sizes = _run(ctx, x, L, 1.0, plane)
      assert np.all(labels == 0) and sizes[0, 0] == n and np.count_nonzero(sizes) == 1


@pytest.mark.parametrize("mode", list(MODES))
def test_no_bond_at_all(ctx, mode):
  """lattices 2 apart with r_cut 1: a 13 x 10 layer of staggered heights (no bond in the plane, so none in 3-D either) and, for
  the 3-D distance, a 6 x 5 x 5 grid: labels == arange, every size 1"""
  layer = np.stack(np.meshgrid(np.arange(13.0), np.arange(10.0), [0.0], indexing="ij"), axis=-1).reshape(-1, 3) * 2.0
  layer[:, 2] = 0.25 * (np.arange(130) % 4)
  grid = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0), np.arange(5.0), indexing="ij"), axis=-1).reshape(-1, 3)[:130] * 2.0
  flags = np.asarray(MODES[mode], dtype=np.float64)
  for x, L, planes in ((layer, np.array([26.0, 20.0, 10.0]) * flags, PLANES), (grid, np.array([12.0, 10.0, 10.0]) * flags, ("xyz",))):
    for plane in planes:
      assert cn.bond_margin(x, L, 1.0, plane) > 0.5
      labels, sizes = _run(ctx, x, L, 1.0, plane)
      assert np.array_equal(labels[0], np.arange(130)) and np.all(sizes == 1)
  # under xy the columns of the grid are stacks: 30 clusters of the points above one another
  _same(_run(ctx, grid, L, 1.0, "xy"), cn.labels_sizes(grid, L, 1.0, "xy"))


def test_exact_ties_on_dyadic_coordinates(ctx):
  """a pair at exactly d = r_cut = 1.25 (3-4-5 on quarters) is not bonded; with the next double above r_cut it is"""
  up = float(np.nextafter(1.25, np.inf))
  for L, shift in ((np.zeros(3), 0.0), (np.array([8.0, 8.0, 0.0]), 3 * 8.0), (np.array([8.0, 8.0, 8.0]), -2 * 8.0)):
    for b in ([0.75, 1.0, 0.0], [0.0, 0.75, 1.0]):
      pts = np.array([[0.25, 0.5, 0.125], [0.25 + b[0] + shift, 0.5 + b[1] - shift, 0.125 + b[2]]])
      plane_d = {"xy": np.hypot(b[0], b[1]), "xyz": 1.25}
      for plane in PLANES:
        tie = plane_d[plane] == 1.25
        assert (cn.bond_margin(pts, L, 1.25, plane) == 0.0) == tie      # exactly on the bond length, in long double too
        at, above = _run(ctx, pts, L, 1.25, plane), _run(ctx, pts, L, up, plane)
        _same(at, cn.labels_sizes(pts, L, 1.25, plane))
        _same(above, cn.labels_sizes(pts, L, up, plane))
        if tie:
          assert at[0].tolist() == [[0, 1]] and above[0].tolist() == [[0, 0]] and above[1].tolist() == [[2, 0]]
        else:      # (0, 0.75) in the plane: bonded either way
          assert at[0].tolist() == [[0, 0]] and above[0].tolist() == [[0, 0]]


@pytest.mark.parametrize("mode", list(MODES))
def test_stacked_and_coincident_points(ctx, mode):
  L = np.array([4.0, 4.0, 4.0]) * np.asarray(MODES[mode], dtype=np.float64)
  pts = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 5.0], [1.0, 1.0, 0.0], [3.0, 3.0, 0.0]])      # 0 and 2 coincide, 1 is stacked on them
  labels, sizes = _run(ctx, pts, L, 0.5, "xy")
  assert labels.tolist() == [[0, 0, 0, 3]] and sizes.tolist() == [[3, 0, 0, 1]]
  labels, sizes = _run(ctx, pts, L, 0.5, "xyz")      # 5 apart in z, 1 through the image where z is periodic: beyond r_cut either way
  assert labels.tolist() == [[0, 1, 0, 3]] and sizes.tolist() == [[2, 1, 0, 1]]
  for plane in PLANES:
    _same(_run(ctx, pts, L, 0.5, plane), cn.labels_sizes(pts, L, 0.5, plane))


@pytest.mark.parametrize("mode", list(MODES))
def test_select(ctx, mode):
  frames, L = _cloud(129, mode)
  rng = np.random.RandomState(8)
  sel = rng.uniform(size=(1, 129)) < 0.6
  for plane in PLANES:
    r_cut = cloud_r_cut(129, plane)
    ref = cn.labels_sizes(frames, L, r_cut, plane, sel)
    got = _run(ctx, frames, L, r_cut, plane, sel)
    _same(got, ref)
    assert np.all(got[0][~sel] == -1) and np.all(got[0][sel] >= 0) and got[1].sum() == sel.sum() and np.all(got[1][~sel] == 0)
    _same(_run(ctx, frames, L, r_cut, plane, sel.astype(np.uint8) * 3), ref)      # any non-zero byte selects
    none = _run(ctx, frames, L, r_cut, plane, np.zeros((1, 129), bool))
    assert np.all(none[0] == -1) and not none[1].any()
    _same(_run(ctx, frames, L, r_cut, plane, np.ones((1, 129), bool)), _ref(("cloud", 129, mode), frames, L, r_cut, plane))
    # a selected point surrounded only by unselected ones: a singleton, although everything is within this r_cut
    one = np.zeros((1, 129), bool)
    one[0, 77] = True
    labels, sizes = _run(ctx, frames, L, 1e3, plane, one)
    assert labels[0, 77] == 77 and sizes[0, 77] == 1 and sizes.sum() == 1 and np.count_nonzero(labels >= 0) == 1


@pytest.mark.parametrize("mode", list(MODES))
def test_seven_frames_in_one_call(ctx, mode):
  """frames that differ, a frame that is one cluster next to a frame with no bond: no label leaks across a frame edge"""
  L, r_cut = BOX * np.asarray(MODES[mode], dtype=np.float64), 0.6
  for seed in range(700, 720):
    rng = np.random.RandomState(seed)
    frames = rng.uniform(0, 1, (7, 65, 3)) * BOX + rng.randint(-2, 3, (7, 65, 3)) * L
    frames[3] = rng.uniform(0, 0.25, (65, 3))      # one cluster: diameter 0.44
    # no bond: a 13 x 5 lattice, 0.625 and 1.25 apart (1.5 and 2 from its images in the box)
    frames[4] = np.stack(np.meshgrid(np.arange(13.0), np.arange(5.0), [0.0], indexing="ij"), axis=-1).reshape(-1, 3) * np.array([0.625, 1.25, 1.0])
    if _margin_ok(frames, L, {p: r_cut for p in PLANES}):
      break
  for plane in PLANES:
    assert cn.bond_margin(frames, L, r_cut, plane) > cn.MARGIN
    ref = cn.labels_sizes(frames, L, r_cut, plane)
    assert np.all(ref[0][3] == 0) and np.array_equal(ref[0][4], np.arange(65)) and len({ref[0][f].tobytes() for f in range(7)}) == 7
    got = _run(ctx, frames, L, r_cut, plane)
    _same(got, ref)
    for f in range(7):
      one = _run(ctx, frames[f], L, r_cut, plane)
      assert np.array_equal(one[0][0], got[0][f]) and np.array_equal(one[1][0], got[1][f])


@pytest.mark.parametrize("mode", list(MODES))
def test_launch_plans(ctx, mode):
  """one-step chunks, chunks that straddle the unit edges, one range per wave; one resident round and eight: the same bits"""
  cases = [(_cloud(n, mode) + (n,)) for n in (65, 129, 200)]
  cases.append((_indexed(_chain_positions(), _chain_orders()["random"]), CHAIN_L[mode], None))
  for frames, L, n in cases:
    for plane in PLANES:
      r_cut = CHAIN_R_CUT if n is None else cloud_r_cut(n, plane)
      base = _run(ctx, frames, L, r_cut, plane)
      for chunk_steps in CHUNK_STEPS:
        for oversub in OVERSUB:
          with _plan(ctx, chunk_steps, oversub):
            _same(_run(ctx, frames, L, r_cut, plane), base)
  assert {k: ctx.get_option(k) for k in DEFAULTS} == DEFAULTS


# ---- resident entry ------------------------------------------------------------------------------------------------
RES_N, RES_BOX, RES_R_CUT = 4096, np.array([96.0, 96.0, 4.0]), 1.125      # 1.8 bonds per point in the plane, 0.7 in 3-D; 85 r_cut across


def _resident(ctx, x, L, r_cut, plane, select=None, **options):
  for k, v in options.items():
    ctx.set_option(k, v)
  try:
    ctx.set_positions(x, 0.1, periodic_length=L, wall=False)
    sel = None if select is None else torch.from_numpy(np.ascontiguousarray(select)).cuda()
    labels, sizes = ctx.cluster_labels_device(r_cut, plane=plane, select=sel)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (x.shape[0],) and tuple(sizes.shape) == (x.shape[0],)
    return labels.cpu().numpy()[None], sizes.cpu().numpy()[None]
  finally:
    for k in options:
      ctx.set_option(k, 1)


@pytest.mark.parametrize("mode", list(MODES))
def test_resident_entry(ctx, mode):
  L = RES_BOX * np.asarray(MODES[mode], dtype=np.float64)
  for seed in range(40, 60):
    x = np.random.RandomState(seed).uniform(0, 1, (RES_N, 3)) * RES_BOX
    if all(cn.bond_margin(x, L, RES_R_CUT, p) > cn.MARGIN for p in PLANES):
      break
  assert all(cn.bond_margin(x, L, RES_R_CUT, p) > cn.MARGIN for p in PLANES)
  assert np.all(np.ptp(x[:, :2], axis=0) > 50 * RES_R_CUT)      # most tile pairs are far beyond the bond length
  order = np.lexsort((x[:, 1] // 6.0, x[:, 0] // 6.0))          # pre-sorted: cell by cell
  sel = np.random.RandomState(1).uniform(size=RES_N) < 0.8
  for plane in PLANES:
    ref = cn.labels_sizes(x, L, RES_R_CUT, plane)
    assert np.count_nonzero(ref[1]) > 500 and ref[1].max() >= 5
    _same(_run(ctx, x, L, RES_R_CUT, plane), ref)
    for cull in (1, 0):
      _same(_resident(ctx, x, L, RES_R_CUT, plane, force_cull=cull), ref)
      lab_s, siz_s = _resident(ctx, x[order], L, RES_R_CUT, plane, force_cull=cull)
      _same((lab_s, siz_s), _run(ctx, x[order], L, RES_R_CUT, plane))      # the batch entry on the same points
      # against the restatement: the same partition, every cluster of the sorted run named by its smallest index in the first order
      canon = np.full(RES_N, RES_N, dtype=np.int64)
      np.minimum.at(canon, lab_s[0], order)
      assert np.array_equal(canon[lab_s[0]][np.argsort(order)], ref[0][0])
    _same(_resident(ctx, x, L, RES_R_CUT, plane, force_sort=0), ref)      # the caller's order, no Morton copy
    if plane == "xy":
      _same(_resident(ctx, x, L, RES_R_CUT, plane, select=sel), cn.labels_sizes(x, L, RES_R_CUT, plane, sel[None]))
  assert ctx.get_option("force_cull") == 1 and ctx.get_option("force_sort") == 1


def test_resident_bilayer_bonds_across_layers_in_the_plane(ctx):
  """two layers 3 r_cut apart in z: under xy every point is bonded to its partner in the other layer (a 3-D tile gap would cull it)"""
  rng = np.random.RandomState(9)
  L = np.array([96.0, 96.0, 0.0])
  for seed in range(9, 29):
    low = np.random.RandomState(seed).uniform(0, 1, (2048, 3)) * np.array([96.0, 96.0, 0.0])
    x = np.concatenate([low, low + np.array([0.125, 0.0, 3 * RES_R_CUT])])[rng.permutation(4096)]
    if all(cn.bond_margin(x, L, RES_R_CUT, p) > cn.MARGIN for p in PLANES):
      break
  assert all(cn.bond_margin(x, L, RES_R_CUT, p) > cn.MARGIN for p in PLANES)
  ref = cn.labels_sizes(x, L, RES_R_CUT, "xy")
  for cull in (1, 0):
    got = _resident(ctx, x, L, RES_R_CUT, "xy", force_cull=cull)
    _same(got, ref)
  upper = x[:, 2] > 0
  assert np.all(got[1] % 2 == 0)      # every cluster holds whole pairs
  for l in np.unique(got[0])[:50]:
    members = got[0][0] == l
    assert upper[members].sum() == (~upper[members]).sum()
  ref3 = cn.labels_sizes(x, L, RES_R_CUT, "xyz")
  _same(_resident(ctx, x, L, RES_R_CUT, "xyz"), ref3)
  for l in np.unique(ref3[0])[:50]:
    assert len(set(upper[ref3[0][0] == l])) == 1      # in 3-D the layers do not meet


def test_resident_refusals(ctx):
  x = np.random.RandomState(2).uniform(0, 4, (100, 3)) + np.array([0, 0, 0.5])
  labels = torch.full((100,), 7, dtype=torch.int32, device="cuda")
  sizes = torch.full((100,), 7, dtype=torch.int32, device="cuda")
  ctx.set_positions(x, 0.1, wall=True)
  with pytest.raises(RmbError, match="cluster labels use raw positions"):
    ctx.cluster_labels_device(1.0, labels=labels, sizes=sizes)
  ctx.set_positions(x, 0.1, wall=False)
  for r_cut in (0.0, -1.0, float("inf"), float("nan")):
    with pytest.raises(RmbError, match="r_cut must be positive and finite"):
      ctx.cluster_labels_device(r_cut, labels=labels, sizes=sizes)
  with pytest.raises(ValueError, match="plane must be"):
    ctx.cluster_labels_device(1.0, plane="xz", labels=labels, sizes=sizes)
  with pytest.raises(ValueError, match="select must be"):
    ctx.cluster_labels_device(1.0, select=torch.ones(99, dtype=torch.bool, device="cuda"), labels=labels, sizes=sizes)
  with pytest.raises(ValueError, match="labels must be"):
    ctx.cluster_labels_device(1.0, labels=labels.long(), sizes=sizes)
  rc = ctx._lib.rmb_cluster_labels_device(ctx._h, None, 1.0, 2, labels.data_ptr(), sizes.data_ptr())
  assert rc == -1 and b"plane must be 0 (xyz) or 1 (xy)" in ctx._lib.rmb_last_error()
  assert ctx._lib.rmb_cluster_labels_device(ctx._h, None, 1.0, 0, None, sizes.data_ptr()) == -1
  torch.cuda.synchronize()
  assert bool((labels == 7).all()) and bool((sizes == 7).all())
  got = ctx.cluster_labels_device(1.0, labels=labels, sizes=sizes)
  assert got[0] is labels and got[1] is sizes
  ref = cn.labels_sizes(x, np.zeros(3), 1.0, "xyz")
  assert np.array_equal(labels.cpu().numpy(), ref[0][0]) and np.array_equal(sizes.cpu().numpy(), ref[1][0])


def test_refused_calls_leave_the_outputs_untouched(ctx):
  frames, L = _cloud(65, "xy", 7)
  dev = _dev(frames)
  labels = torch.full((7, 65), 7, dtype=torch.int32, device="cuda")
  sizes = torch.full((7, 65), 7, dtype=torch.int32, device="cuda")
  for bad in (dev.float(), dev.cpu(), dev[:, :, :2], dev.transpose(0, 1)):
    with pytest.raises(ValueError, match="frames must be"):
      ctx.cluster_labels_frames_device(bad, L, 1.0)
  with pytest.raises(ValueError, match="plane must be"):
    ctx.cluster_labels_frames_device(dev, L, 1.0, plane="xz")
  for sel in (torch.ones((7, 64), dtype=torch.bool, device="cuda"), torch.ones((7, 65), dtype=torch.int32, device="cuda"), np.ones((7, 65), bool)):
    with pytest.raises(ValueError, match="select must be"):
      ctx.cluster_labels_frames_device(dev, L, 1.0, select=sel)
  for out in (dict(labels=labels.long()), dict(sizes=sizes[:, :64]), dict(labels=labels.cpu())):
    with pytest.raises(ValueError, match="must be a contiguous CUDA int32"):
      ctx.cluster_labels_frames_device(dev, L, 1.0, **out)
  for r_cut in (0.0, -1.0, float("inf"), float("nan")):
    with pytest.raises(RmbError, match="r_cut must be positive and finite"):
      ctx.cluster_labels_frames_device(dev, L, r_cut, labels=labels, sizes=sizes)
  lib, Lc = ctx._lib, np.ascontiguousarray(L, dtype=np.float64)
  call = lambda **kw: lib.rmb_cluster_labels_frames_device(      # noqa: E731
      ctx._h, kw.get("frames", dev.data_ptr()), None, kw.get("n_frames", 7), kw.get("n", 65), kw.get("L", Lc.ctypes.data), 1.0, kw.get("plane", 0),
      kw.get("labels", labels.data_ptr()), kw.get("sizes", sizes.data_ptr()))
  for kw, message in ((dict(frames=None), b"null frames"), (dict(labels=None), b"null labels or sizes"), (dict(sizes=None), b"null labels or sizes"),
                      (dict(L=None), b"null periodic_length"), (dict(n_frames=-1), b"negative size"), (dict(n=-1), b"negative size"),
                      (dict(plane=3), b"plane must be 0 (xyz) or 1 (xy)"), (dict(n_frames=2 ** 26, n=65), b"too many points")):
    assert call(**kw) == -1 and message in lib.rmb_last_error(), kw
  assert call(n_frames=0) == 0 and call(n=0) == 0      # nothing to do touches nothing
  torch.cuda.synchronize()
  assert bool((labels == 7).all()) and bool((sizes == 7).all())
  empty = ctx.cluster_labels_frames_device(dev[:0], L, 1.0)
  assert tuple(empty[0].shape) == (0, 65) and tuple(ctx.cluster_labels_frames_device(dev[:, :0].contiguous(), L, 1.0)[1].shape) == (7, 0)
  # out= is overwritten and handed back; one frame as (n, 3)
  got = ctx.cluster_labels_frames_device(dev, L, 0.6, plane="xy", labels=labels, sizes=sizes)
  assert got[0] is labels and got[1] is sizes
  assert cn.bond_margin(frames, L, 0.6, "xy") > cn.MARGIN
  _same((labels.cpu().numpy(), sizes.cpu().numpy()), cn.labels_sizes(frames, L, 0.6, "xy"))
  one = ctx.cluster_labels_frames_device(dev[2], L, 0.6, plane="xy")
  assert tuple(one[0].shape) == (65,) and torch.equal(one[0], labels[2]) and torch.equal(one[1], sizes[2])


def test_resident_configuration_is_left_alone_by_the_frames_entry():
  """a wall M_tt f of the resident blobs before and after"""
  from rigidmultiblobswall_amd import MobilityContext
  rng = np.random.RandomState(4)
  r = rng.uniform(0, 6, (500, 3)) + np.array([0, 0, 0.5])
  f = rng.randn(1500)
  frames, L = _cloud(129, "xy")
  c = MobilityContext(0)
  try:
    c.set_option("deterministic", 1)      # the atomic-free sweep: the same call gives the same bits
    c.set_positions(r, 0.2, wall=True)
    before, again = c.matvec("tt", f, 1.0), c.matvec("tt", f, 1.0)
    assert np.array_equal(before, again)
    c.cluster_labels_frames_device(_dev(frames), L, 0.7)
    torch.cuda.synchronize()
    assert np.array_equal(before, c.matvec("tt", f, 1.0)) and c.n == 500
  finally:
    c.close()


def test_multi_device_context_refuses():
  from rigidmultiblobswall_amd import clusters
  from rigidmultiblobswall_amd.multi import MultiContext
  m = MultiContext([0])
  try:
    assert not hasattr(m, "cluster_labels_frames_device") and not hasattr(m, "cluster_labels_device")
    with pytest.raises(ValueError, match="single-GPU MobilityContext"):
      clusters.Clusters(2, BOX, 1.0, ctx=m)
  finally:
    m.close()
