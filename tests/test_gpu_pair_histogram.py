"""The HIP pair-distance histogram (rmb_pair_histogram*, pair_hist_kernels.h) against the numpy restatement
(_pair_hist_numpy.py), the reference program's goldens through RadialDistribution and the command line, and the sampler's
g(r) hook.

Every comparison of counts is EXACT equality.  That is a fair demand because every input satisfies, and every test asserts, the
edge-margin precondition: in long double no pair has r / dr within 1e-9 of an integer (r_max is the integer n_bins), while
fp64 evaluation errors of r are ~1e-15 relative -- so every correct implementation bins every pair alike.  Inputs that fail
get another seed.  Coincident points built on purpose sit at r = 0 exactly and are exempt."""
import io
import os

import numpy as np
import pytest
import torch

import _pair_hist_numpy as phnp
from _mcmc_moves_common import layout, vertex_sets, write_deck
from conftest import golden_files, load_golden
from rigidmultiblobswall_amd import correlation
from rigidmultiblobswall_amd._lib import RmbError

pytestmark = pytest.mark.gpu

BOX = np.array([9.0, 7.0, 5.0])
MODES = {"open": (0, 0, 0), "x": (1, 0, 0), "xy": (1, 1, 0), "xyz": (1, 1, 1)}
SIZES = (1, 2, 63, 64, 65, 129, 2048, 2049)      # tile edges, the diagonal step-32 peel, the first sorted sizes (32 tiles)
N_BINS = 2000


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _cloud(n, box=BOX, spread=True):
  """n points over the box -- and, in the first two directions, over the neighbouring cells as well, so that periodic runs
  meet separations of more than one period"""
  def make(rng):
    x = rng.uniform(0, 1, (n, 3)) * box
    if spread:
      x[:, :2] += box[:2] * rng.randint(-2, 3, (n, 2))
    return x[None]
  return make


_CASES = {}


def _case(n, mode):
  """(points (n, 3), L, r_max, reference counts), computed once and shared; the margin precondition asserted"""
  if (n, mode) not in _CASES:
    L = BOX * np.array(MODES[mode], dtype=np.float64)
    r_max = 2.2 if n >= 2048 else 4.3      # the sorted sizes: a reach the tile culling can use (open runs span 5 cells)
    frames = phnp.points_with_margin(_cloud(n), L, r_max, N_BINS, 1000 * n + len(mode))
    assert n < 2 or phnp.edge_margin(frames, L, r_max, N_BINS) > phnp.MARGIN
    _CASES[(n, mode)] = (frames[0], L, r_max, phnp.counts(frames, L, r_max, N_BINS))
  return _CASES[(n, mode)]


def _resident(ctx, x, L, r_max, n_bins):
  ctx.set_positions(x, 1.0, L, wall=False)
  return ctx.pair_histogram(r_max, n_bins)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", SIZES)
def test_resident_counts_equal_the_restatement(ctx, n, mode):
  x, L, r_max, ref = _case(n, mode)
  got = _resident(ctx, x, L, r_max, N_BINS)
  assert got.dtype == np.uint64 and got.shape == (N_BINS,)
  assert np.array_equal(got, ref)
  if n >= 65:
    assert ref.sum() > 0
  if n < 2:
    assert got.sum() == 0


def test_culling_is_exact(ctx):
  """4096 points, r_max = 1/16 of the box: with tile culling, without it, and the restatement"""
  n, box = 4096, np.array([32.0, 32.0, 3.0])
  L, r_max = box * np.array([1.0, 1.0, 0.0]), 2.0
  frames = phnp.points_with_margin(_cloud(n, box), L, r_max, N_BINS, 4096)
  assert phnp.edge_margin(frames, L, r_max, N_BINS) > phnp.MARGIN
  ref = phnp.counts(frames, L, r_max, N_BINS)
  culled = _resident(ctx, frames[0], L, r_max, N_BINS)
  ctx.set_option("force_cull", 0)
  try:
    plain = _resident(ctx, frames[0], L, r_max, N_BINS)
  finally:
    ctx.set_option("force_cull", 1)
  assert np.array_equal(culled, plain) and np.array_equal(culled, ref) and ref.sum() > 10000


def test_every_pair_is_met_once(ctx):
  """2049 points, open, r_max beyond the largest possible separation: the counts sum to N (N - 1) / 2"""
  x, L, _, _ = _case(2049, "open")
  reach = 2.0 * float(np.linalg.norm(x.max(axis=0) - x.min(axis=0)))
  assert _resident(ctx, x, L, reach, 64).sum() == 2049 * 2048 // 2
  ctx.set_option("force_sort", 0)
  try:
    assert _resident(ctx, x, L, reach, 64).sum() == 2049 * 2048 // 2
  finally:
    ctx.set_option("force_sort", 1)


def test_device_calls_accumulate(ctx):
  x, L, r_max, ref = _case(129, "xy")
  ctx.set_positions(x, 1.0, L, wall=False)
  out = ctx.pair_histogram_device(r_max, N_BINS)
  assert out.dtype == torch.int64 and out.is_cuda and np.array_equal(out.cpu().numpy().astype(np.uint64), ref)
  again = ctx.pair_histogram_device(r_max, N_BINS, out=out)
  assert again is out and np.array_equal(out.cpu().numpy().astype(np.uint64), 2 * ref)
  for bad in (torch.zeros(N_BINS, dtype=torch.float64, device="cuda"), torch.zeros(N_BINS + 1, dtype=torch.int64, device="cuda"),
              torch.zeros(N_BINS, dtype=torch.int64)):
    with pytest.raises(ValueError, match="out must be"):
      ctx.pair_histogram_device(r_max, N_BINS, out=bad)


def test_coincident_points_land_in_bin_zero(ctx):
  L, r_max, n_bins = BOX * np.array([1.0, 1.0, 0.0]), 3.0, 500

  def make(rng):
    x = _cloud(150)(rng)[0]
    x[40:110] = x[40]      # 70 coincident points, across a tile edge
    return x[None]
  frames = phnp.points_with_margin(make, L, r_max, n_bins, 77, allow_zero=True)
  assert phnp.edge_margin(frames, L, r_max, n_bins, allow_zero=True) > phnp.MARGIN
  ref = phnp.counts(frames, L, r_max, n_bins)
  assert ref[0] >= 70 * 69 // 2
  assert np.array_equal(_resident(ctx, frames[0], L, r_max, n_bins), ref)
  out = ctx.pair_histogram_frames_device(torch.from_numpy(frames).cuda(), L, r_max, n_bins)
  assert np.array_equal(out.cpu().numpy().astype(np.uint64), ref)


@pytest.mark.parametrize("n_bins", [1, 2000, 8192])
def test_bin_counts(ctx, n_bins):
  L, r_max = BOX * np.array([1.0, 1.0, 1.0]), 3.3
  frames = phnp.points_with_margin(_cloud(129), L, r_max, n_bins, 300 + n_bins)
  assert phnp.edge_margin(frames, L, r_max, n_bins) > phnp.MARGIN
  ref = phnp.counts(frames, L, r_max, n_bins)
  assert np.array_equal(_resident(ctx, frames[0], L, r_max, n_bins), ref)
  out = ctx.pair_histogram_frames_device(torch.from_numpy(frames).cuda(), L, r_max, n_bins)
  assert np.array_equal(out.cpu().numpy().astype(np.uint64), ref)


def test_refused_calls(ctx):
  x, L, r_max, _ = _case(65, "xy")
  ctx.set_positions(x, 1.0, L, wall=False)
  frames = torch.from_numpy(x[None].copy()).cuda()
  for kw in (dict(r_max=r_max, n_bins=8193), dict(r_max=0.0, n_bins=100), dict(r_max=-1.0, n_bins=100), dict(r_max=r_max, n_bins=0)):
    with pytest.raises(RmbError):
      ctx.pair_histogram(**kw)
    with pytest.raises(RmbError):
      ctx.pair_histogram_device(**kw)
    with pytest.raises(RmbError):
      ctx.pair_histogram_frames_device(frames, L, **kw)
  with pytest.raises(ValueError, match="frames must be"):
    ctx.pair_histogram_frames_device(frames.float(), L, r_max, 100)
  ctx.set_target_range(0, 32)
  try:
    with pytest.raises(RmbError, match="target range"):
      ctx.pair_histogram(r_max, 100)
  finally:
    ctx.set_target_range(0, 65)
  ctx.set_positions(np.abs(x) + 1.0, 1.0, L, wall=True)
  with pytest.raises(RmbError, match="wall = 0"):
    ctx.pair_histogram(r_max, 100)
  # nothing to count leaves the histogram as it is
  out = torch.full((100,), 7, dtype=torch.int64, device="cuda")
  ctx.pair_histogram_frames_device(frames[:0], L, r_max, 100, out=out)
  ctx.pair_histogram_frames_device(frames[:, :1].contiguous(), L, r_max, 100, out=out)
  ctx.set_positions(x[:1], 1.0, L, wall=False)
  ctx.pair_histogram_device(r_max, 100, out=out)
  assert torch.equal(out, torch.full((100,), 7, dtype=torch.int64, device="cuda"))


# ---- the batch entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames, n", [(1, 65), (3, 65), (5, 1875)])      # 1875: the reference example's N
def test_batch_equals_resident_and_restatement(ctx, n_frames, n):
  box = np.array([40.0, 16.0, 1.2]) if n == 1875 else BOX
  L, r_max = box * np.array([1.0, 1.0, 0.0]), 0.25 * box[0]

  def make(rng):
    return np.concatenate([_cloud(n, box)(rng) for _ in range(n_frames)])
  frames = phnp.points_with_margin(make, L, r_max, N_BINS, 50 * n + n_frames)
  assert phnp.edge_margin(frames, L, r_max, N_BINS) > phnp.MARGIN
  ref = phnp.counts(frames, L, r_max, N_BINS)
  out = ctx.pair_histogram_frames_device(torch.from_numpy(frames).cuda(), L, r_max, N_BINS)
  assert np.array_equal(out.cpu().numpy().astype(np.uint64), ref)
  resident = sum(_resident(ctx, f, L, r_max, N_BINS).astype(np.int64) for f in frames)
  assert np.array_equal(resident.astype(np.uint64), ref)
  # one frame as (n, 3)
  one = ctx.pair_histogram_frames_device(torch.from_numpy(frames[0].copy()).cuda(), L, r_max, N_BINS)
  assert np.array_equal(one.cpu().numpy().astype(np.uint64), phnp.counts(frames[:1], L, r_max, N_BINS))


def test_batch_leaves_the_resident_state_alone():
  """The energy of a sorted configuration depends on the age of its Morton permutation: two evaluations with batch calls in
  between give the bits of two evaluations without."""
  from rigidmultiblobswall_amd import MobilityContext
  rng = np.random.RandomState(9)
  x = rng.uniform(0, 1, (4096, 3)) * np.array([30.0, 30.0, 2.0]) + np.array([0, 0, 0.3])
  L = np.array([30.0, 30.0, 0.0])
  frames = torch.from_numpy(rng.uniform(0, 5, (3, 65, 3))).cuda()
  kw = dict(repulsion_strength=0.3, debye_length=0.1, blob_radius=0.2, repulsion_strength_wall=0.5, debye_length_wall=0.1, weight=0.4)
  results = []
  for with_batch in (True, False):
    c = MobilityContext(0)
    try:
      c.set_positions(x, 0.2, L, wall=False)
      a = c.blob_potential(**kw)
      if with_batch:
        c.pair_histogram_frames_device(frames, L, 2.0, 100)
        c.pair_histogram_frames_device(frames, np.zeros(3), 2.0, 100)
      b = c.blob_potential(**kw)
      assert c.n == 4096
      results.append((a, b))
    finally:
      c.close()
  assert results[0] == results[1]


# ---- goldens of the reference program ------------------------------------------------------------------------------------------
GOLDENS = golden_files("g17_gr_*.npz")


def _golden(path):
  d = load_golden(path)
  return d["frames"], int(d["n_points"]), d["periodic_length"], int(d["n_bins"]), phnp.parse_gr(str(d["output"]))


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[7:-4] for p in GOLDENS])
def test_goldens_through_radial_distribution(ctx, path):
  frames, n, L, n_bins, (r, g, hist) = _golden(path)
  assert phnp.edge_margin(frames, L, 0.5 * L[0], n_bins) > phnp.MARGIN
  rd = correlation.RadialDistribution(n, L, ctx=ctx)      # r_max = lx / 2, 2000 bins, pseudo2d: the program's
  assert rd.batch and rd.n_bins == n_bins
  rd.add(frames[0])
  rd.add_frames(frames[1:3])
  rd.add(torch.from_numpy(frames[3].copy()).cuda())
  assert rd.n_frames == 4
  assert np.array_equal(2 * rd.counts.astype(np.int64), hist)
  assert np.all(np.abs(rd.g() - g) <= 1e-5 * np.abs(g)) and np.all(np.abs(rd.r - r) <= 1e-5 * r)
  rd.close()
  assert ctx.n >= 0 and ctx._h.value      # a caller's context stays open


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[7:-4] for p in GOLDENS])
def test_goldens_through_the_command_line(path, tmp_path):
  frames, n, L, n_bins, (r, g, hist) = _golden(path)
  traj = tmp_path / "run.config"
  traj.write_text(phnp.config_text(frames, final_newline="shifted" in path))
  argv = [str(traj), str(n), repr(float(L[0])), repr(float(L[1])), repr(float(L[2]))]
  buf = io.StringIO()      # the module's main(), which `python -m rigidmultiblobswall_amd.correlation` runs; a process of its own costs 12 s
  assert correlation.main(argv, out=buf) == 0
  text = buf.getvalue()
  r2, g2, h2 = phnp.parse_gr(text)
  assert np.array_equal(h2, hist)
  assert np.all(np.abs(g2 - g) <= 1e-5 * np.abs(g)) and np.all(np.abs(r2 - r) <= 1e-5 * r)
  # --skip 1: the first frame is neither counted nor normalised by
  buf = io.StringIO()
  assert correlation.main(argv + ["--skip", "1", "--bins", "400", "--rmax", "7.5"], out=buf) == 0
  r3, g3, h3 = phnp.parse_gr(buf.getvalue())
  c3 = phnp.counts(frames[1:], L, 7.5, 400)
  if phnp.edge_margin(frames[1:], L, 7.5, 400) > phnp.MARGIN:
    assert np.array_equal(h3, 2 * c3.astype(np.int64))
    g_ref = phnp.g_pseudo2d(c3, 3, n, L[0], L[1], 7.5)
    assert np.all(np.abs(g3 - g_ref) <= 1e-5 * np.abs(g_ref))
  else:
    pytest.fail("the golden's frames 1..3 sit on a bin edge at 400 bins of 7.5: pick other --skip arguments")


def test_radial_distribution_resident_path_and_3d(ctx):
  """2048 points per frame go through the resident, sorted and culled sweep; the 3d normalisation on the same counts"""
  x, L, r_max, ref = _case(2048, "xyz")
  rd = correlation.RadialDistribution(2048, L, r_max=r_max, n_bins=N_BINS, normalisation="3d", ctx=ctx)
  assert not rd.batch
  rd.add_frames(np.stack([x, x]))
  assert rd.n_frames == 2 and np.array_equal(rd.counts, 2 * ref)
  e = (r_max / N_BINS) * np.arange(N_BINS + 1)
  ideal = 0.5 * 2048 * (2048 / np.prod(L)) * 4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3)
  assert np.allclose(rd.g(), ref / ideal, rtol=1e-12, atol=0)
  rd.close()


# ---- the sampler's hook ----------------------------------------------------------------------------------------------------------
SAMPLER_LINES = ("n_steps 20\nn_save 5\ninitial_step 0\ng 0.6\nblob_radius 0.2\nkT 0.05\nperiodic_length 6.0 6.0 0\nrepulsion_strength_wall 0.8\n"
                 "debye_length_wall 0.12\nrepulsion_strength 0.35\ndebye_length 0.09\nseed 31\noutput_name run\nsave_clones one_file\n")
GR = (3.0, 60)


def _run_sampler(directory, moves, gr, **kw):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  from rigidmultiblobswall_amd.read_input import ReadInput
  boom, shell = vertex_sets()
  deck = layout([shell] * 16, 1.4, 1.1, 4, side=6.0)
  os.makedirs(directory)
  path = write_deck(directory, deck, [("structure", "shell", list(range(16)))], SAMPLER_LINES)
  cwd = os.getcwd()
  os.chdir(directory)
  try:
    s = MCMCSampler(ReadInput(path), device=0, moves=moves, gr=gr, check_user_potential=False, **kw)
    try:
      s.run()
    finally:
      s.close()
  finally:
    os.chdir(cwd)
  return s


def _outputs(directory):
  """every file of a run but the wall-clock time and the g(r) table, as bytes"""
  return {f: open(os.path.join(directory, f), "rb").read() for f in sorted(os.listdir(directory)) if not f.endswith((".time", ".gr.dat"))}


@pytest.mark.parametrize("moves", ["all", "single"])
def test_sampler_hook(moves, tmp_path):
  on = _run_sampler(str(tmp_path / "on"), moves, GR)
  off = _run_sampler(str(tmp_path / "off"), moves, None)
  # the chain and every other output are those of the run without the hook
  assert on.accepted == off.accepted and on.energy_log == off.energy_log and on.accepted_moves == off.accepted_moves
  assert _outputs(str(tmp_path / "on")) == _outputs(str(tmp_path / "off"))
  assert not os.path.exists(str(tmp_path / "off" / "run.gr.dat")) and off.gr_counts is None
  # the table against the restatement on the saved frames
  frames = correlation.read_frames(str(tmp_path / "on" / "run.shell.config"), 16)
  L = np.array([6.0, 6.0, 0.0])
  assert frames.shape == (5, 16, 3) and on.gr_frames == 5      # steps 0, 5, 10, 15 and the final save
  assert phnp.edge_margin(frames, L, GR[0], GR[1]) > phnp.MARGIN
  ref = phnp.counts(frames, L, GR[0], GR[1])
  r, g, hist = phnp.parse_gr(open(str(tmp_path / "on" / "run.gr.dat")).read())
  assert np.array_equal(hist, 2 * ref.astype(np.int64)) and ref.sum() > 0 and np.array_equal(on.gr_counts, ref)
  g_ref = phnp.g_pseudo2d(ref, 5, 16, 6.0, 6.0, GR[0])
  assert np.all(np.abs(g - g_ref) <= 1e-5 * np.abs(g_ref))


def test_sampler_hook_host_state(tmp_path):
  """with an energy= function the locations are uploaded for the histogram"""
  on = _run_sampler(str(tmp_path / "on"), "all", GR, energy=lambda r: float(np.sum(r[:, 2])), write_files=False, keep_saved=True)
  frames = np.stack([on.saved[k][0] for k in sorted(on.saved)])
  L = np.array([6.0, 6.0, 0.0])
  assert frames.shape == (5, 16, 3) and phnp.edge_margin(frames, L, GR[0], GR[1]) > phnp.MARGIN
  assert np.array_equal(on.gr_counts, phnp.counts(frames, L, GR[0], GR[1]))
  with pytest.raises(ValueError, match="gr"):
    _run_sampler(str(tmp_path / "bad"), "all", (0.0, 10))
