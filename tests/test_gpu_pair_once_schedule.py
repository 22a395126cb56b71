"""The pair-once frame (pair_once_kernels.h) through both of its kernels -- pair histogram and potential energy, blob and
body forms -- under launch plans the defaults never produce at these sizes: "sym_chunk_steps" 4 cuts a wave's steps into
ONE-step chunks, so every k0 = 0 .. 63 begins a chunk on diagonal and off-diagonal units alike (a unit is then met from 64
chunks, the peeled step 32 of a diagonal unit by a chunk of its own), 28 gives chunks of 7 steps that straddle the unit
edges, 0 and 1024 one contiguous range per wave.  A pair met twice or never at a chunk edge, at the peel or in a partial
last tile changes a count.

Nothing here has a bound of its own: the counts are compared EXACTLY under the asserted edge-margin precondition of
test_gpu_pair_histogram.py, the energies with the checks and references of test_gpu_potential.py and
test_gpu_body_potential.py (imported, not restated).  References are computed once per point set and shared."""
import numpy as np
import pytest
import torch

import _body_forces_numpy as bfn
import _pair_hist_numpy as phnp
import test_gpu_body_potential as tbody
import test_gpu_potential as tpot

pytestmark = pytest.mark.gpu

SIZES = (65, 129, 200)      # two tiles, three tiles, four with a partial last one
MODES = {"open": 0, "xy": 2}
CHUNK_STEPS = (0, 4, 28, 1024)
OVERSUB = (1, 8)
DEFAULTS = {"sym_chunk_steps": 1024, "sym_oversub": 8}
BOX = np.array([9.0, 7.0, 5.0])
N_BINS = 2000
_REFS = {}


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  assert {k: c.get_option(k) for k in DEFAULTS} == DEFAULTS
  yield c
  c.close()


class _plan:
  """the two plan options for the length of a with block"""

  def __init__(self, ctx, chunk_steps, oversub):
    self.ctx, self.values = ctx, {"sym_chunk_steps": chunk_steps, "sym_oversub": oversub}

  def __enter__(self):
    for k, v in self.values.items():
      self.ctx.set_option(k, v)

  def __exit__(self, *exc):
    for k, v in DEFAULTS.items():
      self.ctx.set_option(k, v)


def _shared(key, make):
  if key not in _REFS:
    _REFS[key] = make()
  return _REFS[key]


def hist_case(n, mode, n_frames=1):
  """(frames (n_frames, n, 3), L, r_max beyond every separation, reference counts of every frame); the margin asserted"""
  def make():
    L = BOX * np.array([1.0, 1.0, 0.0]) * (MODES[mode] > 0)

    def cloud(rng):      # over the box and, in x and y, the neighbouring cells: separations of more than one period
      x = rng.uniform(0, 1, (n_frames, n, 3)) * BOX
      x[:, :, :2] += BOX[:2] * rng.randint(-2, 3, (n_frames, n, 2))
      return x
    # the points span five cells in x and y, one in z; an imaged component is at most half a period
    r_max = 1.01 * float(np.linalg.norm(np.where(L > 0, 0.5 * L, BOX * np.array([5.0, 5.0, 1.0]))))
    frames = phnp.points_with_margin(cloud, L, r_max, N_BINS, 7000 + 10 * n + n_frames + MODES[mode])
    assert phnp.edge_margin(frames, L, r_max, N_BINS) > phnp.MARGIN
    return frames, L, r_max, [phnp.counts(f[None], L, r_max, N_BINS) for f in frames]
  return _shared(("hist", n, mode, n_frames), make)


def energy_case(n, mode, form, below=()):
  def make():
    r, L = tpot._cloud(n, 100 + n, MODES[mode])
    if below:
      r[list(below), 2] = [-0.3, 0.0, -1e-9, -2.0, -0.05][:len(below)]
    kw = tpot._params(form, True, n)
    return r, L, kw, tpot._reference(r, L, kw)
  return _shared(("energy", n, mode, form, tuple(below)), make)


def body_case(n, mode):
  x, box = bfn.lattice_cloud(n, n)
  L = np.array([box, box, 0.0]) * (MODES[mode] > 0)
  return x, L, tbody._oracle(("pair_once_schedule", n), x, L)


@pytest.mark.parametrize("oversub", OVERSUB)
@pytest.mark.parametrize("chunk_steps", CHUNK_STEPS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", SIZES)
def test_histogram_meets_every_pair_once(ctx, n, mode, chunk_steps, oversub):
  frames, L, r_max, refs = hist_case(n, mode)
  ctx.set_positions(frames[0], 1.0, L, wall=False)
  with _plan(ctx, chunk_steps, oversub):
    got = ctx.pair_histogram(r_max, N_BINS)
  assert got.sum() == n * (n - 1) // 2
  assert np.array_equal(got, refs[0])


@pytest.mark.parametrize("oversub", OVERSUB)
@pytest.mark.parametrize("chunk_steps", CHUNK_STEPS)
@pytest.mark.parametrize("mode", list(MODES))
def test_batch_equals_resident_frame_by_frame(ctx, mode, chunk_steps, oversub):
  frames, L, r_max, refs = hist_case(65, mode, n_frames=3)
  dev = torch.from_numpy(frames).cuda()
  with _plan(ctx, chunk_steps, oversub):
    resident = []
    for f in frames:
      ctx.set_positions(f, 1.0, L, wall=False)
      resident.append(ctx.pair_histogram(r_max, N_BINS))
    batch = [ctx.pair_histogram_frames_device(dev[k:k + 1].contiguous(), L, r_max, N_BINS).cpu().numpy().astype(np.uint64) for k in range(3)]
    all_frames = ctx.pair_histogram_frames_device(dev, L, r_max, N_BINS).cpu().numpy().astype(np.uint64)
  for k in range(3):
    assert np.array_equal(batch[k], resident[k]) and np.array_equal(resident[k], refs[k]) and resident[k].sum() == 65 * 64 // 2
  assert np.array_equal(all_frames, resident[0] + resident[1] + resident[2])


@pytest.mark.parametrize("oversub", OVERSUB)
@pytest.mark.parametrize("chunk_steps", CHUNK_STEPS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["soft", "yukawa"])
def test_blob_energy(ctx, form, n, mode, chunk_steps, oversub):
  r, L, kw, ref = energy_case(n, mode, form)
  with _plan(ctx, chunk_steps, oversub):
    got = tpot._gpu(ctx, r, L, kw)
  tpot._check(got, ref, "%s n=%d %s chunk_steps=%d oversub=%d" % (form, n, mode, chunk_steps, oversub))


@pytest.mark.parametrize("chunk_steps", CHUNK_STEPS)
@pytest.mark.parametrize("form", ["soft", "yukawa"])
def test_blob_energy_with_blobs_behind_the_wall(ctx, form, chunk_steps):
  """z <= 0 at the first and the last caller index, on both sides of a tile edge and in the partial last tile: those tiles'
  units take the loop with the lower-index test"""
  n = 200
  r, L, kw, ref = energy_case(n, "open", form, below=(0, 63, 64, n // 2 + 5, n - 1))
  assert (r[:, 2] <= 0).sum() == 5
  with _plan(ctx, chunk_steps, 1):
    got = tpot._gpu(ctx, r, L, kw)
  tpot._check(got, ref, "%s behind the wall chunk_steps=%d" % (form, chunk_steps))


@pytest.mark.parametrize("oversub", OVERSUB)
@pytest.mark.parametrize("chunk_steps", CHUNK_STEPS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", SIZES)
def test_body_energy(ctx, n, mode, chunk_steps, oversub):
  x, L, ref = body_case(n, mode)
  ctx.set_positions(x, 1.0, L, wall=False)
  with _plan(ctx, chunk_steps, oversub):
    got = ctx.body_body_potential(tbody.EPS, tbody.B)
  tbody._check_energy(got, ref, "n %d %s chunk_steps=%d oversub=%d" % (n, mode, chunk_steps, oversub))
