"""Potential energy of a blob configuration on the GPU (rmb_blob_potential) against the long-double restatement
(_potential_numpy.py), bound |dU| <= 1e-13 sum|terms| -- the Laplace operators' bound applied to the energy's absolute-term
sum; the reference kernel's index semantics behind the wall, the special distances, bit-reproducibility, and consistency
of U_pair with the blob-blob forces."""
import ctypes

import numpy as np
import pytest
import torch

import _potential_numpy as potnp

pytestmark = pytest.mark.gpu

A = 0.31
BOUND = 1e-13
WORST = {"ratio": 0.0}     # largest |dU| / sum|terms| seen by this module (printed when the context fixture is torn down)


def _params(form, wall_terms, n):
  # a short screening length for the large clouds: the neighbour-list restatement then stays small (see _reference)
  b = (0.05 if form == "soft" else 0.1) * A if n > 2000 else 0.4 * A
  kw = dict(repulsion_strength=0.7, debye_length=b, blob_radius=A, weight=0.9 if wall_terms else 0.0, potential=form)
  if wall_terms:
    kw.update(repulsion_strength_wall=1.3, debye_length_wall=0.5 * A)
  return kw


def _cloud(n, seed, periodic):
  """Random cloud above the wall, some overlapping pairs and some blobs below z = a; side = the periodic length."""
  rng = np.random.RandomState(seed)
  side = 2.2 * A * max(n, 8) ** (1.0 / 3.0)
  r = np.column_stack([side * rng.rand(n), side * rng.rand(n), 0.2 * A + side * rng.rand(n)])
  L = np.array([side if periodic >= 1 else 0.0, side if periodic >= 2 else 0.0, 0.0])
  if periodic:
    r[::7, 0] += side          # positions need not lie in one cell
    r[::11, 0] -= 2 * side
  return r, L


def _reference(r, L, kw):
  """Restatement; from 2000 blobs on only the pairs within 2a + 120 b (yukawa 120 b): every dropped term is below
  e^-120 = 8e-53 of the strength, N^2 / 2 of them stay 30 orders under the bound."""
  n = r.shape[0]
  if n <= 2000:
    return potnp.energy(r, periodic_length=L, split=True, **kw)
  b = kw["debye_length"]
  reach = (2 * A if kw["potential"] == "soft" else 0.0) + 120 * b
  return potnp.energy(r, periodic_length=L, method="neighbours", reach=reach, split=True, **kw)


def _gpu(ctx, r, L, kw):
  ctx.set_positions(r, A, L, wall=False)
  kw = dict(kw)
  eps, b, a = kw.pop("repulsion_strength"), kw.pop("debye_length"), kw.pop("blob_radius")
  return ctx.blob_potential(eps, b, a, **kw)


def _check(got, ref, what=""):
  """The bound on the total, and -- stricter -- on each of the two sums against its own absolute-term sum (a yukawa blob
  below z = a adds 1e12 e_w to the one-blob sum: the total's scale alone would say nothing about the pair sum then)."""
  u1, u2, S1, S2 = ref
  d1, d2 = abs(potnp.EXT(got[0]) - u1), abs(potnp.EXT(got[1]) - u2)
  dt = abs(potnp.EXT(got[0]) + potnp.EXT(got[1]) - (u1 + u2))
  ratio = max(float(d / S) if S > 0 else float(d) for d, S in ((d1, S1), (d2, S2), (dt, S1 + S2)))
  WORST["ratio"] = max(WORST["ratio"], ratio)
  print("%s |dU_one| %.3e of %.6e  |dU_pair| %.3e of %.6e  |dU| %.3e  worst ratio %.3e" % (what, d1, S1, d2, S2, dt, ratio))
  assert dt <= BOUND * (S1 + S2) and d1 <= BOUND * S1 and d2 <= BOUND * S2, (what, float(d1), float(S1), float(d2), float(S2), float(dt))


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()
  print("worst |dU| / sum|terms| of this module = %.3e (bound %.1e)" % (WORST["ratio"], BOUND))     # DESIGN 4 quotes it


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 1025, 24577])
@pytest.mark.parametrize("periodic", [0, 1, 2], ids=["open", "per_x", "per_xy"])
@pytest.mark.parametrize("wall_terms", [False, True], ids=["nowall", "wall"])
@pytest.mark.parametrize("form", ["soft", "yukawa"])
def test_parity_with_the_restatement(ctx, form, wall_terms, periodic, n):
  r, L = _cloud(n, 100 + n, periodic)
  kw = _params(form, wall_terms, n)
  _check(_gpu(ctx, r, L, kw), _reference(r, L, kw), "%s n=%d" % (form, n))


def _monolayer(n, seed):
  rng = np.random.RandomState(seed)
  m = int(np.ceil(np.sqrt(n)))
  g = 2.2 * A
  ix, iy = np.divmod(np.arange(n), m)
  r = np.column_stack([g * ix + 0.2 * A * rng.randn(n), g * iy + 0.2 * A * rng.randn(n), A * (1.05 + 0.5 * rng.rand(n))])
  return r, np.array([g * m, g * m, 0.0])


@pytest.mark.parametrize("form", ["soft", "yukawa"])
def test_parity_on_a_monolayer_of_1e5_blobs(ctx, form):
  r, L = _monolayer(100000, 3)
  r = r[np.random.RandomState(4).permutation(r.shape[0])]      # listed at random: the Morton sort has work to do
  kw = _params(form, True, r.shape[0])
  _check(_gpu(ctx, r, L, kw), _reference(r, L, kw), "monolayer %s" % form)


# ---- semantics of the reference kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["soft", "yukawa"])
@pytest.mark.parametrize("n", [130, 2200], ids=["caller_order", "morton_sorted"])
def test_blobs_behind_the_wall_follow_the_lower_index_rule(ctx, form, n):
  """z <= 0 at the first, a middle and the last caller index and on both sides of a tile edge; the same cloud listed in
  reverse must match the restatement too, and the two orders differ by exactly the pairs with one blob behind the wall:
  such a pair counts only in the order that lists its blob ABOVE the wall first."""
  r, L = _cloud(n, 7, 0)
  below = np.array([0, 63, 64, n // 2 + 5, n - 1])
  r[below, 2] = [-0.3, 0.0, -1e-9, -2.0, -0.05]
  kw = _params(form, True, 100)
  fwd, rev = _gpu(ctx, r, L, kw), _gpu(ctx, r[::-1].copy(), L, kw)
  ref_f, ref_r = _reference(r, L, kw), _reference(r[::-1].copy(), L, kw)
  _check(fwd, ref_f, "forward")
  _check(rev, ref_r, "reversed")
  a, eps, b = potnp.EXT(A), potnp.EXT(kw["repulsion_strength"]), potnp.EXT(kw["debye_length"])
  x = r.astype(potnp.EXT)
  predicted = potnp.EXT(0)
  up = np.setdiff1d(np.arange(n), below)
  for p in below:
    t = potnp.pair_terms(x[p][None, :] - x[up], L, eps, b, a, form)
    predicted += np.where(up < p, t, -t).sum(dtype=potnp.EXT)
  S = ref_f[3]
  assert abs(predicted) > 1e-6 * S                      # the rule matters for this cloud
  assert abs((potnp.EXT(fwd[1]) - potnp.EXT(rev[1])) - predicted) <= 2 * BOUND * S
  assert fwd[0] == pytest.approx(rev[0], rel=1e-14)     # the one-blob sum does not depend on the order


def test_coincident_blobs(ctx):
  r = np.array([[0.3, 0.4, 1.0], [0.3, 0.4, 1.0]])
  kw = _params("soft", False, 2)
  u = _gpu(ctx, r, np.zeros(3), kw)
  contact = kw["repulsion_strength"] + 2 * A * kw["repulsion_strength"] / kw["debye_length"]
  assert np.isfinite(u[1]) and abs(u[1] - contact) <= 4e-16 * contact
  u = _gpu(ctx, r, np.zeros(3), _params("yukawa", False, 2))
  assert u[1] == np.inf


@pytest.mark.parametrize("form", ["soft", "yukawa"])
def test_special_distances(ctx, form):
  a = 0.25                                   # 2a = 0.5 and L / 2 = 4 are exact in binary
  kw = dict(repulsion_strength=0.7, debye_length=0.1, blob_radius=a, weight=0.9, repulsion_strength_wall=1.3, debye_length_wall=0.125,
            potential=form)
  cases = [(np.array([[0.0, 0.0, 1.0], [0.5, 0.0, 1.0]]), np.zeros(3)),            # r = 2a exactly
           (np.array([[0.0, 0.0, 0.25], [3.0, 0.0, 2.0]]), np.zeros(3)),           # z = a exactly (yukawa: e_w a / 0 = inf)
           (np.array([[1.0, 2.0, 1.0], [5.0, 2.0, 1.0]]), np.array([8.0, 0.0, 0.0])),   # exactly L / 2 apart in x
           (np.array([[1.0, 6.5, 1.0], [1.0, 2.5, 1.0]]), np.array([8.0, 8.0, 0.0]))]   # ... and in y, the other sign
  for r, L in cases:
    ctx.set_positions(r, a, L, wall=False)
    got = ctx.blob_potential(0.7, 0.1, a, repulsion_strength_wall=1.3, debye_length_wall=0.125, weight=0.9, potential=form)
    u1, u2, S = potnp.energy(r, periodic_length=L, **kw)
    if np.isinf(float(u1)):
      assert got[0] == float(u1)
    else:
      assert abs(potnp.EXT(got[0]) - u1) <= BOUND * S
    assert abs(potnp.EXT(got[1]) - u2) <= BOUND * S
  if form == "soft":
    ctx.set_positions(cases[0][0], a, np.zeros(3), wall=False)
    assert ctx.blob_potential(0.7, 0.1, a)[1] == 0.7          # exp(0) = 1 exactly at contact


# ---- reproducibility ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["soft", "yukawa"])
def test_bit_reproducible_and_culling_changes_no_bit(ctx, form):
  r, L = _monolayer(24577, 9)
  r = r[np.random.RandomState(1).permutation(r.shape[0])]
  kw = _params(form, True, r.shape[0])
  ref = _reference(r, L, kw)
  try:
    ctx.set_option("potential_resort", 1)                     # a permutation of THIS configuration, whatever ran before
    first = _gpu(ctx, r, L, kw)
    assert _gpu(ctx, r, L, kw) == first                       # two calls
    ctx.set_option("potential_resort", 4)                     # the second of these reuses the permutation of the first
    assert _gpu(ctx, r, L, kw) == first and _gpu(ctx, r, L, kw) == first
    ctx.set_option("potential_resort", 1)
    for sort in (1, 0):
      ctx.set_option("force_sort", sort)
      res = {}
      for cull in (0, 1):
        ctx.set_option("force_cull", cull)
        res[cull] = _gpu(ctx, r, L, kw)
      assert res[0] == res[1], (sort, res)                    # skipped units are exact zeros
      _check(res[1], ref, "sort=%d" % sort)                   # sorted and unsorted agree with the restatement ...
      if sort == 0:
        assert abs(res[1][1] - first[1]) <= BOUND * float(ref[3]) and abs(res[1][0] - first[0]) <= BOUND * float(ref[2])   # ... and with each other
  finally:
    ctx.set_option("force_sort", 1); ctx.set_option("force_cull", 1); ctx.set_option("potential_resort", 16)    # the defaults


def test_caller_order_shuffle_of_a_cloud_above_the_wall(ctx):
  r, L = _cloud(5000, 21, 2)
  kw = _params("soft", True, 5000)
  ref = _reference(r, L, kw)
  u = _gpu(ctx, r, L, kw)
  v = _gpu(ctx, r[np.random.RandomState(2).permutation(5000)], L, kw)
  _check(u, ref, "listed"); _check(v, ref, "shuffled")
  assert abs(u[0] - v[0]) <= BOUND * float(ref[2]) and abs(u[1] - v[1]) <= BOUND * float(ref[3])


# ---- consistency with the forces ---------------------------------------------------------------------------------------
def test_pair_energy_is_the_potential_of_the_blob_blob_forces(ctx):
  """Central difference of U_pair along random directions against -F . delta (rmb_blob_blob_force), h = 1e-5 a: the
  O(h^2) truncation (~1e-10 |F|) and the rounding eps U / h (~1e-8 |F|) are both below 1e-7 |F|."""
  n = 700
  r, L = _cloud(n, 33, 0)
  eps, b = 0.7, 0.4 * A
  ctx.set_positions(r, A, L, wall=False)
  F = ctx.blob_blob_force(eps, b, A)
  rng = np.random.RandomState(5)
  h = 1e-5 * A
  for _ in range(3):
    delta = rng.randn(n, 3)
    delta /= np.linalg.norm(delta)
    ctx.set_positions(r + h * delta, A, L, wall=False)
    up = ctx.blob_potential(eps, b, A)[1]
    ctx.set_positions(r - h * delta, A, L, wall=False)
    um = ctx.blob_potential(eps, b, A)[1]
    fd = (up - um) / (2 * h)
    print("dU/dh %.12e  -F.delta %.12e  |F| %.6e" % (fd, -np.sum(F * delta), np.linalg.norm(F)))
    assert abs(fd + np.sum(F * delta)) <= 1e-7 * np.linalg.norm(F)


# ---- the other entry points --------------------------------------------------------------------------------------------
def test_device_entry_oneshot_and_reference_surface(ctx):
  from rigidmultiblobswall_amd import _lib, potential
  r, L = _cloud(3000, 41, 1)
  kw = _params("yukawa", True, 3000)
  ctx.set_option("potential_resort", 1)      # bit comparisons across contexts: every call builds the permutation of THIS cloud
  host = _gpu(ctx, r, L, kw)
  out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda:0")
  res = ctx.blob_potential_device(kw["repulsion_strength"], kw["debye_length"], A, repulsion_strength_wall=1.3,
                                  debye_length_wall=0.5 * A, weight=0.9, potential="yukawa", out=out)
  assert res is out and tuple(out.cpu().tolist()) == host
  one = np.empty(2)
  rc = _lib.load().rmb_potential_oneshot(3000, ctypes.c_void_p(r.ctypes.data), ctypes.c_void_p(L.ctypes.data), 0.7, kw["debye_length"], 1.3,
                                         0.5 * A, 0.9, A, 1, ctypes.c_void_p(one.ctypes.data))
  assert rc == 0 and tuple(one) == host
  try:
    total = potential.compute_total_energy_hip([], r, periodic_length=L, **kw)
    assert total == host[0] + host[1] and potential.bodies_potential_hip([]) == 0.0
  finally:
    potential.reset()
    ctx.set_option("potential_resort", 16)   # the default
  with pytest.raises(ValueError):
    potential.blobs_potential_hip(r, periodic_length=L, **dict(kw, potential="lennard-jones"))


def test_wrong_state_and_arguments_are_refused(ctx):
  from rigidmultiblobswall_amd._lib import RmbError
  r, L = _cloud(200, 1, 0)
  ctx.set_positions(r, A, L, wall=True)                       # clamped heights: not the sampler's energy
  with pytest.raises(RmbError):
    ctx.blob_potential(0.7, 0.1, A)
  ctx.set_positions(r, A, L, wall=False)
  with pytest.raises(RmbError):
    ctx.blob_potential(0.7, 0.0, A)                           # debye_length
  with pytest.raises(RmbError):
    ctx.blob_potential(0.7, 0.1, A, repulsion_strength_wall=1.0, debye_length_wall=0.0)
  with pytest.raises(ValueError):
    ctx.blob_potential(0.7, 0.1, A, potential="hard")


def test_out_tensor_is_validated(ctx):
  r, L = _cloud(200, 1, 0)
  ctx.set_positions(r, A, L, wall=False)
  bad = [torch.empty(1, dtype=torch.float64, device="cuda:0"),              # short
         torch.empty(4, dtype=torch.float64, device="cuda:0")[::2],         # not contiguous
         torch.empty(2, dtype=torch.float32, device="cuda:0"),              # not fp64
         torch.empty(2, dtype=torch.float64)]                               # host
  for out in bad:
    with pytest.raises(ValueError):
      ctx.blob_potential_device(0.7, 0.1, A, out=out)
