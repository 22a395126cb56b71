"""The tabulated pair law on the device -- force sweep (TableLaw of sym_force_kernel), energy sweep (the TABLE instances of
potential_kernel), their C ABI and the callers -- against the restatement of tests/_pair_table_numpy.py in extended precision:

    |got - EXT| <= MARGIN * C[family, periodic] * 2^-53 * S          (MARGIN = 4)

with the per-pair scales S_U, S_F of that module (the rounding of the Horner form plus the conditioning on r) and its yardstick C
(the float64 restatement's own worst ratio, measured on the CPU by tests/test_pair_table_host.py).  At and beyond r_cut every
output bit is zero.  The worst ratio per family is printed (`-s`) and kept in RESULTS; profiles/r27_pair_table_bounds.txt
records a run."""
import ctypes

import numpy as np
import pytest

import _pair_forces_numpy as pf
import _pair_table_numpy as pt
from _pair_table_numpy import EXT, MARGIN

pytestmark = pytest.mark.gpu
RESULTS = {}
STATE = -2          # RMB_ERR_STATE


@pytest.fixture(autouse=True)
def _ieee():
  with pf.ieee_denormals():
    yield


@pytest.fixture(scope="module")
def Ctx():
  assert pt.LONG_DOUBLE, "np.longdouble has no 64-bit mantissa here: fp64 would be compared with fp64"
  from rigidmultiblobswall_amd import MobilityContext
  return MobilityContext


def _open(Ctx, r, L, T, options=None):
  ctx = Ctx(0)
  for key, val in (options or {}).items():
    ctx.set_option(key, val)
  ctx.set_positions(np.ascontiguousarray(r), 1.0, np.zeros(3) if L is None else L, wall=False)
  ctx.set_pair_table(T)
  return ctx


def _record(key, ratio):
  RESULTS[key] = max(RESULTS.get(key, 0.0), ratio)
  print("%-44s worst %.3f C" % (" ".join(str(k) for k in key), ratio))


def _check_forces(key, got, F, S, periodic, zeros=None):
  assert got.shape == F.shape and np.all(np.isfinite(got)), key
  q = pt.ratios(got, F, S, pt.C["force", periodic])
  _record(key + ("force",), float(q.max()))
  i, k = np.unravel_index(int(np.argmax(q)), q.shape)
  assert q.max() <= MARGIN, "%s: blob %d component %d off by %.3g C (bound %g C): got %.17g, extended precision %s, scale %s" % (
      key, i, k, q.max(), MARGIN, got[i, k], np.format_float_scientific(F[i, k], precision=20), np.format_float_scientific(S[i, k], precision=6))
  if zeros is not None:
    assert len(zeros) >= 4 and pt.is_positive_zero(got[zeros]), "%s: a blob beyond r_cut of every neighbour got %r" % (key, got[zeros])


def _check_energy(key, got, U, S, periodic):
  q = float(pt.ratios(got, U, S, pt.C["energy", periodic]))
  _record(key + ("energy",), q)
  assert np.isfinite(got) and q <= MARGIN, "%s: energy off by %.3g C (bound %g C): got %.17g, extended precision %s, scale %s" % (
      key, q, MARGIN, got, np.format_float_scientific(U, precision=20), np.format_float_scientific(S, precision=6))


def _pair_energy(ctx, T):
  u_one, u_pair = ctx.blob_potential(0.0, 1.0, 0.5, pair_table=T)
  assert pt.is_positive_zero(u_one)
  return u_pair


# ---------------------------------------------------------------------------------------------------------------------
# 1. two blobs over the ladder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [False, True], ids=["open", "box"])
@pytest.mark.parametrize("K", [1, 1024])
def test_two_blobs_over_the_ladder(Ctx, K, box):
  T = pt.lj_table(K)
  ctx = Ctx(0)
  try:
    ctx.set_pair_table(T)
    for rung in pt.RUNGS:
      r, L = pt.ladder_pair(T, rung, box)
      ctx.set_positions(r, 1.0, np.zeros(3) if L is None else L, wall=False)
      got = ctx.pair_table_force()
      assert ctx.get_option("last_path") == 1
      u = _pair_energy(ctx, T)
      F, S = pt.forces(T, r, L)
      U, SU = pt.energy(T, r, L)
      _check_forces(("ladder", K, "box" if box else "open", rung), got, F, S, box)
      _check_energy(("ladder", K, "box" if box else "open", rung), u, U, SU, box)
      assert np.array_equal(got[0], -got[1]), (rung, got)
      if rung in ("cut", "beyond"):
        assert pt.is_positive_zero(got) and pt.is_positive_zero(u), (rung, got, u)
      if rung == "zero":
        assert pt.is_positive_zero(got) and u != 0.0
      if rung in ("half_r0", "in_first", "in_last"):
        assert got[0, 0] != 0.0 and u != 0.0
  finally:
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. clouds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["open", "box", "box3"])
@pytest.mark.parametrize("size", pt.SIZES)
def test_cloud_forces_and_energy(Ctx, size, variant):
  T = pt.lj_table(1024)
  r, L = pt.cloud(size, variant)
  F, S = pt.force_reference(T, size, variant)
  ctx = _open(Ctx, r, L, T)
  try:
    got = ctx.pair_table_force()
    assert ctx.get_option("last_path") == 1
    _check_forces(("cloud", size, variant), got, F, S, L is not None, zeros=pt.loners(T, r, L))
    dev = ctx.pair_table_force_device().cpu().numpy().reshape(-1, 3)
    _check_forces(("cloud_device_entry", size, variant), dev, F, S, L is not None, zeros=pt.loners(T, r, L))
    if variant != "box3":      # the blob energy takes no image in z
      U, SU = pt.energy_reference(T, size, variant)
      _check_energy(("cloud", size, variant), _pair_energy(ctx, T), U, SU, L is not None)
  finally:
    ctx.close()


@pytest.mark.parametrize("K", [1, 16])
def test_cloud_with_a_table_that_jumps_at_r_cut(Ctx, K):
  """shift="none": the law is not zero at r_cut; the builder keeps every pair 1e-9 r_cut away from it."""
  T = pt.lj_table(K, "none")
  for variant in ("open", "box"):
    r, L = pt.cloud(129, variant)
    c = pt.coverage(T, r, L)
    assert c["near_cut"] == 0 and c["beyond"] >= 2 and c["core"] >= 2, c
    ctx = _open(Ctx, r, L, T)
    try:
      F, S = pt.forces(T, r, L)
      _check_forces(("cloud_unshifted", K, variant), ctx.pair_table_force(), F, S, L is not None, zeros=pt.loners(T, r, L))
      U, SU = pt.energy(T, r, L)
      _check_energy(("cloud_unshifted", K, variant), _pair_energy(ctx, T), U, SU, L is not None)
    finally:
      ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. culling and sorting
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["open", "box"])
def test_cull_and_sort_options(Ctx, variant):
  T = pt.lj_table(1024)
  size = 2113
  r, L = pt.cloud(size, variant)
  F, S = pt.force_reference(T, size, variant)
  U, SU = pt.energy_reference(T, size, variant)
  bound = MARGIN * pt.C["force", L is not None] * pt.EPS64 * S.astype(np.float64)
  results = {}
  for options in (dict(force_cull=0), dict(force_cull=1, force_sort=0), dict(force_cull=1, force_sort=1)):
    ctx = _open(Ctx, r, L, T, options)
    try:
      label = "cull%d_sort%d" % (options["force_cull"], options.get("force_sort", 1))
      got = ctx.pair_table_force()
      assert ctx.get_option("last_path") == 1
      _check_forces((label, size, variant), got, F, S, L is not None, zeros=pt.loners(T, r, L))
      _check_energy((label, size, variant), _pair_energy(ctx, T), U, SU, L is not None)
      assert ctx.get_option("last_path") == 1
      results[label] = got
    finally:
      ctx.close()
  base = results["cull1_sort1"]
  for label, got in results.items():      # atomic flushes: two runs agree within the bound of both
    assert np.all(np.abs(got - base) <= 2.0 * bound), label


# ---------------------------------------------------------------------------------------------------------------------
# 4. a Yukawa table against the built-in law
# ---------------------------------------------------------------------------------------------------------------------
def _centres():
  rng = np.random.RandomState(129)
  g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(float)
  r = g[rng.permutation(len(g))[:129]] * 0.8 + 0.12 * (2.0 * rng.rand(129, 3) - 1.0)
  r[:, 2] += 1.0
  R = pt.pair_distances(r)
  assert R.min() >= pt.YUK["r0"] and (R < pt.YUK["r_cut"]).sum() > 129 * 100
  return r


def test_yukawa_table_against_the_built_in_law(Ctx):
  """129 centres no closer than r0 = b, open boundaries, every z > 0: the force-shifted table eps exp(-r/b)/r on [0.5, 8],
  K = 1024, against body_body_force / body_body_potential.  Per pair inside r_cut the table is the interpolant of
  U - U(r_c) - (r - r_c) U'(r_c): the shift terms are added back and the built-in law's pairs beyond r_c taken off, both in
  extended precision.  Tolerance per pair: the Hermite bounds h^4/384 max|U''''| (energy) and sqrt(3)/216 h^3 max|U''''|
  (force, weighted |d_k|/r), plus the rounding bound of each side (this module's and tests/_pair_forces_numpy.py's)."""
  T = pt.yukawa_table("force")
  eps, b, rc = pt.YUK["eps"], pt.YUK["b"], EXT(T.r_cut)
  r = _centres()
  ctx = _open(Ctx, r, None, T)
  try:
    f_tab, u_tab = ctx.pair_table_force(), _pair_energy(ctx, T)
    f_law, u_law = ctx.body_body_force(eps, b), ctx.body_body_potential(eps, b)
  finally:
    ctx.close()
  Uf, dUf = pt.yukawa(eps, b)
  x = r.astype(EXT)
  d = x[None, :, :] - x[:, None, :]
  rr = np.sqrt((d * d).sum(axis=-1))
  np.fill_diagonal(rr, np.inf)
  inside = rr < rc
  Uc, dUc = Uf(rc), dUf(rc)
  w = np.abs(d) / rr[..., None]
  with np.errstate(invalid="ignore"):
    shift_F = np.sum(np.where(inside, dUc / rr, EXT(0))[..., None] * d, axis=1)
    tail_F = np.sum(np.where(inside | np.isinf(rr), EXT(0), dUf(rr) / rr)[..., None] * d, axis=1)
    iu = np.triu(np.ones_like(inside), 1)
    shift_U = np.where(inside & iu, Uc + (rr - rc) * dUc, EXT(0)).sum()
    tail_U = np.where(~inside & iu & np.isfinite(rr), Uf(rr), EXT(0)).sum()
  m4, h = pt.yukawa_d4_max(), EXT(T.h)
  _, S_tab = pt.forces(T, r)
  _, S_law, floor = pf.forces("yukawa", r, None, eps, b, scale=True)
  tol_F = (np.sqrt(EXT(3)) / 216 * h ** 3 * m4) * np.sum(np.where(inside[..., None], w, EXT(0)), axis=1) \
      + MARGIN * EXT(pt.EPS64) * (pt.C["force", False] * S_tab + pf.C["yukawa", False] * S_law) + floor
  err_F = np.abs((f_tab.astype(EXT) + shift_F) - (f_law.astype(EXT) - tail_F))
  _record(("yukawa_vs_law", "force"), float((err_F / tol_F).max()))
  assert np.all(err_F <= tol_F), float((err_F / tol_F).max())
  _, SU_tab = pt.energy(T, r)
  _, SU_law, floor_U, _ = pf.energy("body", r, None, eps, b)
  tol_U = h ** 4 / 384 * m4 * (inside & iu).sum() + MARGIN * EXT(pt.EPS64) * (pt.C["energy", False] * SU_tab + pf.C["body", False] * SU_law) + floor_U
  err_U = abs((EXT(u_tab) + shift_U) - (EXT(u_law) - tail_U))
  _record(("yukawa_vs_law", "energy"), float(err_U / tol_U))
  assert err_U <= tol_U, float(err_U / tol_U)
  assert float((err_F / tol_F).max()) > 1e-3      # the comparison sees the interpolation error, not a slack bound


# ---------------------------------------------------------------------------------------------------------------------
# 6. wall gate and one-blob term
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["soft", "yukawa"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_wall_gate_and_one_blob_term(Ctx, form, where):
  """One blob at z <= 0: listed first it removes every pair it is in (it is the lower index of all of them), listed last
  none.  The one-blob sum is the chosen form's, with 1e5 (1 - z) for that blob."""
  T = pt.lj_table(16)
  r, L = pt.cloud(65, "box")
  r = r.copy()
  low = np.array([r[10, 0] + 0.875, r[10, 1], -0.25])      # next to blob 10, below the wall plane; on the clouds' grid
  r = np.concatenate([[low], r]) if where == "first" else np.concatenate([r, [low]])
  a, eps_w, b_w, weight = 0.25, 2.3, 0.05, 0.7
  ctx = _open(Ctx, r, L, T)
  try:
    u_one, u_pair = ctx.blob_potential(0.0, 1.0, a, repulsion_strength_wall=eps_w, debye_length_wall=b_w, weight=weight, potential=form,
                                       pair_table=T)
    dev = ctx.blob_potential_device(0.0, 1.0, a, repulsion_strength_wall=eps_w, debye_length_wall=b_w, weight=weight, potential=form,
                                    pair_table=T).cpu().numpy()
  finally:
    ctx.close()
  assert dev[0] == u_one and dev[1] == u_pair
  U, SU = pt.energy(T, r, L)
  U_without, _ = pt.energy(T, np.delete(r, 0 if where == "first" else len(r) - 1, axis=0), L)
  gone = abs(U - U_without) <= EXT(2.0) ** -60 * SU        # (two orders of one extended-precision sum)
  assert gone == (where == "first") and (gone or abs(U - U_without) > 1e-6) and abs(U) > 0, (U, U_without)
  _check_energy(("wall_gate", form, where), u_pair, U, SU, True)
  U1, S1 = pt.one_blob(r[:, 2], eps_w, b_w, weight, a, form)
  # the one-blob term is rmb_blob_potential's own: its conditioning 1 + z/b_w as tests/_pair_forces_gpu.run_wall_ladder
  S1 = S1 * (1 + EXT(np.abs(r[:, 2]).max()) / EXT(b_w))
  q = float(pt.ratios(u_one, U1, S1, pf.C["soft" if form == "soft" else "yukawa_energy", False]))
  _record(("wall_gate", form, where, "one_blob"), q)
  assert q <= MARGIN


# ---------------------------------------------------------------------------------------------------------------------
# 9. C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_entry_points_and_state(Ctx):
  import torch
  from rigidmultiblobswall_amd import _lib
  lib = _lib.load()
  T, T1 = pt.lj_table(1024), pt.lj_table(1)
  r, L = pt.cloud(129, "box")
  n = len(r)
  F, S = pt.force_reference(T, 129, "box")
  ctx = Ctx(0)
  try:
    ctx.set_option("force_cull", 0)      # one wave order: host and device entry give the same bits only without a race
    ctx.set_positions(r, 1.0, L, wall=False)
    h = ctx._h
    out = np.zeros(3 * n)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    # no table yet: RMB_ERR_STATE
    assert lib.rmb_pair_table_force(h, vp(out)) == STATE and b"no pair table" in lib.rmb_last_error()
    pot = np.zeros(2)
    assert lib.rmb_blob_potential_table(h, 0.0, 1.0, 0.0, 0.5, 0, vp(pot)) == STATE and b"no pair table" in lib.rmb_last_error()
    c = np.ascontiguousarray(T.coeff)
    assert lib.rmb_ctx_set_pair_table(h, T.r0, T.h, T.K, vp(c)) == 0
    assert lib.rmb_pair_table_force(h, vp(out)) == 0
    first = out.copy().reshape(n, 3)
    _check_forces(("c_abi", "host"), first, F, S, True)
    dev = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    ctx._follow_torch_stream()
    assert lib.rmb_pair_table_force_device(h, ctypes.c_void_p(dev.data_ptr())) == 0
    _check_forces(("c_abi", "device"), dev.cpu().numpy().reshape(n, 3), F, S, True)
    assert lib.rmb_blob_potential_table(h, 0.0, 1.0, 0.0, 0.5, 0, vp(pot)) == 0
    pdev = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert lib.rmb_blob_potential_table_device(h, 0.0, 1.0, 0.0, 0.5, 0, ctypes.c_void_p(pdev.data_ptr())) == 0
    assert np.array_equal(pdev.cpu().numpy(), pot)      # the energy sweep has no atomics: the same bits
    # host and device entry give the same bits: two blobs, one contribution each (the flushes of a cloud are atomics)
    pair, _ = pt.ladder_pair(T, "in_first")
    ctx.set_positions(pair, 1.0, L, wall=False)
    two, two_dev = np.zeros(6), torch.zeros(6, dtype=torch.float64, device="cuda")
    assert lib.rmb_pair_table_force(h, vp(two)) == 0 and lib.rmb_pair_table_force_device(h, ctypes.c_void_p(two_dev.data_ptr())) == 0
    assert two[0] != 0.0 and np.array_equal(two_dev.cpu().numpy(), two)
    ctx.set_positions(r, 1.0, L, wall=False)
    # wall = 1 and a target sub-range are refused
    ctx.set_target_range(0, 64)
    assert lib.rmb_pair_table_force(h, vp(out)) == STATE and b"target range" in lib.rmb_last_error()
    ctx.set_target_range(0, n)
    # K = 1024 -> K = 1 -> K = 1024: the first result again, within the bound
    c1 = np.ascontiguousarray(T1.coeff)
    assert lib.rmb_ctx_set_pair_table(h, T1.r0, T1.h, T1.K, vp(c1)) == 0
    assert lib.rmb_pair_table_force(h, vp(out)) == 0
    F1, S1 = pt.forces(T1, r, L)
    _check_forces(("c_abi", "K1"), out.reshape(n, 3).copy(), F1, S1, True)
    assert lib.rmb_ctx_set_pair_table(h, T.r0, T.h, T.K, vp(c)) == 0
    assert lib.rmb_pair_table_force(h, vp(out)) == 0
    _check_forces(("c_abi", "K1024_again"), out.reshape(n, 3).copy(), F, S, True)
    assert np.all(np.abs(out.reshape(n, 3) - first) <= 2.0 * MARGIN * pt.C["force", True] * pt.EPS64 * S.astype(np.float64))
    # set, clear, ask: RMB_ERR_STATE
    assert lib.rmb_ctx_set_pair_table(h, 0.0, 1.0, 0, None) == 0
    assert lib.rmb_pair_table_force(h, vp(out)) == STATE and b"no pair table" in lib.rmb_last_error()
    assert lib.rmb_pair_table_force_device(h, ctypes.c_void_p(dev.data_ptr())) == STATE
    assert lib.rmb_blob_potential_table_device(h, 0.0, 1.0, 0.0, 0.5, 0, ctypes.c_void_p(pdev.data_ptr())) == STATE
    ctx.set_positions(r, 1.0, L, wall=True)
    assert lib.rmb_ctx_set_pair_table(h, T.r0, T.h, T.K, vp(c)) == 0
    assert lib.rmb_pair_table_force(h, vp(out)) == STATE and b"wall = 0" in lib.rmb_last_error()
  finally:
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. sampler
# ---------------------------------------------------------------------------------------------------------------------
def test_sampler_runs_a_table(tmp_path, monkeypatch):
  """Four 15-blob boomerangs, 20 steps, moves="all", both one-blob forms: every energy the device sampler logs (the start
  energy and every proposal's: the running energy is one of them after every step) against the restatement's of the same
  proposal within the bound, and the same accept/reject sequence for the same seed."""
  import _mcmc_moves_common as mc
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  from rigidmultiblobswall_amd.read_input import ReadInput
  T = pt.lj_table(1024)
  boom, _ = mc.vertex_sets()
  deck = mc.layout([boom] * 4, 1.6, 1.4, 11)
  a, g, kT, eps_w, b_w = 0.2, 0.6, 0.05, 0.8, 0.12
  lines = ("n_steps 20\nn_save 1\ninitial_step 0\ng %r\nblob_radius %r\nkT %r\nperiodic_length 8 8 0\nrepulsion_strength_wall %r\n"
           "debye_length_wall %r\nrepulsion_strength 0.35\ndebye_length 0.09\nseed 5\noutput_name run\n" % (g, a, kT, eps_w, b_w))
  path = mc.write_deck(str(tmp_path), deck, [("structure", "boom", [0, 1, 2, 3])], lines)
  monkeypatch.chdir(tmp_path)
  L = np.array([8.0, 8.0, 0.0])
  for form in ("soft", "yukawa"):
    scales = []

    def energy(r, form=form):
      U, S = pt.energy(T, r, L)
      U1, S1 = pt.one_blob(r[:, 2], eps_w, b_w, g, a, form)
      scales.append(pt.C["energy", True] * S + pf.C["soft" if form == "soft" else "yukawa_energy", False] * S1 * (1 + EXT(np.abs(r[:, 2]).max()) / EXT(b_w)))
      return float(U + U1)
    cpu = MCMCSampler(ReadInput(path), potential=form, energy=energy, write_files=False).run()
    gpu = MCMCSampler(ReadInput(path), device=0, potential=form, write_files=False, pair_table=T, gr=(3.0, 16))
    try:
      gpu.run()
      assert gpu.accepted == cpu.accepted and 0 < sum(cpu.accepted) < 20 and len(cpu.accepted) == 20, (cpu.accepted, gpu.accepted)
      assert len(gpu.energy_log) == len(cpu.energy_log) == len(scales) == 21
      q = max(abs(eg - ec) / (MARGIN * pt.EPS64 * float(s)) for eg, ec, s in zip(gpu.energy_log, cpu.energy_log, scales))
      _record(("sampler", form, "energy_log"), q * MARGIN)
      assert q <= 1.0 + 1e-3      # (the restatement's total was rounded to float64 once: 2^-53 of a sum the scale bounds)
      # a fresh evaluation of the current configuration (the sampler's own: blob_potential(..., pair_table=T) of the coordinates
      # composed anew from the accepted locations and quaternions) against the running energy
      running = ([gpu.energy_log[0]] + [e for e, ok in zip(gpu.energy_log[1:], gpu.accepted) if ok])[-1]
      fresh = gpu.state.current_energy()
      assert abs(fresh - running) <= 2 * MARGIN * pt.EPS64 * float(max(scales)), (fresh, running)
      assert gpu.gr_frames > 0 and np.sum(gpu.gr_counts) > 0          # --gr keeps working
    finally:
      gpu.close()
  with pytest.raises(ValueError, match="single"):
    MCMCSampler(ReadInput(path), device=0, write_files=False, pair_table=T, moves="single")


# ---------------------------------------------------------------------------------------------------------------------
# 8. steppers
# ---------------------------------------------------------------------------------------------------------------------
STEP_TOL = 1e-7          # the deterministic tolerance of the body-body hook tests (tests/test_gpu_body_forces.py)


def _numpy_pair_forces(T, L):
  import torch

  def f(r):
    F, _ = pt.forces(T, r.detach().cpu().numpy(), L)
    return torch.as_tensor(F.astype(np.float64), device=r.device)
  return f


def _roller_start():
  rng = np.random.RandomState(16)
  g = np.stack(np.meshgrid(np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 2) * 1.05
  x = np.concatenate([g + 0.05 * rng.randn(16, 2), 1.0 + 0.1 * rng.rand(16, 1)], axis=1)
  x[:, :2] -= x[:, :2].min(axis=0) - 0.25       # inside the cell: pairs across its faces
  return np.round(x / pt.GRID) * pt.GRID, np.array([4.0, 4.0, 0.0])      # the exact grid of the box clouds


def test_roller_stepper_runs_a_table(tmp_path):
  """16 rollers, two steps of deterministic_adams_bashforth_rollers with blob_pair_table = T against the same integrator fed
  the restatement's forces through calc_blob_blob_forces; then a `table_hip` deck against the attribute."""
  from rigidmultiblobswall_amd.pair_table import PairTable
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rollers
  T = pt.lj_table(16)
  T.save(str(tmp_path / "lj.table"))
  T = PairTable.load(str(tmp_path / "lj.table"))          # the table the deck will read
  x, L = _roller_start()
  scheme, a, eta, dt = "deterministic_adams_bashforth_rollers", 0.4, 1.1, 0.02

  def make(**kw):
    integ = rollers.RollersIntegrator(x, scheme, a, eta, device="cuda:0", **kw)
    integ.periodic_length = L.copy()
    integ.omega_one_roller = np.array([0.0, 2.0, 0.0])
    integ.repulsion_strength, integ.debye_length = 0.7, 0.1      # a table REPLACES the contact law
    return integ
  tab, ref = make(), make()
  tab.blob_pair_table = T
  ref.repulsion_strength = 0.0
  ref.calc_blob_blob_forces = _numpy_pair_forces(T, L)
  f_tab = tab.calc_blob_blob_forces(tab.location).cpu().numpy()
  F, S = pt.forces(T, x, L)
  assert np.abs(F).max() > 1e-3
  _check_forces(("roller_hook",), f_tab, F, S, True)
  for integ in (tab, ref):
    for step in range(2):
      integ.advance_time_step(dt, step=step)
  xt, xr = tab.location.cpu().numpy(), ref.location.cpu().numpy()
  moved = np.abs(xr - x).max()
  assert moved > 1e-4 and np.abs(xt - xr).max() < STEP_TOL * moved, (np.abs(xt - xr).max(), moved)
  # the deck
  (tmp_path / "blob.vertex").write_text("1\n0 0 0\n")
  with open(tmp_path / "rollers.clones", "w") as fh:
    fh.write("16\n" + "".join("%.17g %.17g %.17g 1.0 0.0 0.0 0.0\n" % tuple(p) for p in x))
  lines = [("scheme", scheme), ("mobility_vector_prod_implementation", "hip"), ("blob_blob_force_implementation", "table_hip"),
           ("blob_blob_pair_table", "lj.table"), ("domain", "single_wall"), ("repulsion_strength", "0.7"), ("debye_length", "0.1"),
           ("repulsion_strength_wall", "0"), ("g", "0"), ("dt", "%r" % dt), ("n_steps", "2"), ("eta", "%r" % eta), ("blob_radius", "%r" % a),
           ("kT", "0"), ("omega_one_roller", "0 2 0"), ("periodic_length", "4 4 0"), ("seed", "1"), ("output_name", str(tmp_path / "run")),
           ("structure", "blob.vertex rollers.clones")]
  (tmp_path / "inputfile.dat").write_text("".join("%-40s %s\n" % kv for kv in lines))
  deck = rollers.integrator_from_input(ReadInput(str(tmp_path / "inputfile.dat")), device="cuda:0")
  assert deck.blob_pair_table is not None and np.array_equal(deck.blob_pair_table.coeff, T.coeff)
  for step in range(2):
    deck.advance_time_step(dt, step=step)
  assert np.abs(deck.location.cpu().numpy() - xt).max() < STEP_TOL * moved
  for integ in (tab, ref, deck):
    integ.close()


def test_rigid_stepper_runs_a_table():
  """4 twelve-blob shells, two steps of deterministic_adams_bashforth with blob_pair_table = T against the same integrator
  whose blob-force hook adds the restatement's pair forces to the one-blob forces."""
  import _mcmc_moves_common as mc
  from rigidmultiblobswall_amd.rigid_integrator import RigidIntegrator
  T = pt.lj_table(16)
  _, shell = mc.vertex_sets()
  deck = mc.layout([shell] * 4, 1.5, 1.6, 21)
  a, eta, dt = 0.2, 1.0, 0.02

  def make():
    integ = RigidIntegrator([shell] * 4, deck.loc, deck.quat, "deterministic_adams_bashforth", a, eta, device="cuda:0")
    integ.g = 0.3
    integ.repulsion_strength, integ.debye_length = 0.7, 0.1      # a table REPLACES the contact law
    return integ
  tab, ref = make(), make()
  tab.blob_pair_table = T
  ref.repulsion_strength = 0.0
  pair = _numpy_pair_forces(T, None)
  one_blob = ref._blob_forces
  ref.calc_blob_forces = lambda r: one_blob(r) + pair(r)
  assert np.abs(pt.forces(T, deck.blobs())[0]).max() > 1e-3
  for integ in (tab, ref):
    for step in range(2):
      integ.advance_time_step(dt, step=step)
  xt, xr = tab.location.cpu().numpy(), ref.location.cpu().numpy()
  qt, qr = tab.orientation.cpu().numpy(), ref.orientation.cpu().numpy()
  moved = np.abs(xr - deck.loc).max()
  assert moved > 1e-4 and np.abs(xt - xr).max() < STEP_TOL * moved and np.abs(qt - qr).max() < STEP_TOL, (np.abs(xt - xr).max(), moved)
  for integ in (tab, ref):
    integ.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. F = -grad U
# ---------------------------------------------------------------------------------------------------------------------
def test_force_is_minus_the_gradient_of_the_energy(Ctx):
  """65 blobs in a box (Lx, Ly, 0), every z > 0, K = 16: for a direction D (a random unit vector of R^3N, put on the grid 2^-10
  so that x +- delta D is exact for delta = 2^-12) the force sweep's -sum_i F_i . D_i against the central difference
  g = (E(x + delta D) - E(x - delta D)) / (2 delta) of the energy sweep.

  Tolerance, pair by pair, with phi(s) = u(r(s)), r(s) = |d + s w|, w = D_j - D_i, v = |w|, |s| <= delta, so that
  |r'| <= v, |r''| <= v^2/r, |r'''| <= 3 v^3/r^2 and r >= r_min = r(0) - delta v:
    * inside one polynomial piece phi is smooth and g_pair - phi'(0) = delta^2/6 phi'''(xi):
        |phi'''| <= |u'''| v^3 + 3 |u''| v^3/r_min + 3 |u'| v^3/r_min^2,
      with the cubic's exact |u'''| = 6 |c3|/h^3 and |u''| <= (2|c2| + 6|c3|)/h^2, |u'| <= (|c1| + 2|c2| + 3|c3|)/h on the piece
      (core: u'' = u''' = 0, |u'| = |c[0][1]|/h; beyond r_cut: nothing);
    * a pair whose range [r - delta v, r + delta v] meets a breakpoint (a knot, r0, r_cut) has phi' Lipschitz only:
      |g_pair - phi'(0)| <= delta/2 max|phi''|, |phi''| <= |u''| v^2 + |u'| v^2/r_min over the pieces it touches, plus the
      interpolant's defect there -- the four coefficients are rounded once each, so u jumps by at most 2 2^-53 sum|c| at a knot,
      which the difference divides by 2 delta (both bounds are charged to such a pair);
    * rounding: the two energies' bounds MARGIN C 2^-53 S over 2 delta, and the forces' bounds times |D|."""
  T = pt.lj_table(16)
  r, L = pt.cloud(65, "box")
  n, delta = len(r), 2.0 ** -12
  assert np.all(r[:, 2] > 0)
  D = np.random.RandomState(5).randn(n, 3)
  D = np.round(D / np.linalg.norm(D) * 1024.0) / 1024.0
  rp, rm = r + delta * D, r - delta * D
  assert np.array_equal((rp - r) / delta, D) and np.array_equal((r - rm) / delta, D) and abs(np.linalg.norm(D) - 1.0) < 1e-2
  ctx = _open(Ctx, r, L, T)
  try:
    F = ctx.pair_table_force()
    ctx.set_positions(rp, 1.0, L, wall=False)
    Ep = _pair_energy(ctx, T)
    ctx.set_positions(rm, 1.0, L, wall=False)
    Em = _pair_energy(ctx, T)
  finally:
    ctx.close()
  lhs = -(F.astype(EXT) * D.astype(EXT)).sum()
  g = (EXT(Ep) - EXT(Em)) / EXT(2 * delta)
  # per-piece maxima: piece 0 = core, 1 .. K = intervals, K + 1 = beyond
  a = np.abs(T.coeff.astype(EXT))
  h, K = EXT(T.h), T.K
  du = np.concatenate([[a[0, 1] / h], (a[:, 1] + 2 * a[:, 2] + 3 * a[:, 3]) / h, [EXT(0)]])
  d2 = np.concatenate([[EXT(0)], (2 * a[:, 2] + 6 * a[:, 3]) / h ** 2, [EXT(0)]])
  d3 = np.concatenate([[EXT(0)], 6 * a[:, 3] / h ** 3, [EXT(0)]])
  jump = np.concatenate([[a[0].sum()], a.sum(axis=1), [a[-1].sum()]]) * 2 * EXT(pt.EPS64)

  def piece(rho):
    x = (rho - EXT(T.r0)) / h
    return np.where(rho < EXT(T.r0), 0, np.where(rho >= EXT(T.r_cut), K + 1, np.minimum(np.floor(x), K - 1) + 1)).astype(int)
  ii, jj = np.triu_indices(n, 1)
  d = pt._image((r[jj] - r[ii]).astype(EXT), pt._period(L), EXT, (0, 1))
  rr = np.sqrt((d * d).sum(axis=1))
  v = np.sqrt((((D[jj] - D[ii]).astype(EXT)) ** 2).sum(axis=1))
  lo, hi = piece(rr - delta * v), piece(rr + delta * v)
  r_min = rr - delta * v
  assert r_min.min() > 0.1
  span = [np.arange(l, u + 1) for l, u in zip(lo, hi)]
  mx = lambda tab: np.array([tab[s].max() for s in span], dtype=EXT)      # noqa: E731
  DU, D2, D3, J = mx(du), mx(d2), mx(d3), mx(jump)
  M3 = D3 * v ** 3 + 3 * D2 * v ** 3 / r_min + 3 * DU * v ** 3 / r_min ** 2
  M2 = D2 * v ** 2 + DU * v ** 2 / r_min
  crossing = hi > lo
  trunc = (EXT(delta) ** 2 / 6 * M3).sum()
  knots = np.where(crossing, EXT(delta) / 2 * M2 + J / EXT(2 * delta), EXT(0)).sum()
  Sp, Sm = pt.energy(T, rp, L)[1], pt.energy(T, rm, L)[1]
  _, S_F = pt.forces(T, r, L)
  rounding = MARGIN * EXT(pt.EPS64) * (pt.C["energy", True] * (Sp + Sm) / EXT(2 * delta) + pt.C["force", True] * (S_F * np.abs(D)).sum())
  tol = trunc + knots + rounding
  print("F.D %.6e, difference %.3e, tolerance %.3e = third derivative %.3e + %d knot crossings %.3e + rounding %.3e"
        % (float(lhs), float(abs(lhs - g)), float(tol), float(trunc), int(crossing.sum()), float(knots), float(rounding)))
  _record(("gradient", "K16"), float(abs(lhs - g) / tol) * MARGIN)
  assert crossing.sum() >= 1 and abs(lhs) > 100 * tol          # the tolerance is a small part of what is compared
  assert abs(lhs - g) <= tol
