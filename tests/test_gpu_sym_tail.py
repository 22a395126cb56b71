"""One-vector symmetric sweeps (sym2t_kernel, sym_kernel, sym_coop_kernel) at the smallest sizes the two-target rule admits,
with the doubled-height operands of their wall tt instances (sym_kernels.h: kSymZi2).

The dynamic tail this file was first written for -- the last steps of a launch handed out on demand -- was built, passed
these cases with `sym_tail` in {0, 500, 1000} x `sym_tail_piece` in {1, 16, 64} x `sym_min_steps` in {1, 7, 64} at <= 8.4e-16,
and was taken out again because it was slower at every size (profiles/r21_dynamic_tail_rejected.txt,
tools/experiments/dynamic_tail.patch).  What stays are the cases that do not need its options.

Sizes: 193 blobs = 4 tiles, the fewest the two-target rule admits; 257 = 5 tiles, the last row pair has no second row; 449
has a partial last tile; 1000 with ~2 % of the blobs below z = a (height clamp + B damping).  Every case sets
`sym_two_targets` = 2, so that sym2t_kernel (last_path 4) runs at these sizes.

Bound: 1e-13 relative L2, the bound tests/test_gpu_parity.py uses between two runs of one kernel (TOL_SHARD).  Another cut
of the step ranges leaves the pair arithmetic alone, so results differ by the arrival order of the atomics, ~1e-16 per
term; the same bound is asked against the CPU oracle on these small clouds.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-13
SIZES = [193, 257, 449, 1000]
KINDS = ("tt", "tr", "rt", "rr")
ORACLE = {"tt": "mobility_trans_times_force", "tr": "mobility_trans_times_torque", "rt": "mobility_rot_times_force",
          "rr": "mobility_rot_times_torque"}


def cloud(N, seed=None):
  """D2 cloud (5 % volume fraction, a = 0.5) lowered so that about 2 % of the blobs lie below z = a."""
  rng = np.random.RandomState(N if seed is None else seed)
  a, eta = 0.5, 1.0
  Lbox = (N * (4.0 / 3.0) * np.pi * a ** 3 / 0.05) ** (1.0 / 3.0)
  r = rng.rand(N, 3) * Lbox
  r[:, 2] += a - 0.02 * Lbox
  return r, rng.randn(N, 3), eta, a


@pytest.fixture(scope="module")
def Ctx():
  from rigidmultiblobswall_amd import MobilityContext
  return MobilityContext


def make_ctx(Ctx, r, a, wall, **opts):
  ctx = Ctx(0)
  ctx.set_option("sym_two_targets", 2)
  for k, v in opts.items():
    ctx.set_option(k, v)
  ctx.set_positions(r, a, None, wall)
  return ctx


_REF = {}


def default_plan(Ctx, N, wall, kind):
  """The product on the default plan (two targets per lane): computed once per (N, wall, kind), read-only."""
  key = (N, wall, kind)
  if key not in _REF:
    r, v, eta, a = cloud(N)
    ctx = make_ctx(Ctx, r, a, wall)
    try:
      u = ctx.matvec(kind, v, eta)
      assert ctx.get_option("last_path") == 4
    finally:
      ctx.close()
    u.setflags(write=False)
    _REF[key] = u
  return _REF[key]


@pytest.mark.parametrize("wall", [True, False], ids=["wall", "no_wall"])
@pytest.mark.parametrize("N", SIZES)
def test_two_targets_vs_oracle_every_kind(Ctx, oracle, N, wall):
  """Strided chunks of 16 steps, 7 steps per wave at least: ranges begin and end inside units.  Every kind against the CPU
  oracle and against the default plan."""
  r, v, eta, a = cloud(N)
  if N == 1000 and wall:
    assert 8 <= np.sum(r[:, 2] < a) <= 40
  ctx = make_ctx(Ctx, r, a, wall, sym_chunk_steps=16, sym_min_steps=7)
  try:
    for kind in KINDS:
      u = ctx.matvec(kind, v, eta)
      assert ctx.get_option("last_path") == 4, (kind, ctx.get_option("last_path"))
      ref = getattr(oracle, ("single_wall_" if wall else "no_wall_") + ORACLE[kind] + "_oracle")(r, v, eta, a)
      e, e0 = rel_err(u, ref), rel_err(u, default_plan(Ctx, N, wall, kind))
      print("N %d wall %d %s: vs oracle %.2e, vs default plan %.2e" % (N, wall, kind, e, e0))
      assert np.all(np.isfinite(u))
      assert e < TOL, (N, wall, kind, e)
      assert e0 < TOL, (N, wall, kind, e0)
  finally:
    ctx.close()


@pytest.mark.parametrize("two_targets", [2, 0], ids=["sym2t_kernel", "sym_kernel"])
@pytest.mark.parametrize("N", SIZES)
def test_steps_per_wave_equal_default_plan(Ctx, N, two_targets):
  """`sym_min_steps` in {1, 7, 64} with 16-step strided chunks on wall tt, per-wave kernels with one and two targets per lane."""
  r, v, eta, a = cloud(N)
  ctx = make_ctx(Ctx, r, a, True, sym_chunk_steps=16)
  if not two_targets:
    ctx.set_option("sym_two_targets", 0)
    ctx.set_option("sym_coop", 0)
  try:
    for min_steps in (1, 7, 64):
      ctx.set_option("sym_min_steps", min_steps)
      u = ctx.matvec("tt", v, eta)
      assert ctx.get_option("last_path") == (4 if two_targets else 1)
      e = rel_err(u, default_plan(Ctx, N, True, "tt"))
      print("N %d two_targets %d sym_min_steps %d: vs default plan %.2e" % (N, two_targets, min_steps, e))
      assert e < TOL, (N, min_steps, e)
  finally:
    ctx.close()


def test_repeated_products_leave_accumulators_zero(Ctx):
  """Five products with different forces on ONE context: each equals the same product on a fresh context."""
  N = 449
  r, v, eta, a = cloud(N)
  rng = np.random.RandomState(5)
  forces = [rng.randn(N, 3) * (10.0 ** k) for k in range(5)]
  ctx = make_ctx(Ctx, r, a, True, sym_chunk_steps=16)
  try:
    for k, f in enumerate(forces):
      u = ctx.matvec("tt", f, eta)
      assert ctx.get_option("last_path") == 4
      fresh = make_ctx(Ctx, r, a, True, sym_chunk_steps=16)
      try:
        u1 = fresh.matvec("tt", f, eta)
      finally:
        fresh.close()
      assert rel_err(u, u1) < TOL, (k, rel_err(u, u1))
  finally:
    ctx.close()


def test_pair_shards_and_deterministic_equal_full_product(Ctx):
  """A 3-way pair shard adds up to the full product, and deterministic = 1 (one-sided sweep) gives it too."""
  import torch
  N = 1000
  r, v, eta, a = cloud(N)
  vd = torch.as_tensor(v.reshape(-1), device="cuda")
  ctx = make_ctx(Ctx, torch.as_tensor(r.reshape(-1), device="cuda"), a, True)
  try:
    full = ctx.matvec_device("tt", vd, eta).cpu().numpy()
    assert ctx.get_option("last_path") == 4
    assert rel_err(full, default_plan(Ctx, N, True, "tt")) < TOL
    total = np.zeros(3 * N)
    for g in range(3):
      total += ctx.matvec_pairshard_device("tt", vd, eta, g, 3).cpu().numpy()
    assert rel_err(total, full) < TOL, rel_err(total, full)
    ctx.set_option("deterministic", 1)
    d = ctx.matvec_device("tt", vd, eta).cpu().numpy()
    assert ctx.get_option("last_path") == 0
    assert rel_err(d, full) < TOL, rel_err(d, full)
  finally:
    ctx.close()


def test_doubled_height_operands_bit_identical_across_kernels(Ctx):
  """One nonzero source blob: every target's sum is a single term, so the words do not depend on arrival order, and
  sym2t_kernel, sym_kernel and sym_coop_kernel -- which keep 2 z_i in the lane for wall tt -- must agree word for word
  (N = 257; the same products tools/sym_single_source_bits.py prints to compare two builds)."""
  sys.path.insert(0, os.path.join(ROOT, "tools"))
  import sym_single_source_bits as bits
  for source in bits.SOURCES:
    res = bits.products(Ctx, source)
    assert [res[k][0] for k in ("sym2t_kernel", "sym_kernel", "sym_coop_kernel")] == [4, 1, 3]
    w = res["sym2t_kernel"][1].view(np.uint64)
    assert np.count_nonzero(res["sym2t_kernel"][1]) > 3 * (bits.N - 1)
    for name in ("sym_kernel", "sym_coop_kernel"):
      other = res[name][1].view(np.uint64)
      assert np.array_equal(w, other), (source, name, int(np.sum(w != other)))
