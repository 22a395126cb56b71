"""Rotational products above a free (stress-free) surface on the GPU (context option "free_surface_rotation"): every kind
and multi-block operation against the mirror construction over the unbounded oracle (tests/_free_surface_mirror.py), the
paths they take, pair shards, the deterministic pass, what stays refused, and the roller schemes on top of them.

Sizes: 130 = symmetric sweep, two tiles + 2; 257 = a fifth tile with one blob; 24 and 100 = the one-sided sweep."""
import numpy as np
import pytest
import torch

from conftest import rel_err
import _free_surface_mirror as fm

pytestmark = pytest.mark.gpu

ETA, A = 1.1, 0.3
TOL = 1e-13         # the bound of the project's free-surface kernel tests against the oracle
_REF = {}


def _dev(x):
  return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64).reshape(-1), device="cuda")


def _case(oracle, n, periodic):
  """Cloud, two vectors and every mirror product of them, computed once per (n, periodic)."""
  key = (n, periodic)
  if key not in _REF:
    r = fm.cloud(n, A, 5 + n)
    L = fm.periodic_box(n, A) if periodic else None
    rng = np.random.RandomState(100 + n)
    f, t = rng.randn(3 * n), rng.randn(3 * n)
    ref = {"tt_f": fm.product(oracle, "tt", r, f, ETA, A, L), "tr_t": fm.product(oracle, "tr", r, t, ETA, A, L),
           "rt_f": fm.product(oracle, "rt", r, f, ETA, A, L), "rr_t": fm.product(oracle, "rr", r, t, ETA, A, L),
           "tr_f": fm.product(oracle, "tr", r, f, ETA, A, L)}
    _REF[key] = (r, L, f, t, ref)
  return _REF[key]


def _ctx(r, L=None, rotation=1):
  from rigidmultiblobswall_amd import MobilityContext
  ctx = MobilityContext(0)
  ctx.set_option("free_surface_rotation", rotation)
  ctx.set_positions(_dev(r), A, L, wall="free_surface")
  return ctx


@pytest.mark.parametrize("n,periodic", [(24, False), (100, False), (130, False), (257, False), (24, True), (130, True)])
def test_every_kind_and_operation_against_the_mirror_oracle(oracle, n, periodic):
  from rigidmultiblobswall_amd._lib import RmbError
  r, L, f, t, ref = _case(oracle, n, periodic)
  ctx = _ctx(r, L)
  fd, td = _dev(f), _dev(t)
  symmetric = n >= 128

  def path_ok(what):
    chunks = ctx.last_launch()["chunks"]
    assert (chunks == 0) if symmetric else (chunks >= 1), "%s at n = %d took the %s path" % (what, n, "one-sided" if chunks else "symmetric")

  try:
    for rep in range(2):      # the second round: the accumulators were left zeroed
      for kind, vec, want in (("tr", td, ref["tr_t"]), ("rt", fd, ref["rt_f"]), ("rr", td, ref["rr_t"])):
        err = rel_err(ctx.matvec_device(kind, vec, ETA).cpu().numpy(), want)
        path_ok(kind)
        print("n = %d periodic = %s %s: %.3e" % (n, periodic, kind, err))
        assert err <= TOL, (kind, err)
      err = rel_err(ctx.matvec_device("tt_tr", fd, ETA, vec2=td).cpu().numpy(), ref["tt_f"] + ref["tr_t"])
      path_ok("tt_tr")
      print("n = %d periodic = %s tt_tr: %.3e" % (n, periodic, err))
      assert err <= TOL
      u, w = ctx.matvec_op_device("grand", (fd, td), ETA)
      path_ok("grand")
      eu, ew = rel_err(u.cpu().numpy(), ref["tt_f"] + ref["tr_t"]), rel_err(w.cpu().numpy(), ref["rt_f"] + ref["rr_t"])
      print("n = %d periodic = %s grand: %.3e %.3e" % (n, periodic, eu, ew))
      assert eu <= TOL and ew <= TOL
      (u,) = ctx.matvec_op_device("velocity_from_force_torque", (fd, td), ETA)
      path_ok("velocity_from_force_torque")
      assert rel_err(u.cpu().numpy(), ref["tt_f"] + ref["tr_t"]) <= TOL
      u, w = ctx.matvec_op_device("force_column", (fd,), ETA)
      path_ok("force_column")
      eu, ew = rel_err(u.cpu().numpy(), ref["tt_f"]), rel_err(w.cpu().numpy(), ref["rt_f"])
      print("n = %d periodic = %s force_column: %.3e %.3e" % (n, periodic, eu, ew))
      assert eu <= TOL and ew <= TOL
      ua, ub = ctx.matvec_op_device("tr_multi", (td, fd), ETA)
      path_ok("tr_multi")
      assert rel_err(ua.cpu().numpy(), ref["tr_t"]) <= TOL and rel_err(ub.cpu().numpy(), ref["tr_f"]) <= TOL
      # the translation product of the boundary is untouched by the option
      assert rel_err(ctx.matvec_device("tt", fd, ETA).cpu().numpy(), ref["tt_f"]) <= TOL
    # the option set back: the refusals of a reference-faithful free-surface context
    ctx.set_option("free_surface_rotation", 0)
    for kind in ("tr", "rt", "rr"):
      with pytest.raises(RmbError, match="free surface"):
        ctx.matvec_device(kind, fd, ETA)
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec_op_device("grand", (fd, td), ETA)
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec_op_device("tr_multi", (fd, td), ETA)
  finally:
    ctx.close()


def test_deterministic_symmetric_grand_is_bitwise_reproducible(oracle):
  r, L, f, t, ref = _case(oracle, 130, False)
  ctx = _ctx(r)
  try:
    ctx.set_option("deterministic", 2)
    fd, td = _dev(f), _dev(t)
    u1, w1 = [x.clone() for x in ctx.matvec_op_device("grand", (fd, td), ETA)]
    u2, w2 = ctx.matvec_op_device("grand", (fd, td), ETA)
    assert torch.equal(u1, u2) and torch.equal(w1, w2)
    assert rel_err(u1.cpu().numpy(), ref["tt_f"] + ref["tr_t"]) <= TOL and rel_err(w1.cpu().numpy(), ref["rt_f"] + ref["rr_t"]) <= TOL
    # a single block through the same pass
    assert rel_err(ctx.matvec_device("rr", td, ETA).cpu().numpy(), ref["rr_t"]) <= TOL
  finally:
    ctx.close()


def test_deterministic_one_sided_sweep_above_the_symmetric_threshold(oracle):
  """`deterministic = 1` sends 257 blobs through the one-sided sweep: five source tiles, a second workgroup of targets
  holding one blob; fixed summation order, so bitwise reproducible."""
  r, L, f, t, ref = _case(oracle, 257, False)
  ctx = _ctx(r)
  try:
    ctx.set_option("deterministic", 1)
    fd, td = _dev(f), _dev(t)
    for kind, vec, vec2, want in (("tr", td, None, ref["tr_t"]), ("rt", fd, None, ref["rt_f"]), ("rr", td, None, ref["rr_t"]),
                                  ("tt_tr", fd, td, ref["tt_f"] + ref["tr_t"])):
      u1 = ctx.matvec_device(kind, vec, ETA, vec2=vec2).clone()
      assert ctx.last_launch()["chunks"] >= 1, "%s did not take the one-sided sweep" % kind
      assert torch.equal(u1, ctx.matvec_device(kind, vec, ETA, vec2=vec2))
      assert rel_err(u1.cpu().numpy(), want) <= TOL, kind
    u, w = ctx.matvec_op_device("grand", (fd, td), ETA)
    assert ctx.last_launch()["chunks"] >= 1
    assert rel_err(u.cpu().numpy(), ref["tt_f"] + ref["tr_t"]) <= TOL and rel_err(w.cpu().numpy(), ref["rt_f"] + ref["rr_t"]) <= TOL
  finally:
    ctx.close()


@pytest.mark.parametrize("n", [130, 100])
def test_pair_shards_sum_to_the_full_product(oracle, n):
  """What G = 3 ranks compute (pair shard g of G into a full-length partial) summed the way all_reduce will; a shard takes
  the symmetric kernel whatever n."""
  r, L, f, t, ref = _case(oracle, n, False)
  ctx = _ctx(r)
  try:
    fd, td = _dev(f), _dev(t)
    parts = [ctx.matvec_op_device("grand", (fd, td), ETA, shard=g, nshards=3) for g in range(3)]
    u = torch.stack([p[0] for p in parts]).sum(0).cpu().numpy()
    w = torch.stack([p[1] for p in parts]).sum(0).cpu().numpy()
    eu, ew = rel_err(u, ref["tt_f"] + ref["tr_t"]), rel_err(w, ref["rt_f"] + ref["rr_t"])
    print("n = %d grand shards: %.3e %.3e" % (n, eu, ew))
    assert eu <= TOL and ew <= TOL
    full = ctx.matvec_op_device("grand", (fd, td), ETA)
    assert rel_err(u, full[0].cpu().numpy()) <= TOL and rel_err(w, full[1].cpu().numpy()) <= TOL
    rr = sum(ctx.matvec_pairshard_device("rr", td, ETA, g, 3).cpu().numpy() for g in range(3))
    assert rel_err(rr, ref["rr_t"]) <= TOL
    assert rel_err(rr, ctx.matvec_device("rr", td, ETA).cpu().numpy()) <= TOL
  finally:
    ctx.close()


def test_variants_the_rotational_products_do_not_have_are_refused(oracle):
  from rigidmultiblobswall_amd._lib import RmbError
  r, L, f, t, ref = _case(oracle, 130, False)
  fd, td = _dev(f), _dev(t)
  ctx = _ctx(r, np.array([9.0, 9.0, 9.0]))      # images along z
  try:
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec_device("rr", td, ETA)
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec_op_device("grand", (fd, td), ETA)
    ctx.set_positions(_dev(r), A, None, wall="free_surface")
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec_device("tr", td, ETA, in_plane=True)
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec_op_device("velocity_from_force_torque", (fd, td), ETA, in_plane=True)
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec2_device("tt", fd, td, ETA)
    ctx.set_option("precision", 32)
    for call in (lambda: ctx.matvec_device("rt", fd, ETA), lambda: ctx.matvec_op_device("force_column", (fd,), ETA),
                 lambda: ctx.matvec_op_device("rr_multi", (fd, td), ETA)):
      with pytest.raises(RmbError, match="free surface"):
        call()
    ctx.set_option("precision", 64)
    assert rel_err(ctx.matvec_device("rt", fd, ETA).cpu().numpy(), ref["rt_f"]) <= TOL
  finally:
    ctx.close()


# ---- rollers ----------------------------------------------------------------------------------------------------------
def _rollers(n=130, seed=3):
  """n rollers, heights in [0.5 a, 6 a]."""
  rng = np.random.RandomState(seed)
  side = 2.2 * A * n ** (1.0 / 3.0)
  return np.column_stack([side * rng.rand(n), side * rng.rand(n), A * (0.5 + 5.5 * rng.rand(n))])


def _integrator(r0, scheme, device="cuda:0", ctx=None, rng=None, tolerance=1e-8):
  from rigidmultiblobswall_amd.rollers import RollersIntegrator
  integ = RollersIntegrator(r0, scheme, A, ETA, tolerance=tolerance, domain="free_surface", device=device, ctx=ctx, rng=rng,
                            seed=None if rng is not None else 1)
  integ.g, integ.repulsion_strength_wall, integ.debye_length_wall = 0.2, 0.05, 0.1 * A
  integ.repulsion_strength, integ.debye_length = 0.02, 0.1 * A
  integ.omega_one_roller = np.array([0.0, 5.0, 0.0])
  integ.report_rejections = False
  return integ


def test_free_kinematics_forward_euler_step(oracle):
  r0 = _rollers()
  integ = _integrator(r0, "deterministic_forward_euler")
  try:
    F = (integ.calc_one_blob_forces(integ.location) + integ.calc_blob_blob_forces(integ.location)).cpu().numpy().reshape(-1)
    T = integ.get_torque().cpu().numpy()
    dt = 0.01
    integ.advance_time_step(dt)
    want = r0.reshape(-1) + dt * fm.fused_row(oracle, r0, F, T, ETA, A)
    err = np.abs(integ.location.cpu().numpy().reshape(-1) - want).max() / np.abs(want).max()
    print("forward Euler step: %.3e" % err)
    assert err <= 1e-12
    assert integ.ctx.get_option("free_surface_rotation") == 1 and integ.ctx.get_option("free_surface") == 1
    assert integ.invalid_configuration_count == 0
  finally:
    integ.close()


def test_prescribed_kinematics_torque_against_a_dense_solve(oracle):
  """M_rr T = omega - M_rt F solved by GMRES to `tolerance` on the normalised right-hand side: the torque differs from
  the dense solve by at most kappa(M_rr) tolerance (relative)."""
  r0 = _rollers()
  tol = 1e-10
  integ = _integrator(r0, "deterministic_forward_euler", tolerance=tol)
  integ.free_kinematics = "False"
  try:
    F = (integ.calc_one_blob_forces(integ.location) + integ.calc_blob_blob_forces(integ.location)).cpu().numpy().reshape(-1)
    velocity, torque = integ.compute_deterministic_velocity_and_torque()
    Mrr = fm.dense_block(oracle, "rr", r0, ETA, A)
    omega = np.tile(integ.get_omega_one_roller(), len(r0))
    want_T = np.linalg.solve(Mrr, omega - fm.product(oracle, "rt", r0, F, ETA, A))
    kappa = np.linalg.cond(Mrr)
    err = rel_err(torque.cpu().numpy(), want_T)
    print("torque against the dense solve %.3e, kappa(M_rr) = %.3e, bound %.3e" % (err, kappa, kappa * tol))
    assert err <= kappa * tol
    want_v = fm.fused_row(oracle, r0, F, want_T, ETA, A)
    assert rel_err(velocity.cpu().numpy(), want_v) <= kappa * tol
    assert integ.det_iterations_count > 0
  finally:
    integ.close()


def test_a_roller_under_a_free_surface_runs_the_other_way():
  """A lone roller at h = 1.5 a driven by a torque along y: its image above a no-slip wall drags it forward (+x), the
  counter-rotating image of a stress-free surface pushes it back."""
  from rigidmultiblobswall_amd.rollers import RollersIntegrator
  ux = {}
  for domain in ("free_surface", "single_wall"):
    integ = RollersIntegrator(np.array([[0.0, 0.0, 1.5 * A]]), "deterministic_forward_euler", A, ETA, domain=domain, device="cuda:0", seed=1)
    integ.omega_one_roller = np.array([0.0, 5.0, 0.0])
    velocity, _ = integ.compute_deterministic_velocity_and_torque()
    ux[domain] = float(velocity[0])
    integ.close()
  print(ux)
  assert ux["single_wall"] > 0.0 > ux["free_surface"]


def test_native_lanczos_on_the_grand_mobility_equals_the_generic_loop(oracle):
  r0 = _rollers()
  nat, gen = _integrator(r0, "stochastic_first_order"), _integrator(r0, "stochastic_first_order")
  gen.native_lanczos = False
  rng = np.random.RandomState(11)
  n6 = 6 * len(r0)
  try:
    for tol, factor in ((1e-4, 1.0), (1e-9, 0.37)):
      z = _dev(rng.randn(n6))
      out = []
      for integ in (nat, gen):
        integ.kT, integ.tolerance = 0.5 * factor ** 2, tol      # sqrt(2 kT / dt) = factor at dt = 1
        integ._bind(integ.location)
        before = integ.stoch_iterations_count
        noise = integ._lanczos(integ.grand_mobility, n6, z, 1.0, product="grand")
        out.append((noise.cpu().numpy(), integ.stoch_iterations_count - before))
      print(tol, out[0][1], out[1][1], rel_err(out[0][0], out[1][0]))
      assert out[0][1] == out[1][1] >= 2
      assert rel_err(out[0][0], out[1][0]) <= tol
    assert nat.lanczos_native_loop_calls == 2 and gen.lanczos_native_loop_calls == 0
    # the defining identity |G^{1/2} z|^2 = z . G z, G the grand mobility of the mirror system
    z = rng.randn(n6)
    nat.kT, nat.tolerance = 0.5, 1e-10
    nat._bind(nat.location)
    noise = nat._lanczos(nat.grand_mobility, n6, _dev(z), 1.0, product="grand").cpu().numpy()
    u, w = fm.grand(oracle, r0, z[:n6 // 2], z[n6 // 2:], ETA, A)
    zGz = float(z @ np.concatenate([u, w]))
    print("|noise|^2 / z.G z - 1 = %.3e" % (noise @ noise / zGz - 1.0))
    assert abs(noise @ noise / zGz - 1.0) < 1e-8
    assert nat.lanczos_native_loop_calls == 3
  finally:
    nat.close(); gen.close()


@pytest.mark.parametrize("scheme", ["stochastic_adams_bashforth", "stochastic_mid_point"])
def test_stochastic_steps_on_the_gpu_equal_the_cpu_stand_in(oracle, scheme):
  """One step with the same seeded RandomState on the GPU context and on the mirror stand-in: the two Lanczos forcings
  each stop at `tolerance`, the steps agree to ten times that."""
  r0 = _rollers()
  tol, dt = 1e-6, 0.01
  disp = []
  for device, ctx in (("cuda:0", None), ("cpu", fm.MirrorContext(oracle))):
    integ = _integrator(r0, scheme, device=device, ctx=ctx, rng=np.random.RandomState(5), tolerance=tol)
    integ.kT = 1e-3
    try:
      integ.advance_time_step(dt)
      assert integ.invalid_configuration_count == 0
      assert integ.stoch_iterations_count > 0
      disp.append(integ.location.cpu().numpy() - r0)
    finally:
      integ.close()
  err = rel_err(disp[0], disp[1])
  print("%s: displacement of the GPU step against the stand-in %.3e" % (scheme, err))
  assert err <= 10 * tol
