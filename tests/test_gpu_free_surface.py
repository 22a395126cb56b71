"""Rigid multiblobs above a free (stress-free) surface on the GPU: dense blocks, the saddle-point operator, the native and
the generic solver loops, the g15 decks of tools/gen_golden_free_surface.py, this engine's own preconditioner blocks, and
the sign of the boundary's effect on a shell's mobility."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err
from _rigid_common import replay, reference_counters, write_case
from test_free_surface_host import free_surface_dense, dense_K, _golden, _utility_deck

pytestmark = pytest.mark.gpu

ETA = 1.1
SHELL12_A = 0.41642


def _cloud(n, a, seed):
  """n blobs above the surface, some below z = a (the image's overlapping branch), blobs 0 and 1 touching."""
  rng = np.random.RandomState(seed)
  side = 2.2 * a * n ** (1.0 / 3.0)
  r = np.column_stack([side * rng.rand(n), side * rng.rand(n), 0.05 * a + side * rng.rand(n)])
  r[0, 2] = 0.4 * a
  r[1] = r[0] + [2 * a, 0, 0]
  assert np.sum(r[:, 2] < a) >= 2
  return r


def _free_surface_ctx(r, a, L=None):
  from rigidmultiblobswall_amd import MobilityContext
  ctx = MobilityContext(0)
  ctx.set_positions(torch.as_tensor(np.ascontiguousarray(r).reshape(-1), device="cuda"), a, L, wall="free_surface")
  return ctx


def _shells(nb, seed=0):
  """nb twelve-blob shells of the g15 decks on a grid, centres near height 1: lowest blobs below z = a."""
  g = _golden("det_euler_shells")
  rng = np.random.RandomState(seed)
  m = int(np.ceil(np.sqrt(nb)))
  loc = np.array([[2.4 * (k % m) + 0.1 * rng.rand(), 2.4 * (k // m) + 0.1 * rng.rand(), 1.0 + 0.1 * (rng.rand() - 0.5)] for k in range(nb)])
  q = rng.randn(nb, 4)
  return g["vertex_shell"], loc, q / np.linalg.norm(q, axis=1)[:, None]


def _suspension(refs, loc, quat, a, **kw):
  from rigidmultiblobswall_amd.rigid import RigidSuspension
  return RigidSuspension(refs, loc, quat, a, ETA, boundary="free_surface", device=torch.device("cuda:0"), **kw)


# ---- dense blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bodies,n_b", [(1, 130), (2, 12)])
def test_dense_blocks_equal_the_product_of_unit_vectors_and_the_numpy_block(n_bodies, n_b):
  """Column k of body_mobility_dense_device on a free-surface context = matvec_device("tt") of e_k (130 blobs: the
  symmetric free-surface kernel, two full tiles + 2; 24 blobs: the one-sided sweep), symmetric to rounding, and the numpy
  block to 1e-13 (the bound of the kernels against the oracle); blobs below z = a and a touching pair included."""
  a = 0.3
  n = n_bodies * n_b
  r = _cloud(n, a, 5 + n)
  ctx = _free_surface_ctx(r, a)
  try:
    first = torch.arange(0, n, n_b, device="cuda", dtype=torch.int64)
    M = ctx.body_mobility_dense_device(first, n_b, ETA).cpu().numpy()
    assert M.shape == (n_bodies, 3 * n_b, 3 * n_b)
    e = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    for b in range(n_bodies):
      lo = 3 * b * n_b
      ref = free_surface_dense(r[b * n_b:(b + 1) * n_b], ETA, a)
      scale = np.abs(ref).max()
      print("body %d: |M - numpy| / |numpy| = %.3e, asymmetry %.3e" % (b, rel_err(M[b], ref), np.abs(M[b] - M[b].T).max() / scale))
      assert rel_err(M[b], ref) <= 1e-13
      assert np.abs(M[b] - M[b].T).max() <= 4e-16 * scale * 8        # a few ulp of the largest entry
      worst = 0.0
      for k in range(3 * n_b):
        e.zero_(); e[lo + k] = 1.0
        col = ctx.matvec_device("tt", e, ETA).cpu().numpy()[lo:lo + 3 * n_b]
        worst = max(worst, np.abs(col - M[b][:, k]).max() / scale)
      print("body %d: worst column against the product %.3e" % (b, worst))
      assert worst <= 1e-13
  finally:
    ctx.close()


# ---- the operator ---------------------------------------------------------------------------------------------------
def _operator_case(name):
  if name == "one_body_130":
    ref = _cloud(130, 0.3, 11) - np.array([1.0, 1.0, 0.0])
    return [ref], np.array([[0.0, 0.0, 0.0]]) + 0.0, np.array([[1.0, 0, 0, 0]]), 0.3
  if name == "3x42":
    shell = np.load(os.path.join(GOLDEN, "g9_rigid_det_euler_42blob_shells.npz"))["vertex_shell42"]
    d = np.linalg.norm(shell[:, None] - shell[None], axis=2)
    a = float(d[d > 0].min() / 2)
    rng = np.random.RandomState(2)
    q = rng.randn(3, 4)
    return [shell] * 3, np.array([[0.0, 0, 1.1], [2.5, 0.2, 1.2], [0.3, 2.6, 1.15]]), q / np.linalg.norm(q, axis=1)[:, None], a
  nb = {"8x12": 8, "16x12": 16}[name]
  shell, loc, quat = _shells(nb, seed=nb)
  return [shell] * nb, loc, quat, SHELL12_A


@pytest.mark.parametrize("name", ["one_body_130", "8x12", "3x42", "16x12"])
def test_rigid_operator_on_a_free_surface_context(name):
  """rigid_operator_device against matvec + K products assembled in torch and against the numpy block.  130 and 192 blobs
  take the symmetric sweep + the free-surface finishing launch, 96 and 126 the product + block launch."""
  refs, loc, quat, a = _operator_case(name)
  rs = _suspension(refs, loc, quat, a)
  try:
    assert rs.ctx_wall == "free_surface" and rs.wall is False and float(rs.r_dev.view(-1, 3)[:, 2].min()) < a
    g = rs.groups[0]
    n3 = 3 * rs.n_blobs
    x = torch.as_tensor(np.random.RandomState(4).randn(rs.size), device="cuda")
    out = rs.ctx.rigid_operator_device(g.K, x, ETA, torch.empty_like(x))
    lam, U = x[:n3].contiguous(), x[n3:].reshape(rs.n_bodies, 6, 1)
    top = rs.ctx.matvec_device("tt", lam, ETA) - torch.bmm(g.K, U).reshape(-1)
    bot = -torch.bmm(g.K.transpose(1, 2), lam.reshape(rs.n_bodies, -1, 1)).reshape(-1)
    want = torch.cat([top, bot]).cpu().numpy()
    M = free_surface_dense(rs.r_vectors, ETA, a)
    K = dense_K(rs.r_vectors, loc, g.n_b)
    xn = x.cpu().numpy()
    want_np = np.concatenate([M @ xn[:n3] - K @ xn[n3:], -K.T @ xn[:n3]])
    print("%s: against torch %.3e, against numpy %.3e" % (name, rel_err(out.cpu().numpy(), want), rel_err(out.cpu().numpy(), want_np)))
    assert rel_err(out.cpu().numpy(), want) <= 1e-13
    assert rel_err(out.cpu().numpy(), want_np) <= 1e-13
    assert rel_err(rs.apply_operator(x).cpu().numpy(), want_np) <= 1e-13
    # a second application: the accumulators were left zeroed
    assert rel_err(rs.ctx.rigid_operator_device(g.K, x, ETA, torch.empty_like(x)).cpu().numpy(), want) <= 1e-13
  finally:
    rs.close()


def test_operator_against_the_golden_of_the_reference():
  g = _golden("operator")
  nb = len(g["locations"])
  rs = _suspension([g["vertex"]] * nb, g["locations"], g["quaternions"], float(g["blob_radius"]))
  try:
    assert np.abs(rs.r_vectors - g["r_vectors"].reshape(-1, 3)).max() < 1e-13
    x = torch.as_tensor(g["vector"], device="cuda")
    n3 = 3 * rs.n_blobs
    err = rel_err(rs.apply_operator(x).cpu().numpy(), g["operator"])
    err_p = rel_err(rs.mobility_times_lambda(x[:n3]).cpu().numpy(), g["product"])
    print("operator %.3e product %.3e" % (err, err_p))
    assert err <= 1e-12 and err_p <= 1e-12
  finally:
    rs.close()


def test_pseudo_periodic_operator_through_the_generic_path(oracle):
  """L in x and y: no fused finishing launch there, the product + the block launch; against the oracle's free-surface product."""
  shell, loc, quat = _shells(16, seed=3)
  L = np.array([11.0, 10.5, 0.0])
  rs = _suspension([shell] * 16, loc, quat, SHELL12_A, periodic_length=L)
  try:
    n3 = 3 * rs.n_blobs
    x = torch.as_tensor(np.random.RandomState(6).randn(rs.size), device="cuda")
    xn = x.cpu().numpy()
    K = dense_K(rs.r_vectors, loc, 12)
    Mlam = oracle.free_surface_mobility_trans_times_force_oracle(rs.r_vectors, xn[:n3], ETA, SHELL12_A, periodic_length=L)
    want = np.concatenate([Mlam - K @ xn[n3:], -K.T @ xn[:n3]])
    err = rel_err(rs.apply_operator(x).cpu().numpy(), want)
    print("periodic operator %.3e" % err)
    assert err <= 1e-13
    open_rs = _suspension([shell] * 16, loc, quat, SHELL12_A)
    assert rel_err(open_rs.apply_operator(x).cpu().numpy(), want) > 1e-6        # the images are there
    open_rs.close()
  finally:
    rs.close()


# ---- native and generic loops ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [8, 16])
def test_native_gmres_loop_equals_the_python_loop_above_a_free_surface(nb):
  """rmb_rigid_gmres_device against the Python-loop GMRES (selected as tests/test_gpu_rigid.py does for the wall): same
  iteration count, solutions equal to solver tolerance; 8 shells (the g15 deck: product + block launch), 16 shells (192
  blobs: symmetric sweep + the free-surface finishing launch with the fused dots)."""
  if nb == 8:
    g = _golden("det_euler_shells")
    shell, loc, quat = g["vertex_shell"], g["locations_shell"], g["quaternions_shell"]
  else:
    shell, loc, quat = _shells(nb, seed=1)
  nat = _suspension([shell] * nb, loc, quat, SHELL12_A, block_boundary="no_wall")
  pyl = _suspension([shell] * nb, loc, quat, SHELL12_A, block_boundary="no_wall")
  pyl.native_gmres = False
  rng = np.random.RandomState(5)
  try:
    for kw in (dict(tol=1e-9, restart=60), dict(tol=1e-6, restart=5)):
      rhs = torch.as_tensor(rng.randn(nat.size), device="cuda:0")
      xn, inn = nat.solve(rhs, **kw)
      xp, ip = pyl.solve(rhs, **kw)
      assert inn.get("native_gmres") and "native_gmres" not in ip and ip.get("native_steps", 0) > 0
      print(nb, kw, inn["iterations"], ip["iterations"], rel_err(xn.cpu().numpy(), xp.cpu().numpy()))
      assert inn["iterations"] == ip["iterations"] and inn["converged"] and ip["converged"]
      assert rel_err(xn.cpu().numpy(), xp.cpu().numpy()) <= kw["tol"]
      true_res = float(torch.linalg.norm(pyl.apply_operator(xn) - rhs) / torch.linalg.norm(rhs))
      assert true_res < 5 * kw["tol"], (kw, true_res)
  finally:
    nat.close(); pyl.close()


@pytest.mark.parametrize("nb", [8, 16])
def test_native_lanczos_loop_equals_the_generic_one_above_a_free_surface(nb):
  """rmb_rigid_lanczos_device against stochastic_forcing on the generic path: same iteration count, same noise."""
  shell, loc, quat = _shells(nb, seed=2)
  nat = _suspension([shell] * nb, loc, quat, SHELL12_A, block_boundary="no_wall")
  gen = _suspension([shell] * nb, loc, quat, SHELL12_A, block_boundary="no_wall")
  gen.native_lanczos = False
  rng = np.random.RandomState(11)
  try:
    for tol, factor in ((1e-4, 1.0), (1e-9, 0.37)):
      z = torch.as_tensor(rng.randn(3 * nat.n_blobs), device="cuda:0")
      a_, ia = nat.stochastic_forcing(z, factor, tol=tol)
      b_, ib = gen.stochastic_forcing(z, factor, tol=tol)
      print(nb, tol, ia, ib, rel_err(a_.cpu().numpy(), b_.cpu().numpy()))
      assert ia == ib and ia >= 2
      assert rel_err(a_.cpu().numpy(), b_.cpu().numpy()) <= tol
    assert nat.lanczos_native_loop_calls == 2 and gen.lanczos_native_loop_calls == 0
    # the defining identity: with w = L^-1 noise = (P^T M P)^{1/2} z, |w|^2 = (P z) . M (P z), M the free-surface mobility
    z = torch.as_tensor(rng.randn(3 * nat.n_blobs), device="cuda:0")
    a_, _ = nat.stochastic_forcing(z, 1.0, tol=1e-10)
    w = nat._blockdiag(a_, "Linv")
    Pz = nat._blockdiag(z, "Linv", transpose=True).cpu().numpy()
    zMz = float(Pz @ (free_surface_dense(nat.r_vectors, ETA, SHELL12_A) @ Pz))
    assert abs(float(torch.dot(w, w)) / zMz - 1.0) < 1e-8
  finally:
    nat.close(); gen.close()


# ---- trajectories of the reference's driver -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["det_euler_shells", "det_ab_shells", "slip_trapz_shells", "det_euler_mixed"])
def test_g15_deck_replay_matches_the_reference_driver(tmp_path, name):
  g = _golden(name)
  integ, worst_x, worst_q = replay(g, tmp_path, "cuda:0", None)
  ref = reference_counters(g)
  print(name, worst_x, worst_q, integ.det_iterations_count, ref["deterministic_iterations_count"], integ.stoch_iterations_count,
        ref["stochastic_iterations_count"])
  assert integ.domain == "free_surface" and integ.susp.ctx_wall == "free_surface" and integ.susp.block_boundary == "no_wall"
  tol = 1e-7 if float(g["kT"]) == 0.0 else 1e-6
  assert worst_x < tol and worst_q < tol, (worst_x, worst_q)
  assert integ.invalid_configuration_count == ref["invalid_configuration_count"] == 0
  assert integ.det_iterations_count == ref["deterministic_iterations_count"]
  assert integ.stoch_iterations_count == ref["stochastic_iterations_count"]
  integ.close()


def test_command_line_writes_the_references_output_files(tmp_path):
  import subprocess
  import sys
  from conftest import ROOT
  from rigidmultiblobswall_amd import structures
  g = _golden("det_euler_shells")
  deck = write_case(g, str(tmp_path))
  res = subprocess.run([sys.executable, "-m", "rigidmultiblobswall_amd", "--input-file", deck], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  tl = g["trajectory_locations_shell"]
  n, loc, quat = structures.read_clones_file(os.path.join(str(tmp_path), "run.shell.%08d.clones" % (len(tl) - 1)))
  assert np.abs(loc - tl[-1]).max() < 1e-7 * np.abs(tl[-1] - tl[0]).max()
  info = open(os.path.join(str(tmp_path), "run.info")).read()
  assert "deterministic_iterations_count = %d" % reference_counters(g)["deterministic_iterations_count"] in info
  assert "num_blobs          96" in open(os.path.join(str(tmp_path), "run.bodies_info")).read()


# ---- this engine's own blocks ---------------------------------------------------------------------------------------
def test_free_surface_blocks_reach_the_same_velocities_in_no_more_iterations(tmp_path):
  """The 8-shell deck with `hip_free_surface` blocks against `python_no_wall` blocks, one deterministic step, solver
  tolerance 1e-10 (the deck's): the same velocities to 100 tol, in no more GMRES iterations.  Two right-preconditioned
  solves that stop at a relative residual <= tol differ by at most 2 kappa(A) tol (kappa(A) of the saddle-point matrix,
  printed here, is a few hundred at this configuration); 100 tol is well inside that and far below what a wrong block
  would leave."""
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rigid_integrator
  g = _golden("det_euler_shells")
  res = {}
  for blocks in ("python_no_wall", "hip_free_surface"):
    d = tmp_path / blocks
    d.mkdir()
    gg = dict(g, deck=str(g["deck"]).replace("python_no_wall", blocks))
    read = ReadInput(write_case(gg, str(d)))
    integ = rigid_integrator.integrator_from_input(read, device="cuda:0")
    assert integ.susp.block_boundary == ("no_wall" if blocks == "python_no_wall" else "free_surface")
    x0 = integ.location.cpu().numpy().copy()
    r0 = integ.susp.r_vectors.copy()
    integ.advance_time_step(read.dt, step=0)
    res[blocks] = ((integ.location.cpu().numpy() - x0) / read.dt, integ.det_iterations_count)
    integ.close()
  a, eta, tol = float(g["blob_radius"]), 1.1, 1e-10
  M, K = free_surface_dense(r0, eta, a), dense_K(r0, g["locations_shell"], 12)
  A = np.block([[M, -K], [-K.T, np.zeros((K.shape[1], K.shape[1]))]])
  kappa = np.linalg.cond(A)
  diff = rel_err(res["hip_free_surface"][0], res["python_no_wall"][0])
  print("velocities differ by %.3e (2 kappa tol = %.3e), iterations %d (own blocks) vs %d" %
        (diff, 2 * kappa * tol, res["hip_free_surface"][1], res["python_no_wall"][1]))
  assert diff <= 100 * tol
  assert res["hip_free_surface"][1] <= res["python_no_wall"][1]


# ---- physics --------------------------------------------------------------------------------------------------------
def test_a_free_surface_speeds_up_parallel_motion_and_slows_down_normal_motion():
  """Body mobility of one 12-blob shell at centre height 2 R_h: the image of a stress-free surface is a co-moving sphere
  for motion along the surface and a counter-moving one for motion towards it; a no-slip wall slows both."""
  from rigidmultiblobswall_amd.rigid import RigidSuspension
  shell = _golden("det_euler_shells")["vertex_shell"]
  mu = {}
  for boundary in ("free_surface", "no_wall", "single_wall"):
    rs = RigidSuspension([shell], np.array([[0.0, 0.0, 2.0]]), np.array([[1.0, 0, 0, 0]]), SHELL12_A, ETA, boundary=boundary,
                         device=torch.device("cuda:0"))
    M, K = rs.dense_blob_mobility(), rs.dense_K()
    N = torch.linalg.inv(K.t() @ torch.linalg.solve(M, K)).cpu().numpy()
    mu[boundary] = (0.5 * (N[0, 0] + N[1, 1]), N[2, 2])
    rs.close()
  print(mu)
  assert mu["free_surface"][0] > mu["no_wall"][0] > mu["single_wall"][0]
  assert mu["free_surface"][1] < mu["no_wall"][1]


# ---- one-shot utilities ---------------------------------------------------------------------------------------------
def test_utilities_follow_the_decks_boundary(oracle, tmp_path):
  """`body_mobility` (dense free-surface blocks of the whole suspension) and `mobility` with the velocity field on a grid
  (the free-surface source -> target product) on the 8-shell deck."""
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import utilities
  g = _golden("det_euler_shells")
  a = float(g["blob_radius"])
  d = tmp_path / "bm"; d.mkdir()
  out = utilities.run(ReadInput(_utility_deck(g, d, "body_mobility", blocks="hip_free_surface")), device="cuda:0")
  M, K = free_surface_dense(out["r_vectors"], 1.1, a), dense_K(out["r_vectors"], g["locations_shell"], 12)
  N = np.linalg.inv(K.T @ np.linalg.solve(M, K))
  assert rel_err(out["body_mobility"], N) <= 1e-10
  assert rel_err(np.loadtxt(str(d / "run.body_mobility.dat")), N) <= 1e-10
  d = tmp_path / "mob"; d.mkdir()
  extra = "plot_velocity_field -1 8 6 -1 8 5 0.1 3 4\ntracer_radius 0\n"
  out = utilities.run(ReadInput(_utility_deck(g, d, "mobility", extra=extra)), device="cuda:0")
  lam, U = out["lambda_blobs"].reshape(-1), out["velocity"].reshape(-1)
  assert np.linalg.norm(M @ lam - K @ U) <= 1e-8 * np.linalg.norm(K @ U)
  coor = out["grid_coor"]
  ref = oracle.free_surface_mobility_trans_times_force_source_target_oracle(out["r_vectors"], coor, lam, np.full(96, a), np.zeros(len(coor)), 1.1)
  assert coor.shape == (120, 3) and rel_err(out["grid_velocity"], ref) <= 1e-12
  assert os.path.exists(str(d / "run.velocity_field.vtk"))


# ---- what a free-surface context refuses ----------------------------------------------------------------------------
def test_products_without_a_free_surface_form_are_refused():
  from rigidmultiblobswall_amd import MobilityContext
  from rigidmultiblobswall_amd._lib import RmbError
  a = 0.3
  r = _cloud(150, a, 9)
  ctx = _free_surface_ctx(r, a)
  raw = MobilityContext(0)
  raw.set_positions(torch.as_tensor(r.reshape(-1), device="cuda"), a, wall=False)
  try:
    v = [torch.as_tensor(np.random.RandomState(k).randn(450), device="cuda") for k in range(3)]
    # the product on a wall = 0 context, as before; the same kernel on both contexts (1e-13: atomic flushes in any order)
    want = raw.matvec_device("tt_free", v[0], ETA)
    assert rel_err(ctx.matvec_device("tt", v[0], ETA).cpu().numpy(), want.cpu().numpy()) <= 1e-13
    assert rel_err(ctx.matvec_device("tt_free", v[0], ETA).cpu().numpy(), want.cpu().numpy()) <= 1e-13
    for kind in ("tr", "rt", "rr"):
      with pytest.raises(RmbError, match="free surface"):
        ctx.matvec_device(kind, v[0], ETA)
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec_device("tt_tr", v[0], ETA, vec2=v[1])
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec_device("tt", v[0], ETA, in_plane=True)
    for op, k in (("grand", 2), ("velocity_from_force_torque", 2), ("force_column", 1), ("tr_multi", 2)):
      with pytest.raises(RmbError, match="free surface"):
        ctx.matvec_op_device(op, v[:k], ETA)
    with pytest.raises(RmbError, match="free surface"):
      ctx.matvec2_device("tt", v[0], v[1], ETA)
    # tt_multi: one free-surface sweep per vector
    outs = ctx.matvec_op_device("tt_multi", v, ETA)
    for vi, ui in zip(v, outs):
      assert rel_err(ui.cpu().numpy(), raw.matvec_device("tt_free", vi, ETA).cpu().numpy()) <= 1e-13
    # the boundary follows set_positions: the same context with a wall again, then unbounded
    ctx.set_positions(torch.as_tensor(r.reshape(-1), device="cuda"), a, wall=True)
    assert ctx.get_option("free_surface") == 0
    ctx.matvec_device("rr", v[0], ETA)
  finally:
    ctx.close(); raw.close()
