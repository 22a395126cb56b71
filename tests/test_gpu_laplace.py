"""Phoretic bodies on the GPU: the Laplace layer operators against the reference's values (g12), the fused sweeps, the
phoretic slip against the reference's calc_slip (g12_laplace_slip_*), and replays of the reference driver on phoretic
decks (g13_phoretic_*)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_files, load_golden, rel_err
from _rigid_common import reference_counters, write_case
import _laplace_numpy as lapnp

pytestmark = pytest.mark.gpu

_OPS = [("single_layer", "Laplace_single_layer_operator_hip", False, False),
        ("double_layer", "Laplace_double_layer_operator_hip", True, False),
        ("deriv_double_layer", "Laplace_deriv_double_layer_operator_hip", True, False),
        ("dipole", "Laplace_dipole_operator_hip", False, False),
        ("single_layer_st", "Laplace_single_layer_operator_source_target_hip", False, True),
        ("double_layer_st", "Laplace_double_layer_operator_source_target_hip", True, True)]


def _call(fn_name, g, normals, st, wall):
  from rigidmultiblobswall_amd import laplace
  fn = getattr(laplace, fn_name)
  if st:
    args = (g["r"], g["target"], g["field"], g["weights"]) + ((g["normals"],) if normals else ())
  else:
    args = (g["r"], g["field"], g["weights"]) + ((g["normals"],) if normals else ())
  return fn(*args, wall=wall)


@pytest.mark.parametrize("wall", [0, 1])
@pytest.mark.parametrize("name,fn,normals,st", _OPS, ids=[o[0] for o in _OPS])
def test_operators_match_reference(name, fn, normals, st, wall):
  g = load_golden(os.path.join(GOLDEN, "g12_laplace_operators.npz"))
  out = _call(fn, g, normals, st, wall)
  assert rel_err(out, g["%s_wall%d" % (name, wall)]) <= 1e-12


def _cloud(n, seed):
  rng = np.random.RandomState(seed)
  L = (n / 0.05) ** (1.0 / 3.0)
  r = np.column_stack([L * rng.rand(n), L * rng.rand(n), 0.5 + 0.3 * L * rng.rand(n)])
  nrm = rng.randn(n, 3)
  nrm /= np.linalg.norm(nrm, axis=1)[:, None]
  return r, nrm, rng.randn(n), 0.2 + rng.rand(n), rng.randn(n)


@pytest.mark.parametrize("wall", [0, 1])
def test_large_cloud_against_numpy_on_sampled_targets(wall):
  from rigidmultiblobswall_amd import laplace
  n = 20011
  r, nrm, f, w, _ = _cloud(n, 5)
  rows = np.random.RandomState(6).choice(n, 96, replace=False)
  rows = np.concatenate([rows, [0, 63, 64, 511, 512, n - 1]])
  for kind, fn, normals in (("S", "Laplace_single_layer_operator_hip", False), ("D", "Laplace_double_layer_operator_hip", True),
                            ("G", "Laplace_deriv_double_layer_operator_hip", True), ("P", "Laplace_dipole_operator_hip", False)):
    out = getattr(laplace, fn)(r, f, w, *((nrm,) if normals else ()), wall=wall)
    out = out.reshape(n, 3) if kind in ("G", "P") else out
    ref = lapnp.apply(kind, r, f, w, nrm if normals else None, wall=wall, targets_idx=rows)
    assert rel_err(out[rows], ref) <= 1e-12, kind
  tgt = r[rows[:40]] + 0.01
  tgt[3] = r[7]
  out = laplace.Laplace_double_layer_operator_source_target_hip(r, tgt, f, w, nrm, wall=wall)
  assert rel_err(out, lapnp.apply("D", r, f, w, nrm, wall=wall, tgt=tgt)) <= 1e-12


def _dev(*arrays):
  return [torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.float64, device="cuda:0") for a in arrays]


def test_fused_sweeps_equal_their_compositions_and_repeat_bitwise():
  from rigidmultiblobswall_amd.context import MobilityContext
  ctx = MobilityContext(0)
  n = 9000
  for wall in (False, True):
    r, nrm, p, w, q = _dev(*_cloud(n, 11 + wall))
    op = ctx.laplace_operator_device(r, w, p=p, q=q, normals=nrm, alpha=0.5, wall=wall)
    op2 = ctx.laplace_operator_device(r, w, p=p, q=q, normals=nrm, alpha=0.5, wall=wall)
    assert torch.equal(op, op2)                                         # bit-reproducible
    D = ctx.laplace_operator_device(r, w, p=p, normals=nrm, wall=wall)   # -D[p]
    S = ctx.laplace_operator_device(r, w, q=q, wall=wall)                # S[q]
    assert rel_err((op).cpu().numpy(), (0.5 * p + D + S).cpu().numpy()) <= 1e-13
    gr = ctx.laplace_gradient_device(r, w, p=p, q=q, normals=nrm, wall=wall)
    assert torch.equal(gr, ctx.laplace_gradient_device(r, w, p=p, q=q, normals=nrm, wall=wall))
    G = ctx.laplace_gradient_device(r, w, p=p, normals=nrm, wall=wall)  # 2 G[p]
    P = ctx.laplace_gradient_device(r, w, q=q, wall=wall)               # -2 P[q]
    assert rel_err(gr.cpu().numpy(), (G + P).cpu().numpy()) <= 1e-13
    # against the reference-shaped host operators
    rn, nn, pn, wn, qn = [t.cpu().numpy() for t in (r, nrm, p, w, q)]
    from rigidmultiblobswall_amd import laplace
    ref = 0.5 * pn - laplace.Laplace_double_layer_operator_hip(rn, pn, wn, nn, wall=wall) + \
        laplace.Laplace_single_layer_operator_hip(rn, qn, wn, wall=wall)
    assert rel_err(op.cpu().numpy(), ref) <= 1e-13
    a = laplace.Laplace_dipole_operator_hip(rn, qn, wn, wall=wall)
    assert np.array_equal(a, laplace.Laplace_dipole_operator_hip(rn, qn, wn, wall=wall))
  ctx.close()


def _suspension_from_slip_fixture(g):
  from rigidmultiblobswall_amd.rigid import RigidSuspension
  nb = len(g["locations"])
  susp = RigidSuspension([g["vertex"]] * nb, g["locations"], g["quaternions"], float(g["blob_radius"]), 1.0,
                         wall=str(g["domain"]) == "single_wall", device="cuda:0")
  return susp


@pytest.mark.parametrize("path", golden_files("g12_laplace_slip_*.npz"),
                         ids=[os.path.basename(p)[17:-4] for p in golden_files("g12_laplace_slip_*.npz")])
def test_phoretic_slip_matches_reference_calc_slip(path):
  from rigidmultiblobswall_amd.laplace import PhoreticSlip
  g = load_golden(path)
  susp = _suspension_from_slip_fixture(g)
  nb = len(g["locations"])
  ps = PhoreticSlip(susp, np.tile(g["laplace"], (nb, 1)), background=g["background"],
                    diffusion_coefficient=float(g["diffusion_coefficient"]), tolerance=float(g["tolerance"]),
                    wall=str(g["domain"]) == "single_wall")
  slip = ps.compute(susp).cpu().numpy()
  assert rel_err(ps.concentration.cpu().numpy(), g["concentration"]) <= 1e-10
  assert rel_err(slip, g["slip"]) <= 1e-10
  assert abs(ps.last_iterations - int(g["iterations"])) <= 1
  # same configuration: the result is reused, no second solve
  assert ps.compute(susp) is ps.compute(susp) and ps.solves == 1
  susp.close()


def _replay(g, tmp_path):
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rigid_integrator, structures
  deck = write_case(g, str(tmp_path))
  for ID in [str(x) for x in g["IDs"]]:
    np.savetxt(os.path.join(str(tmp_path), ID + ".Laplace"), g["laplace_" + ID], fmt="%.17g")
  read = ReadInput(deck)
  integ = rigid_integrator.integrator_from_input(read, device="cuda:0")
  rigid_integrator.run(read, integ)
  worst_x = worst_q = 0.0
  for ID in [str(x) for x in g["IDs"]]:
    tl, tq = g["trajectory_locations_" + ID], g["trajectory_quaternions_" + ID]
    scale = max(np.abs(tl[-1] - tl[0]).max(), 1e-300)
    for step in range(len(tl)):
      n, loc, quat = structures.read_clones_file(os.path.join(str(tmp_path), "run.%s.%08d.clones" % (ID, step)))
      worst_x = max(worst_x, np.abs(loc - tl[step]).max() / scale)
      worst_q = max(worst_q, np.abs(quat - tq[step]).max())
  return integ, worst_x, worst_q


G13 = golden_files("g13_phoretic_*.npz")


@pytest.mark.parametrize("path", G13, ids=[os.path.basename(p)[13:-4] for p in G13])
def test_phoretic_deck_replay_matches_reference_driver(tmp_path, path):
  g = load_golden(path)
  integ, worst_x, worst_q = _replay(g, tmp_path)
  tol = 1e-7 if float(g["kT"]) == 0.0 else 1e-6
  assert worst_x < tol and worst_q < tol, (worst_x, worst_q)
  ref = reference_counters(g)
  assert integ.invalid_configuration_count == ref["invalid_configuration_count"] == 0
  assert abs(integ.det_iterations_count - ref["deterministic_iterations_count"]) <= 2
  assert integ.stoch_iterations_count == ref["stochastic_iterations_count"]
  assert integ.calc_slip.solves >= int(g["n_steps"]) and integ.calc_slip.iterations > 0
  integ.close()


def test_janus_step_solves_to_tolerance_and_slip_is_tangential():
  from rigidmultiblobswall_amd.rigid_integrator import RigidIntegrator
  from rigidmultiblobswall_amd.laplace import PhoreticSlip
  g = load_golden(os.path.join(GOLDEN, "g12_laplace_slip_janus_wall.npz"))
  shell, lap = g["vertex"], g["laplace"]
  m = 16
  nb = m * m
  rng = np.random.RandomState(3)
  loc = np.array([[3.0 * (k % m), 3.0 * (k // m), 1.5 + 0.5 * rng.rand()] for k in range(nb)])
  q = rng.randn(nb, 4)
  q /= np.linalg.norm(q, axis=1)[:, None]
  a = float(g["blob_radius"])
  integ = RigidIntegrator([shell] * nb, loc, q, "deterministic_forward_euler", a, 1.0, tolerance=1e-8, device="cuda:0")
  ps = PhoreticSlip(integ.susp, np.tile(lap, (nb, 1)), background=g["background"], diffusion_coefficient=0.7,
                    tolerance=1e-8)
  integ.calc_slip = ps
  integ.advance_time_step(0.01, step=0)
  assert ps.solves == 1 and ps.last_residual <= 1e-8
  # true residual of the concentration solve at the configuration it was solved at (the start of the step)
  integ._move(torch.as_tensor(loc, device="cuda:0"), torch.as_tensor(q, device="cuda:0"))
  slip = ps.compute(integ.susp)
  c = ps.concentration
  ctx = ps._ctx
  from rigidmultiblobswall_amd.rigid_integrator import lab_frame_slip
  n = lab_frame_slip(integ.susp, ps.normals_body)
  r = integ.susp.r_dev
  Ac = ctx.laplace_operator_device(r, ps.weights, p=c, q=ps.k * c, normals=n, alpha=0.5, wall=True)
  rv = r.view(-1, 3)
  rhs = ps.c0 + rv @ ps.grad0 + (rv * (rv @ ps.H)).sum(1) + ctx.laplace_operator_device(r, ps.weights, q=ps.e, wall=True)
  assert float(torch.linalg.norm(Ac - rhs) / torch.linalg.norm(rhs)) <= 1e-8
  nn = n.view(-1, 3)
  normal_part = (nn * slip).sum(1)
  assert float(normal_part.norm()) <= 1e-12 * float(slip.norm())
  assert float(slip.norm()) > 0
  integ.close()
