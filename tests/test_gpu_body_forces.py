"""Body-body forces on the GPU: the Yukawa sweep over body centres (rmb_body_body_force, the BodyYukawaLaw instance of
sym_force_kernel) against the reference's recorded forces and the numpy restatement, its entry points, and the time
steppers that add it (tests/golden/g16_*, tools/gen_golden_body_forces.py)."""
import os

import numpy as np
import pytest
import torch

import _body_forces_numpy as bfn
from conftest import ROOT, golden_files, load_golden, rel_err
from _rigid_common import replay, reference_counters, write_case
from _rollers_common import run_and_compare

pytestmark = pytest.mark.gpu

TOL_D2 = 1e-12      # the bound of the blob-force-versus-oracle parity tests (test_gpu_parity.py), measured the same way: rel_err


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


@pytest.fixture(scope="module")
def golden():
  return load_golden(golden_files("g16_body_forces.npz")[0])


def _sweep(ctx, x, L, eps, b):
  ctx.set_positions(x, 1.0, L, wall=False)
  return ctx.body_body_force(eps, b)


# ---- the kernel ----------------------------------------------------------------------------------------------------------
def test_kernel_matches_the_reference_forces(ctx, golden):
  """Every case of g16_body_forces.npz to 1e-12 max|F|, the kernel-versus-golden bound of the project."""
  eps, b = float(golden["repulsion_strength"]), float(golden["debye_length"])
  for name in [str(n) for n in golden["names"]]:
    ref = golden["FT_" + name][0::2]
    F = _sweep(ctx, golden["x_" + name], golden["L_" + name], eps, b)
    err = np.abs(F - ref).max() / np.abs(ref).max()
    print("%-10s %.2e max|F|" % (name, err))
    assert F.shape == ref.shape and err <= 1e-12, (name, err)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_kernel_matches_the_restatement_at_the_tile_edges(ctx, n):
  """One centre (zeros), a pair, one tile short of / exactly / one past full (64: the peeled step 32 of a diagonal unit),
  three tiles.  Bound: rel_err < 1e-12, as the blob forces against the oracle; the restatement in double sits 1.9e-16 ..
  1.7e-15 max|F| from itself in long double on the fixture clouds (test_body_forces_host.py prints it): 4 x that is far
  inside the bound, so the Yukawa law needs no more."""
  x, _ = bfn.lattice_cloud(n, 1610 + n)
  eps, b = 1.3, 0.8
  F = _sweep(ctx, x, np.zeros(3), eps, b)
  if n == 1:
    assert F.shape == (1, 3) and not np.any(F)
    return
  err = rel_err(F, bfn.forces(x, None, eps, b).astype(np.float64))
  print("n = %d  rel_err %.2e" % (n, err))
  assert np.all(np.isfinite(F)) and err < TOL_D2, err


def test_kernel_on_700_periodic_centres_in_any_order(ctx):
  """700 centres (11 tiles), periodic in all three directions; the same cloud listed in another order gives the same forces
  on the same centres."""
  n = 700
  x, box = bfn.lattice_cloud(n, 1620)
  L = np.array([box, box, box])
  eps, b = 1.3, 0.8
  ref = bfn.forces(x, L, eps, b).astype(np.float64)
  F = _sweep(ctx, x, L, eps, b)
  perm = np.random.RandomState(3).permutation(n)
  Fp = _sweep(ctx, x[perm], L, eps, b)
  print("rel_err %.2e, shuffled %.2e" % (rel_err(F, ref), rel_err(Fp, ref[perm])))
  assert rel_err(F, ref) < TOL_D2 and rel_err(Fp, ref[perm]) < TOL_D2
  assert np.abs(F.sum(axis=0)).max() < 1e-10 * np.abs(F).sum()     # pairwise antisymmetric


@pytest.mark.parametrize("n", [200, 1984, 1985])
def test_culled_units_change_nothing(ctx, n):
  """Two clusters 1000 b apart, listed one after the other: every tile pair across the gap is beyond 750 b and is culled;
  the result equals the restatement, which evaluates every pair.  1984 centres = 31 tiles, the last size that keeps the
  caller's order; 1985 = 32 tiles, the first that takes the Morton-sorted copy."""
  b, eps = 0.01, 0.4
  x, box = bfn.lattice_cloud(n, 1630, spacing=0.05, jitter=0.005, dims=2)
  x[n // 2:, 0] += box + 1000.0 * b
  assert x[n // 2:, 0].min() - x[:n // 2, 0].max() > 750.0 * b
  F = _sweep(ctx, x, np.zeros(3), eps, b)
  assert ctx.last_launch()["tiles"] == (n + 63) // 64
  err = rel_err(F, bfn.forces(x, None, eps, b).astype(np.float64))
  print("n = %d  rel_err %.2e" % (n, err))
  assert err < TOL_D2, err


def test_coincident_centres_spoil_only_themselves(ctx):
  """r = 0 divides by zero in the reference; here the two coincident centres get non-finite forces and every other
  centre the force the restatement gives it (the pair's own term is the only non-finite one)."""
  x, _ = bfn.lattice_cloud(130, 1640)
  x[77] = x[5]
  eps, b = 1.3, 0.8
  F = _sweep(ctx, x, np.zeros(3), eps, b)
  others = np.setdiff1d(np.arange(130), [5, 77])
  ref = bfn.forces(x, None, eps, b).astype(np.float64)
  assert not np.any(np.isfinite(F[[5, 77]]).all(axis=1))
  assert np.all(np.isfinite(F[others])) and rel_err(F[others], ref[others]) < TOL_D2


def test_force_is_minus_the_gradient_of_the_yukawa_energy(ctx):
  """Central difference of the existing Yukawa pair energy (rmb_blob_potential, form "yukawa") along random directions
  against -F . delta, as test_pair_energy_is_the_potential_of_the_blob_blob_forces, with its bound 1e-7 |F|.  The host
  test test_restated_force_is_minus_the_gradient_of_the_yukawa_energy checks that the reference law itself stays inside
  that bound for this cloud and step (it misses by 1e-12 .. 1e-11 |F| there, in long double and in double)."""
  x, L, eps, b, h = bfn.gradient_cloud()
  F = _sweep(ctx, x, L, eps, b)
  rng = np.random.RandomState(bfn.GRADIENT["seed"])
  for _ in range(bfn.GRADIENT["directions"]):
    delta = rng.randn(*x.shape)
    delta /= np.linalg.norm(delta)
    ctx.set_positions(x + h * delta, 1.0, L, wall=False)
    up = ctx.blob_potential(eps, b, 1.0, potential="yukawa")[1]
    ctx.set_positions(x - h * delta, 1.0, L, wall=False)
    um = ctx.blob_potential(eps, b, 1.0, potential="yukawa")[1]
    fd = (up - um) / (2 * h)
    print("dU/dh %.12e  -F.delta %.12e  |F| %.6e" % (fd, -np.sum(F * delta), np.linalg.norm(F)))
    assert abs(fd + np.sum(F * delta)) <= 1e-7 * np.linalg.norm(F)


# ---- entry points ----------------------------------------------------------------------------------------------------------
def test_device_entry_writes_the_callers_tensor(ctx, golden):
  """The _device entry with out= fills the caller's tensor with what the host entry returns.  Bit for bit on the
  two-centre cases, where every sum has one term; with more centres a force is the sum of several waves' atomic
  flushes, whose order is not fixed from one launch to the next, and the two entries agree to rounding."""
  eps, b = float(golden["repulsion_strength"]), float(golden["debye_length"])
  for name in [str(n) for n in golden["names"]]:
    x, L = golden["x_" + name], golden["L_" + name]
    host = _sweep(ctx, x, L, eps, b)
    out = torch.full((3 * len(x),), -1.0, dtype=torch.float64, device="cuda:0")
    res = ctx.body_body_force_device(eps, b, out=out)
    assert res.data_ptr() == out.data_ptr()
    dev = out.cpu().numpy().reshape(-1, 3)
    if len(x) == 2:
      assert np.array_equal(dev, host)
    assert np.abs(dev - host).max() <= 1e-14 * np.abs(host).max()
    fresh = ctx.body_body_force_device(eps, b).cpu().numpy().reshape(-1, 3)
    assert np.abs(fresh - host).max() <= 1e-14 * np.abs(host).max()
  with pytest.raises(ValueError):
    ctx.body_body_force_device(eps, b, out=torch.empty(5, dtype=torch.float64, device="cuda:0"))


def test_argument_and_state_checks(ctx):
  x, _ = bfn.lattice_cloud(10, 1650)
  ctx.set_positions(x, 1.0, np.zeros(3), wall=False)
  for bad in (0.0, -1.0, float("nan")):
    with pytest.raises(Exception, match="debye_length"):
      ctx.body_body_force(1.0, bad)
  ctx.set_positions(x, 1.0, np.zeros(3), wall=True)
  with pytest.raises(Exception, match="wall = 0"):
    ctx.body_body_force(1.0, 1.0)
  ctx.set_positions(x, 1.0, np.zeros(3), wall=False)
  ctx.set_target_range(2, 7)
  with pytest.raises(Exception, match="target range"):
    ctx.body_body_force(1.0, 1.0)
  ctx.set_target_range(0, 10)
  assert np.all(np.isfinite(ctx.body_body_force(1.0, 1.0)))


def test_reference_call_shape(golden):
  """calc_body_body_forces_torques_hip(bodies, r_vectors, **kwargs): centres from b.location, (2 N_b, 3) with zero torque
  rows, equal to the reference's array."""
  import types
  from rigidmultiblobswall_amd import dispatch
  f = dispatch.set_body_body_forces_torques("python")
  eps, b = float(golden["repulsion_strength"]), float(golden["debye_length"])
  for name in ("n65_xy", "n200_xyz", "n2_open"):
    x, L, ref = golden["x_" + name], golden["L_" + name], golden["FT_" + name]
    bodies = [types.SimpleNamespace(location=np.copy(xi), orientation=None) for xi in x]
    FT = f(bodies, np.zeros((7, 3)), periodic_length=L, repulsion_strength=eps, debye_length=b)
    assert FT.shape == ref.shape and not np.any(FT[1::2])
    assert np.abs(FT - ref).max() <= 1e-12 * np.abs(ref).max()
  assert f([], np.zeros((0, 3)), repulsion_strength=eps, debye_length=b).shape == (0, 3)


# ---- time steppers ---------------------------------------------------------------------------------------------------------
RIGID = golden_files("g16_rigid_*.npz")
ROLLERS = golden_files("g16_rollers_*.npz")


def test_fixture_lists():
  assert len(RIGID) == 3 and len(ROLLERS) == 2


@pytest.mark.parametrize("path", RIGID, ids=[os.path.basename(p)[4:-4] for p in RIGID])
def test_rigid_deck_replay_matches_reference_driver(tmp_path, path):
  """The decks the reference's driver ran with `body_body_force_torque_implementation python`, through
  integrator_from_input; tolerances of the g9 replays."""
  g = load_golden(path)
  assert "body_body_force_torque_implementation    python" in str(g["deck"])
  integ, worst_x, worst_q = replay(g, tmp_path, "cuda:0", None)
  assert integ.body_body_force == (2.0, 0.8)
  tol = 1e-7 if float(g["kT"]) == 0.0 else 1e-6
  print("worst location %.2e, quaternion %.2e" % (worst_x, worst_q))
  assert worst_x < tol and worst_q < tol, (worst_x, worst_q)
  ref = reference_counters(g)
  assert integ.invalid_configuration_count == ref["invalid_configuration_count"] == 0
  assert integ.stoch_iterations_count == ref["stochastic_iterations_count"]
  integ.close()


def _roller_deck(g, tmp_path):
  L = np.asarray(g["periodic_length"], dtype=np.float64)
  (tmp_path / "blob.vertex").write_text("1\n0 0 0\n")
  with open(tmp_path / "rollers.clones", "w") as fh:
    fh.write("%d\n" % len(g["trajectory"][0]))
    for x in g["trajectory"][0]:
      fh.write("%.17g %.17g %.17g 1.0 0.0 0.0 0.0\n" % tuple(x))
  lines = [("scheme", str(g["scheme"])), ("mobility_vector_prod_implementation", "pycuda"), ("blob_blob_force_implementation", "numba"),
           ("body_body_force_torque_implementation", "python"), ("domain", str(g["domain"])),
           ("repulsion_strength", "%.17g" % float(g["repulsion_strength"])), ("debye_length", "%.17g" % float(g["debye_length"])),
           ("repulsion_strength_wall", "%.17g" % float(g["repulsion_strength_wall"])),
           ("debye_length_wall", "%.17g" % float(g["debye_length_wall"])), ("dt", "%.17g" % float(g["dt"])),
           ("n_steps", "%d" % int(g["n_steps"])), ("n_save", "1"), ("solver_tolerance", "%.17g" % float(g["tolerance"])),
           ("eta", "%.17g" % float(g["eta"])), ("g", "%.17g" % float(g["g"])), ("blob_radius", "%.17g" % float(g["a"])),
           ("kT", "%.17g" % float(g["kT"])), ("omega_one_roller", "%.17g %.17g %.17g" % tuple(g["omega_one_roller"])),
           ("free_kinematics", str(g["free_kinematics"])), ("periodic_length", "%.17g %.17g %.17g" % tuple(L)),
           ("seed", "%d" % int(g["seed"])), ("save_clones", "one_file_per_step"), ("output_name", str(tmp_path / "run_rollers")),
           ("structure", "blob.vertex rollers.clones")]
  deck = tmp_path / "inputfile_rollers.dat"
  deck.write_text("".join("%-40s %s\n" % kv for kv in lines))
  return str(deck)


@pytest.mark.parametrize("path", ROLLERS, ids=[os.path.basename(p)[4:-4] for p in ROLLERS])
def test_roller_deck_replay_matches_reference_integrator(tmp_path, path):
  """The reference's roller integrator with its body-body law in the pair-force hook (the generator says how), through a
  deck and integrator_from_input; 1e-7 deterministic, 1e-6 Brownian."""
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rollers
  g = load_golden(path)
  read = ReadInput(_roller_deck(g, tmp_path))
  integ = rollers.integrator_from_input(read, device="cuda:0")
  assert integ.body_body_force == (float(g["repulsion_strength"]), float(g["debye_length"]))
  assert np.array_equal(integ.periodic_length, g["periodic_length"])
  worst = run_and_compare(g, integ)
  print("worst %.2e" % worst)
  assert worst < (1e-7 if float(g["kT"]) == 0.0 else 1e-6), worst
  assert integ.invalid_configuration_count == int(g["invalid_configuration_count"])
  integ.close()


def test_force_evaluation_restores_the_resident_mobility_view(tmp_path):
  """72 blobs take the one-sided sweep, whose sums have a fixed order: the same product before and after a force
  evaluation (which makes the 6 centres resident and puts the blobs back) is equal bit for bit, and the body-body rows
  are the restatement's."""
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rigid_integrator
  g = load_golden([p for p in RIGID if p.endswith("g16_rigid_det_ab.npz")][0])
  integ = rigid_integrator.integrator_from_input(ReadInput(write_case(g, str(tmp_path))), device="cuda:0")
  c = integ.susp.ctx
  v = torch.as_tensor(np.random.RandomState(1).randn(3 * integ.Nblobs), device="cuda:0")
  before = c.matvec_device("tt", v, integ.eta).clone()
  FT = integ.force_torque_calculator()
  assert c.n == integ.Nblobs
  after = c.matvec_device("tt", v, integ.eta)
  assert torch.equal(before, after)
  integ.body_body_force = None
  FT0 = integ.force_torque_calculator()
  eps, b = 2.0, 0.8
  ref = bfn.forces(g["locations_shell"], None, eps, b).astype(np.float64)
  diff = (FT - FT0).cpu().numpy()
  assert np.abs(diff[:, :3] - ref).max() <= 1e-12 * np.abs(ref).max() and not np.any(diff[:, 3:])
  assert torch.equal(c.matvec_device("tt", v, integ.eta), before)
  integ.close()


def test_roller_force_path_adds_the_term_on_the_bound_positions():
  """RollersIntegrator.body_body_force: the pair-force hook returns the blob-blob forces plus the sweep over the same
  resident positions; alone (repulsion_strength = 0) it is the restatement."""
  from rigidmultiblobswall_amd.rollers import RollersIntegrator
  x, box = bfn.lattice_cloud(150, 1660, dims=2)
  x[:, 2] += 1.0
  integ = RollersIntegrator(x, "deterministic_adams_bashforth_rollers", 0.4, 1.1, device="cuda:0")
  integ.periodic_length = np.array([box, box, 0.0])
  integ.body_body_force = (0.6, 0.7)
  ref = bfn.forces(x, integ.periodic_length, 0.6, 0.7).astype(np.float64)
  alone = integ.calc_blob_blob_forces(integ.location).cpu().numpy()
  assert rel_err(alone, ref) < TOL_D2
  integ.repulsion_strength, integ.debye_length = 0.5, 0.1
  both = integ.calc_blob_blob_forces(integ.location).cpu().numpy()
  integ.body_body_force = None
  blob = integ.calc_blob_blob_forces(integ.location).cpu().numpy()
  assert rel_err(both - blob, ref) < 1e-11      # a difference of two sums
  integ.close()


def test_command_line_runs_a_rigid_deck_with_body_body_forces(tmp_path):
  import subprocess
  import sys
  from rigidmultiblobswall_amd import structures
  g = load_golden([p for p in RIGID if p.endswith("g16_rigid_det_midpoint.npz")][0])
  deck = write_case(g, str(tmp_path))
  res = subprocess.run([sys.executable, "-m", "rigidmultiblobswall_amd", "--input-file", deck], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  tl = g["trajectory_locations_shell"]
  n, loc, quat = structures.read_clones_file(os.path.join(str(tmp_path), "run.shell.%08d.clones" % (len(tl) - 1)))
  assert np.abs(loc - tl[-1]).max() < 1e-7 * np.abs(tl[-1] - tl[0]).max()
