"""Rigid multiblobs above a free (stress-free) surface, host side: which decks are accepted, the golden `operator` of
tools/gen_golden_free_surface.py against a numpy restatement of the block (this pins the golden itself), and the g15
decks through the oracle-backed CPU stack."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err
from _oracle_ctx import OracleContext
from _rigid_common import replay, reference_counters, write_case


# ---- numpy restatement of the free-surface block (mobility_numba.py:1840-1926) ----------------------------------------
def _rpy(d):
  """(..., 3) separations in units of a -> (..., 3, 3) RPY blocks in units of 1 / (8 pi eta a); r <= 2: overlapping form."""
  r2 = np.sum(d * d, axis=-1)
  r = np.sqrt(r2)
  with np.errstate(divide="ignore", invalid="ignore"):
    far = r > 2
    c1 = np.where(far, (1.0 + 2.0 / (3.0 * r2)) / r, 4.0 / 3.0 * (1.0 - 0.28125 * r))
    c2 = np.where(far, (1.0 - 2.0 / r2) / r2 / r, 4.0 / 3.0 * 0.09375 / r)
    c2 = np.where(r2 > 0, c2, 0.0)                     # d = 0 (a blob with itself): the caller overwrites that block
  return c1[..., None, None] * np.eye(3) + c2[..., None, None] * d[..., :, None] * d[..., None, :]


def free_surface_dense(r, eta, a):
  """(3N, 3N) blob mobility above a free surface at z = 0: RPY(r_i - r_j) + RPY(x, y, z_i + z_j) with the image's z column
  negated (+ on xx, xy, yx, yy, zx, zy; - on xz, yz, zz); self block 4/3 I + the blob's own image at distance 2 z_i / a."""
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  n = len(r)
  d = (r[:, None, :] - r[None, :, :]) / a
  M = _rpy(d)
  M[np.arange(n), np.arange(n)] = 4.0 / 3.0 * np.eye(3)
  R = d.copy()
  R[..., 2] = (r[:, None, 2] + r[None, :, 2]) / a
  image = _rpy(R)
  image[..., :, 2] *= -1.0
  return ((M + image) / (8.0 * np.pi * eta * a)).transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)


def dense_K(r, locations, n_b):
  """(3N, 6 n_bodies) geometric matrix: rows of blob i of body b are [I, -(r_i - x_b) x]."""
  r = np.asarray(r).reshape(-1, 3)
  K = np.zeros((3 * len(r), 6 * len(locations)))
  for i, x in enumerate(r):
    b = i // n_b
    rx, ry, rz = x - locations[b]
    K[3 * i:3 * i + 3, 6 * b:6 * b + 3] = np.eye(3)
    K[3 * i:3 * i + 3, 6 * b + 3:6 * b + 6] = [[0, rz, -ry], [-rz, 0, rx], [ry, -rx, 0]]
  return K


class FreeSurfaceOracleContext(OracleContext):
  """The CPU stand-in with the oracle's free-surface product behind kind "tt_free" (raw heights, as the engine's)."""

  def _wrapped(self, kind, v, eta, in_plane):
    if kind != "tt_free":
      return OracleContext._wrapped(self, kind, v, eta, in_plane)
    assert not self.wall and not in_plane
    return self.o.free_surface_mobility_trans_times_force_oracle(self.r, v.detach().cpu().numpy(), eta, self.a, periodic_length=self.L)


def _golden(name):
  return load_golden(os.path.join(GOLDEN, "g15_free_surface_%s.npz" % name))


# ---- the golden operator --------------------------------------------------------------------------------------------
def test_golden_operator_equals_the_numpy_block():
  g = _golden("operator")
  r, x, a, eta = g["r_vectors"].reshape(-1, 3), g["vector"], float(g["blob_radius"]), float(g["eta"])
  assert float(r[:, 2].min()) < a                      # the image's overlapping branch is in the fixture
  n3 = r.size
  M = free_surface_dense(r, eta, a)
  assert np.abs(M - M.T).max() <= 1e-15 * np.abs(M).max()
  assert rel_err(M @ x[:n3], g["product"]) <= 1e-13
  K = dense_K(r, g["locations"], len(g["vertex"]))
  want = np.concatenate([M @ x[:n3] - K @ x[n3:], -K.T @ x[:n3]])
  assert rel_err(want, g["operator"]) <= 1e-13


def test_numpy_block_equals_the_oracle_product(oracle):
  rng = np.random.RandomState(3)
  a, eta = 0.3, 0.9
  r = np.column_stack([3 * rng.rand(40), 3 * rng.rand(40), 0.05 + 1.5 * rng.rand(40)])
  r[1] = r[0] + [2 * a, 0, 0]                          # a touching pair
  f = rng.randn(120)
  assert r[:, 2].min() < a
  assert rel_err(free_surface_dense(r, eta, a) @ f, oracle.free_surface_mobility_trans_times_force_oracle(r, f, eta, a)) <= 1e-13


# ---- which decks run --------------------------------------------------------------------------------------------------
def _deck(tmp_path, blobs, product, scheme="deterministic_forward_euler", extra="", structure="structure body.vertex body.clones"):
  (tmp_path / "body.vertex").write_text("3\n0 0 0\n1 0 0\n0 1 0\n")
  (tmp_path / "body.clones").write_text("1\n0 0 3 1 0 0 0\n")
  deck = tmp_path / "inputfile.dat"
  deck.write_text("""scheme %s
mobility_blobs_implementation %s
mobility_vector_prod_implementation %s
blob_radius 0.25
eta 1.0
dt 0.01
n_steps 1
output_name %s
%s
%s
""" % (scheme, blobs, product, str(tmp_path / "run"), structure, extra))
  return str(deck)


@pytest.mark.parametrize("blobs,product,block_boundary", [
    ("python_no_wall", "numba_free_surface", "no_wall"),
    ("C++_no_wall", "pycuda_free_surface", "no_wall"),
    ("numba_no_wall", "hip_free_surface", "no_wall"),
])
def test_free_surface_decks_with_unbounded_blocks_are_accepted(oracle, tmp_path, blobs, product, block_boundary):
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rigid_integrator as ri
  integ = ri.integrator_from_input(ReadInput(_deck(tmp_path, blobs, product)), device="cpu", ctx=FreeSurfaceOracleContext(oracle))
  assert integ.domain == "free_surface" and integ.susp.boundary == "free_surface" and integ.susp.block_boundary == block_boundary
  assert integ.susp.wall is False and integ.susp.ctx_wall is False and integ.susp._tt == "tt_free"       # a stand-in context: raw heights + the free-surface kind
  integ.advance_time_step(0.01, step=0)
  assert integ.det_iterations_count > 0


def test_free_surface_blocks_are_accepted_by_the_deck_check_and_need_the_engine(oracle, tmp_path):
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import deck_modes, rigid_integrator as ri
  read = ReadInput(_deck(tmp_path, "hip_free_surface", "hip_free_surface"))
  assert deck_modes.validate(read) == "free_surface" and deck_modes.free_surface_blocks(read) == "free_surface"
  read = ReadInput(_deck(tmp_path, "C++_free_surface", "numba_free_surface", scheme="deterministic_forward_euler_dense_algebra"))
  assert deck_modes.validate(read) == "free_surface"
  integ = ri.integrator_from_input(read, device="cpu", ctx=FreeSurfaceOracleContext(oracle))
  with pytest.raises(ValueError, match="free surface"):       # the stand-in has no dense free-surface blocks
    integ.susp.dense_blob_mobility()


@pytest.mark.parametrize("blobs,product,scheme,extra,needle", [
    ("python", "numba_free_surface", "deterministic_forward_euler", "", "free surface"),            # wall blocks
    ("C++", "pycuda_free_surface", "deterministic_forward_euler", "", "free surface"),
    ("C++_free_surface", "numba", "deterministic_forward_euler", "", "free surface"),               # free-surface blocks, wall product
    ("hip_free_surface", "numba_no_wall", "deterministic_forward_euler", "domain no_wall", "free surface"),   # ... unbounded product
    ("python_no_wall", "numba_free_surface", "deterministic_forward_euler", "domain no_wall", "domain"),
    ("python_no_wall", "numba_free_surface", "deterministic_forward_euler_dense_algebra", "", "free surface"),
    ("python_no_wall", "radii_numba_free_surface", "deterministic_forward_euler", "", "radii"),
])
def test_inconsistent_free_surface_decks_raise(oracle, tmp_path, blobs, product, scheme, extra, needle):
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rigid_integrator as ri
  with pytest.raises(ValueError, match=needle):
    ri.integrator_from_input(ReadInput(_deck(tmp_path, blobs, product, scheme=scheme, extra=extra)), device="cpu",
                             ctx=FreeSurfaceOracleContext(oracle))


def test_phoretic_decks_and_roller_decks_above_a_free_surface_raise(oracle, tmp_path):
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rigid_integrator as ri, rollers
  (tmp_path / "body.Laplace").write_text("".join("0 0 1 0 1 1 1\n" for _ in range(3)))
  deck = _deck(tmp_path, "python_no_wall", "numba_free_surface", structure="structure body.vertex body.clones body.Laplace")
  with pytest.raises(ValueError, match="free surface"):
    ri.integrator_from_input(ReadInput(deck), device="cpu", ctx=FreeSurfaceOracleContext(oracle))
  deck = _deck(tmp_path, "python_no_wall", "numba_free_surface", scheme="deterministic_forward_euler_rollers")
  with pytest.raises(ValueError, match="free surface"):
    rollers.integrator_from_input(ReadInput(deck), device="cpu", ctx=FreeSurfaceOracleContext(oracle))


def test_contexts_and_precisions_that_are_not_served_raise(oracle):
  from rigidmultiblobswall_amd.rigid import RigidSuspension
  from rigidmultiblobswall_amd.rigid_integrator import RigidIntegrator
  ref = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
  loc, quat = np.array([[0.0, 0, 3]]), np.array([[1.0, 0, 0, 0]])

  from rigidmultiblobswall_amd.multi import MultiContext
  from rigidmultiblobswall_amd.distributed import ReplicatedContext
  from rigidmultiblobswall_amd.laplace import PhoreticSlip
  for base in (MultiContext, ReplicatedContext):      # refused by class, subclasses included (no engine is created here)
    class Facade(base):
      def __init__(self):
        pass

      def __del__(self):
        pass
    with pytest.raises(ValueError, match="free surface"):
      RigidSuspension([ref], loc, quat, 0.25, 1.0, boundary="free_surface", device="cpu", ctx=Facade())
  with pytest.raises(ValueError, match="block_boundary"):
    RigidSuspension([ref], loc, quat, 0.25, 1.0, boundary="single_wall", block_boundary="no_wall", device="cpu", ctx=OracleContext(oracle))
  integ = RigidIntegrator([ref], loc, quat, "deterministic_forward_euler", 0.25, 1.0, domain="free_surface", device="cpu",
                          ctx=FreeSurfaceOracleContext(oracle), block_boundary="no_wall")
  assert integ.susp.wall is False            # a boolean: a free surface is not a no-slip wall
  with pytest.raises(ValueError, match="free surface"):
    PhoreticSlip(integ.susp, np.tile([0.0, 0, 1, 0, 1, 1, 1], (3, 1)))
  with pytest.raises(ValueError, match="free surface"):
    integ.precision = "single"
  with pytest.raises(ValueError, match="free surface"):
    integ.susp.solve_mixed_precision(torch.ones(integ.susp.size, dtype=torch.float64))
  # wall = True / False keep their meaning
  assert RigidSuspension([ref], loc, quat, 0.25, 1.0, wall=True, device="cpu", ctx=OracleContext(oracle)).boundary == "single_wall"
  assert RigidSuspension([ref], loc, quat, 0.25, 1.0, wall=False, device="cpu", ctx=OracleContext(oracle)).boundary == "no_wall"


def test_lockstep_products_count_one_sweep_per_vector(oracle):
  from rigidmultiblobswall_amd.rigid import RigidSuspension
  ref = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
  rs = RigidSuspension([ref], np.array([[0.0, 0, 0.2]]), np.array([[1.0, 0, 0, 0]]), 0.25, 1.0, boundary="free_surface",
                       block_boundary="no_wall", device="cpu", ctx=FreeSurfaceOracleContext(oracle))
  vs = [torch.randn(9, dtype=torch.float64) for _ in range(3)]
  out = rs.mobility_times_lambdas(vs)
  assert rs.sweep_count == 3 and rs.matvec_count == 3 and rs.matvec2_count == 0
  M = free_surface_dense(rs.r_vectors, 1.0, 0.25)
  for v, u in zip(vs, out):
    assert rel_err(u.numpy(), M @ v.numpy()) <= 1e-13


# ---- the g15 decks through the oracle-backed stack -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["det_euler_shells", "det_ab_shells", "slip_trapz_shells", "det_euler_mixed"])
def test_g15_decks_on_the_oracle_backed_stack(oracle, tmp_path, name):
  g = _golden(name)
  assert float(g["lowest_blob"]) < float(g["blob_radius"])
  integ, worst_x, worst_q = replay(g, tmp_path, "cpu", FreeSurfaceOracleContext(oracle))
  tol = 1e-7 if float(g["kT"]) == 0.0 else 1e-6
  assert worst_x < tol and worst_q < tol, (worst_x, worst_q)
  ref = reference_counters(g)
  assert integ.invalid_configuration_count == ref["invalid_configuration_count"] == 0
  assert integ.det_iterations_count == ref["deterministic_iterations_count"]
  assert integ.stoch_iterations_count == ref["stochastic_iterations_count"]


def _utility_deck(g, tmp_path, scheme, blocks="python_no_wall", extra=""):
  deck = write_case(dict(g, deck=str(g["deck"]).replace("deterministic_forward_euler", scheme).replace("python_no_wall", blocks) + extra),
                    str(tmp_path))
  return deck


def test_mobility_utility_follows_the_decks_boundary(oracle, tmp_path):
  """utilities.run, scheme `mobility`, on the 8-shell deck: the velocities solve the free-surface saddle-point system."""
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import utilities
  g = _golden("det_euler_shells")
  out = utilities.run(ReadInput(_utility_deck(g, tmp_path, "mobility")), device="cpu", ctx=FreeSurfaceOracleContext(oracle))
  r, a = out["r_vectors"], float(g["blob_radius"])
  M, K = free_surface_dense(r, 1.1, a), dense_K(r, g["locations_shell"], 12)
  lam, U = out["lambda_blobs"].reshape(-1), out["velocity"].reshape(-1)
  assert np.linalg.norm(M @ lam - K @ U) <= 1e-8 * np.linalg.norm(K @ U)          # no slip; solver_tolerance 1e-10
  assert rel_err(K.T @ lam, out["force"]) <= 1e-12
  assert rel_err(np.loadtxt(str(tmp_path / "run.velocity.dat")), out["velocity"]) <= 1e-15
  with pytest.raises(ValueError, match="free surface"):
    utilities.run(ReadInput(_utility_deck(g, tmp_path, "mobility", blocks="python")), device="cpu", ctx=FreeSurfaceOracleContext(oracle))
