"""Rollers above a free (stress-free) surface, host side: the mirror-image construction the GPU kernels are checked
against (tests/_free_surface_mirror.py), the `domain free_surface` roller decks, and one step on the CPU stand-in."""
import numpy as np
import pytest
import torch

from _oracle_ctx import OracleContext
import _free_surface_mirror as fm
from test_rollers_host import _write_deck

ETA, A = 1.1, 0.3


@pytest.mark.parametrize("n,periodic", [(40, False), (24, True)])
def test_mirror_construction_reproduces_the_references_translation_product(oracle, n, periodic):
  r = fm.cloud(n, A, 5 + n)
  L = fm.periodic_box(n, A) if periodic else None
  f = np.random.RandomState(n).randn(3 * n)
  kw = {"periodic_length": L} if periodic else {}
  want = oracle.free_surface_mobility_trans_times_force_oracle(r, f, ETA, A, **kw)
  err = np.linalg.norm(fm.product(oracle, "tt", r, f, ETA, A, L) - want) / np.linalg.norm(want)
  print("n = %d periodic = %s: mirror tt against the oracle's free-surface product %.3e" % (n, periodic, err))
  assert err <= 1e-13


@pytest.mark.parametrize("periodic", [False, True])
def test_grand_mobility_of_the_mirror_system_is_symmetric_and_open_positive_definite(oracle, periodic):
  n = 24
  r = fm.cloud(n, A, 29)
  G = fm.dense_grand(oracle, r, ETA, A, fm.periodic_box(n, A) if periodic else None)
  asym = np.abs(G - G.T).max() / np.abs(G).max()
  print("periodic = %s: asymmetry %.3e of the largest entry" % (periodic, asym))
  assert asym <= 8 * 4e-16
  if not periodic:
    lam = np.linalg.eigvalsh(0.5 * (G + G.T)).min()
    print("smallest eigenvalue %.3e" % lam)
    assert lam > 0.0


R0 = np.array([[0.0, 0.0, 1.0], [3.0, 0.0, 1.5], [0.0, 3.0, 1.2]])


def _free_deck(tmp_path, domain="free_surface", scheme="deterministic_forward_euler_rollers", extra=""):
  deck = _write_deck(tmp_path, R0, scheme=scheme, extra="domain %s\n%s" % (domain, extra))
  text = open(deck).read().replace("mobility_vector_prod_implementation    pycuda", "mobility_vector_prod_implementation    numba_free_surface")
  open(deck, "w").write(text)
  return deck


def test_roller_decks_with_domain_free_surface(oracle, tmp_path):
  from rigidmultiblobswall_amd.read_input import ReadInput
  from rigidmultiblobswall_amd import rollers, rigid_integrator, deck_modes
  read = ReadInput(_free_deck(tmp_path))
  assert deck_modes.validate(read, uses_dense_blocks=False) == "free_surface"
  ctx = fm.MirrorContext(oracle)
  integ = rollers.integrator_from_input(read, device="cpu", ctx=ctx)
  assert integ.domain == "free_surface" and ctx.get_option("free_surface_rotation") == 1
  # the reference's spelling of the boundary still names products the reference does not have
  with pytest.raises(ValueError, match="free surface"):
    rollers.integrator_from_input(ReadInput(_free_deck(tmp_path, domain="single_wall")), device="cpu", ctx=fm.MirrorContext(oracle))
  # the engine's spelling needs the free-surface product, and is for roller decks
  deck = _free_deck(tmp_path)
  text = open(deck).read().replace("numba_free_surface", "numba")
  open(deck, "w").write(text)
  with pytest.raises(ValueError, match="free_surface"):
    rollers.integrator_from_input(ReadInput(deck), device="cpu", ctx=fm.MirrorContext(oracle))
  with pytest.raises(ValueError, match="single_wall"):
    deck_modes.validate(ReadInput(_free_deck(tmp_path)), uses_dense_blocks=True)
  with pytest.raises(ValueError, match="single_wall"):
    rigid_integrator.integrator_from_input(ReadInput(_free_deck(tmp_path, scheme="deterministic_forward_euler")), device="cpu",
                                           ctx=fm.MirrorContext(oracle))
  # wall formulas of the uncorrelated schemes, single precision, contexts without the option
  with pytest.raises(ValueError, match="free surface"):
    rollers.integrator_from_input(ReadInput(_free_deck(tmp_path, extra="hydro_interactions 0")), device="cpu", ctx=fm.MirrorContext(oracle))
  with pytest.raises(ValueError, match="free surface"):
    integ.precision = "single"
  with pytest.raises(ValueError, match="free surface"):
    rollers.RollersIntegrator(R0, "deterministic_forward_euler", A, ETA, domain="free_surface", device="cpu", ctx=OracleContext(oracle))
  from rigidmultiblobswall_amd.multi import MultiContext
  from rigidmultiblobswall_amd.distributed import ReplicatedContext
  for base in (MultiContext, ReplicatedContext):      # refused by class (no engine is created here)
    class Facade(base):
      def __init__(self):
        pass

      def __del__(self):
        pass
    with pytest.raises(ValueError, match="free surface"):
      rollers.RollersIntegrator(R0, "deterministic_forward_euler", A, ETA, domain="free_surface", device="cpu", ctx=Facade())


def test_one_forward_euler_step_of_three_rollers_on_the_stand_in(oracle):
  """r + dt (M_tt F + M_tr T) with F = gravity + wall repulsion + blob-blob repulsion and the constant torque of free
  kinematics, the products from the mirror construction."""
  from rigidmultiblobswall_amd.rollers import RollersIntegrator
  a, eta, dt = 0.4, 1.3, 0.01
  r0 = np.array([[0.0, 0.0, 0.9], [1.0, 0.1, 0.5], [0.2, 1.1, 0.35]])      # the last one below z = a
  ctx = fm.MirrorContext(oracle)
  integ = RollersIntegrator(r0, "deterministic_forward_euler", a, eta, domain="free_surface", device="cpu", ctx=ctx)
  integ.g, integ.repulsion_strength_wall, integ.debye_length_wall = 0.3, 0.05, 0.1
  integ.repulsion_strength, integ.debye_length = 0.02, 0.1
  integ.omega_one_roller = np.array([0.0, 5.0, 0.0])
  F = (integ.calc_one_blob_forces(integ.location) + integ.calc_blob_blob_forces(integ.location)).numpy().reshape(-1)
  T = integ.get_torque().numpy()
  assert np.any(T != 0) and np.any(F[:2] != 0)
  integ.advance_time_step(dt)
  want = r0.reshape(-1) + dt * fm.fused_row(oracle, r0, F, T, eta, a)
  got = integ.location.numpy().reshape(-1)
  err = np.abs(got - want).max() / np.abs(want).max()
  print("forward Euler step against the mirror products: %.3e" % err)
  assert err <= 1e-12
  assert integ.wall_overlaps == int(np.sum(got.reshape(-1, 3)[:, 2] < a)) >= 1
  assert ctx.free_surface and ctx.get_option("free_surface_rotation") == 1
  # a step that ends below the surface is rejected as with the wall
  assert not integ._valid(torch.tensor([[0.0, 0.0, -0.1]], dtype=torch.float64))
