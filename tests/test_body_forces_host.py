"""Body-body forces, host side: the numpy restatement against the reference's recorded forces (tests/golden/g16_body_forces.npz,
tools/gen_golden_body_forces.py), the C exports, deck validation and the dispatch table.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import _body_forces_numpy as bfn
from conftest import ROOT, golden_files, load_golden
from _oracle_ctx import OracleContext
from test_rollers_host import _write_deck


def _cases():
  g = load_golden(golden_files("g16_body_forces.npz")[0])
  return g, [str(n) for n in g["names"]]


def test_restatement_reproduces_the_reference_forces():
  """Long double restatement against calc_body_body_forces_torques_python: 1e-13 of the largest force component.  The
  restatement in double sits 1.9e-16 .. 1.7e-15 max|F| from itself in long double on these clouds (printed)."""
  g, names = _cases()
  assert sorted(names) == sorted("n%d_%s" % (n, t) for n in (2, 65, 200) for t in ("open", "xy", "xyz"))
  eps, b = float(g["repulsion_strength"]), float(g["debye_length"])
  for name in names:
    x, L, FT = g["x_" + name], g["L_" + name], g["FT_" + name]
    assert FT.shape == (2 * len(x), 3) and not np.any(FT[1::2])      # the law has no torque
    F = bfn.forces(x, L, eps, b)
    scale = np.abs(FT).max()
    err = float(np.abs(F - FT[0::2]).max() / scale)
    self_err = float(np.abs(bfn.forces(x, L, eps, b, dtype=np.float64) - F).max() / scale)
    print("%-10s restatement - reference %.2e max|F|, double - long double %.2e max|F|" % (name, err, self_err))
    assert err <= 1e-13
    assert np.abs(np.sum(F, axis=0)).max() <= 1e-15 * np.abs(F).sum()      # F_ji = -F_ij


def test_restated_force_is_minus_the_gradient_of_the_yukawa_energy():
  """The cloud and step of the GPU gradient test (_body_forces_numpy.GRADIENT): the central difference of the restated
  energy, in long double (truncation alone) and in double (with the rounding eps U / h), stays within 1e-7 |F| of
  -F . delta, so that bound can be asked of the kernels."""
  GRADIENT, gradient_cloud = bfn.GRADIENT, bfn.gradient_cloud
  x, L, eps, b, h = gradient_cloud()
  F = bfn.forces(x, L, eps, b)
  nF = float(np.linalg.norm(F.astype(np.float64)))
  rng = np.random.RandomState(GRADIENT["seed"])
  for _ in range(GRADIENT["directions"]):
    delta = rng.randn(*x.shape)
    delta /= np.linalg.norm(delta)
    want = -float(np.sum(F * delta))
    for dtype in (np.longdouble, np.float64):
      fd = float((bfn.energy(x + h * delta, L, eps, b, dtype) - bfn.energy(x - h * delta, L, eps, b, dtype)) / (2 * h))
      print("%-10s dU/dh %.12e  -F.delta %.12e  |F| %.6e  miss %.2e |F|" % (dtype.__name__, fd, want, nF, abs(fd - want) / nF))
      assert abs(fd - want) <= 1e-7 * nF


def test_both_exports_exist_and_refuse_a_null_context():
  from rigidmultiblobswall_amd import _lib
  lib = _lib.load()
  header = open(os.path.join(ROOT, "include", "rmb_mobility.h")).read()
  for name in ("rmb_body_body_force", "rmb_body_body_force_device"):
    assert name in _lib.SYMBOLS and ("int %s(" % name) in header
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert getattr(lib, name)(None, 1.0, 1.0, None) < 0


def _read_roller_deck(tmp_path, line):
  from rigidmultiblobswall_amd.read_input import ReadInput
  r0 = np.array([[0.0, 0.0, 1.0], [3.0, 0.0, 1.5], [0.0, 3.0, 1.2]])
  return ReadInput(_write_deck(tmp_path, r0, extra=line))


@pytest.mark.parametrize("impl", ["python", "hip"])
def test_deck_validation_accepts_the_option_with_the_capability_flag(tmp_path, impl):
  from rigidmultiblobswall_amd import deck_modes
  read = _read_roller_deck(tmp_path, "body_body_force_torque_implementation " + impl)
  assert read.body_body_force_torque_implementation == impl
  assert deck_modes.validate(read, uses_dense_blocks=False, body_body_forces=True) == "single_wall"
  for kw in ({}, {"body_body_forces": False}):       # the default keeps refusing
    with pytest.raises(ValueError, match="body-body"):
      deck_modes.validate(read, uses_dense_blocks=False, **kw)


def test_deck_is_refused_on_a_context_without_the_sweep(oracle, tmp_path):
  from rigidmultiblobswall_amd import rollers
  assert not hasattr(OracleContext(oracle), "body_body_force_device")
  read = _read_roller_deck(tmp_path, "body_body_force_torque_implementation hip")
  with pytest.raises(ValueError, match="body-body"):
    rollers.integrator_from_input(read, device="cpu", ctx=OracleContext(oracle))


def test_the_multi_device_contexts_do_not_claim_the_sweep():
  from rigidmultiblobswall_amd import MobilityContext
  from rigidmultiblobswall_amd.multi import MultiContext
  from rigidmultiblobswall_amd.distributed import ReplicatedContext
  assert hasattr(MobilityContext, "body_body_force") and hasattr(MobilityContext, "body_body_force_device")
  for cls in (MultiContext, ReplicatedContext):
    assert not hasattr(cls, "body_body_force_device")


def test_deck_with_an_unknown_body_body_string_is_refused(tmp_path):
  from rigidmultiblobswall_amd import deck_modes
  read = _read_roller_deck(tmp_path, "body_body_force_torque_implementation fortran")
  for flag in (False, True):
    with pytest.raises(ValueError, match="unknown"):
      deck_modes.validate(read, uses_dense_blocks=False, body_body_forces=flag)


def test_dispatch_table():
  from rigidmultiblobswall_amd import dispatch, forces
  assert dispatch.set_body_body_forces_torques("hip") is forces.calc_body_body_forces_torques_hip
  assert dispatch.set_body_body_forces_torques("python") is forces.calc_body_body_forces_torques_hip
  zero = dispatch.set_body_body_forces_torques("None")
  out = zero([object()] * 4, np.zeros((9, 3)), periodic_length=np.zeros(3), repulsion_strength=1.0, debye_length=1.0)
  assert out.shape == (8, 3) and not np.any(out)
  with pytest.raises(ValueError, match="body_body_force_torque_implementation"):
    dispatch.set_body_body_forces_torques("numba")
