"""Golden data for the body-body forces (tests/golden/g16_*).  Build-container only: needs the reference checkout.

Everything recorded here is computed by the reference's own code, on the CPU:
  * g16_body_forces.npz -- multi_bodies_functions.calc_body_body_forces_torques_python on clouds of body locations
    (N_b = 2, 65, 200; open, periodic in x and y, periodic in all three directions; centres on both sides of the half box);
  * g16_rigid_*.npz -- the reference's driver (multi_bodies.py) on decks of six 12-blob shells with
    `body_body_force_torque_implementation python`, through oracle/gen_golden_rigid_integrator.py's runner (its deck
    template with the option and the two force parameters replaced; nothing in oracle/ is edited);
  * g16_rollers_*.npz -- the reference's roller integrator (QuaternionIntegratorRollers) through
    oracle/gen_golden_rollers.py's builder.  That integrator takes its forces from two hooks, calc_one_blob_forces and
    calc_blob_blob_forces (quaternion_integrator_rollers.py:930-933), and never calls the body-body function itself; the
    pair-force hook here returns the reference's blob-blob forces plus the reference's
    calc_body_body_forces_torques_python evaluated on the same coordinates (every roller is a body located at its blob),
    with the deck's repulsion_strength / debye_length for both laws, as the reference's kwargs.

Every trajectory is run a second time without the body-body term; the generator asserts that this run ends further from
the recorded one than 100 x the tolerance the replay tests compare with (1e-7 deterministic, 1e-6 Brownian, relative to
the largest displacement), so a stepper that drops the term cannot pass.

Usage:  python tools/gen_golden_body_forces.py --ref REFERENCE_CHECKOUT [--out tests/golden] [--only forces|rigid|rollers]
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_rigid_integrator as gri  # noqa: E402
import gen_golden_rollers as gro  # noqa: E402


def jittered_lattice(rng, n, spacing, jitter):
  """n points of a cubic lattice of the given spacing, each moved by at most `jitter` per direction: the smallest
  separation is >= spacing - 2 sqrt(3) jitter."""
  m = int(np.ceil(n ** (1.0 / 3.0)))
  ijk = np.array([(i, j, k) for i in range(m) for j in range(m) for k in range(m)], dtype=float)
  pick = rng.permutation(len(ijk))[:n]
  return ijk[pick] * spacing + jitter * (2.0 * rng.rand(n, 3) - 1.0)


def body_force_cases(mbf, out_dir):
  rng = np.random.RandomState(1601)
  eps, b = 1.7, 0.9
  data = {"names": []}
  for n in (2, 65, 200):
    m = int(np.ceil(n ** (1.0 / 3.0)))
    spacing, jitter = 1.3, 0.1          # smallest separation >= 1.3 - 0.35 > b
    x = jittered_lattice(rng, n, spacing, jitter) + 0.37
    if n == 2:
      x = np.array([[0.4, 0.3, 0.6], [0.4 + 0.7 * spacing * m, 0.9, 1.5]])      # further apart than half the box in x
    box = spacing * m       # the lattice fills the box: pairs on both sides of L/2 in every periodic direction
    for tag, L in (("open", (0.0, 0.0, 0.0)), ("xy", (box, 1.1 * box, 0.0)), ("xyz", (box, 1.1 * box, box))):
      L = np.array(L)
      d = x[:, None, :] - x[None, :, :]
      for k in range(3):
        if L[k] > 0:
          d[..., k] -= np.rint(d[..., k] / L[k]) * L[k]
      r = np.linalg.norm(d, axis=-1) + 1e9 * np.eye(n)
      assert r.min() >= b, (n, tag, r.min())                    # smallest minimal-image separation >= b
      assert np.abs(x[:, None, :] - x[None, :, :]).max() > 0.5 * box      # pairs on both sides of the half box
      bodies = [types.SimpleNamespace(location=np.copy(xi), orientation=None) for xi in x]
      ft = mbf.calc_body_body_forces_torques_python(bodies, x, periodic_length=L, repulsion_strength=eps, debye_length=b)
      name = "n%d_%s" % (n, tag)
      data["names"].append(name)
      data["x_" + name], data["L_" + name], data["FT_" + name] = x, L, ft
      print("  g16_body_forces %-12s max|F| = %.3e" % (name, np.abs(ft).max()), flush=True)
  data["names"] = np.array(data["names"])
  np.savez_compressed(os.path.join(out_dir, "g16_body_forces.npz"), repulsion_strength=eps, debye_length=b, **data)


# ---- rigid decks through the reference's driver -------------------------------------------------------------------
def rigid_cases(ref, out_dir):
  from read_input import read_vertex_file
  shell = read_vertex_file.read_vertex_file(os.path.join(ref, "multi_bodies", "Structures", "shell_N_12_Rg_0.3960_Rh_0.5.vertex"))[:, :3]
  rng = np.random.RandomState(1602)
  loc = np.array([[1.6 * (k % 3) + 0.1 * rng.rand(), 1.6 * (k // 3) + 0.1 * rng.rand(), 1.1 + 0.4 * rng.rand()] for k in range(6)])
  bodies = [("shell", shell, loc, gri.random_quaternions(rng, 6))]
  template = gri.DECK
  assert "body_body_force_torque_implementation    None" in template and "repulsion_strength                       0.3" in template
  # a Debye length of the order of the spacing, so that the term between the centres (1.6 apart) moves the shells
  forces = template.replace("repulsion_strength                       0.3", "repulsion_strength                       2.0") \
                   .replace("debye_length                             0.1", "debye_length                             0.8")
  assert forces != template
  with_term = forces.replace("body_body_force_torque_implementation    None", "body_body_force_torque_implementation    python")
  cases = [("g16_rigid_det_ab", "deterministic_adams_bashforth", 5, {}, 1e-7),
           ("g16_rigid_det_midpoint", "deterministic_midpoint", 3, {}, 1e-7),
           ("g16_rigid_stoch_slip_trapz", "stochastic_Slip_Trapz", 3, dict(kT=0.0041, seed=16), 1e-6)]
  scratch = tempfile.mkdtemp(prefix="g16_none_")
  try:
    for name, scheme, n_steps, kw, tol in cases:
      gri.DECK = with_term
      gri.case(ref, out_dir, name, scheme, bodies, n_steps, a=0.25, **kw)
      gri.DECK = forces
      gri.case(ref, scratch, name, scheme, bodies, n_steps, a=0.25, **kw)
      g, g0 = np.load(os.path.join(out_dir, name + ".npz")), np.load(os.path.join(scratch, name + ".npz"))
      assert "body_body_force_torque_implementation    python" in str(g["deck"])
      t, t0 = g["trajectory_locations_shell"], g0["trajectory_locations_shell"]
      apart = np.abs(t[-1] - t0[-1]).max() / np.abs(t[-1] - t[0]).max()
      print("  %-32s without the term: %.3e of the largest displacement away" % (name, apart), flush=True)
      assert apart > 100 * tol, (name, apart)
  finally:
    gri.DECK = template


# ---- rollers through the reference's integrator ---------------------------------------------------------------------
def roller_trajectory(lib, scheme, r0, p, n_steps, body_body):
  mbf = lib[3]
  integ = gro.make_integrator(lib, r0, scheme, p)
  if body_body:
    blob_blob = integ.calc_blob_blob_forces
    L = np.asarray(p["periodic_length"], dtype=float)

    def pair_forces(r_vectors, *args, **kwargs):
      r = np.reshape(r_vectors, (-1, 3))
      bodies = [types.SimpleNamespace(location=np.copy(x), orientation=None) for x in r]
      ft = mbf.calc_body_body_forces_torques_python(bodies, r, periodic_length=L, repulsion_strength=p["repulsion_strength"],
                                                    debye_length=p["debye_length"])
      return blob_blob(r_vectors, *args, **kwargs) + ft[0::2]
    integ.calc_blob_blob_forces = pair_forces
  np.random.seed(p["seed"])
  traj = [r0.copy()]
  for _ in range(n_steps):
    integ.advance_time_step(p["dt"])
    traj.append(np.array([b.location for b in integ.bodies]))
  return np.array(traj), integ


def roller_cases(lib, out_dir):
  cases = [("g16_rollers_det_ab_periodic", "deterministic_adams_bashforth_rollers", 12, 4, dict(periodic_length=(4.2, 4.2, 0.0)), 1e-7),
           ("g16_rollers_stoch_ab", "stochastic_adams_bashforth_rollers", 12, 3, dict(kT=0.0041, seed=17), 1e-6)]
  for name, scheme, N, n_steps, over, tol in cases:
    p = dict(gro.BASE)
    p.update(debye_length=0.4)       # of the order of the spacing (2.6 a = 1.04): the term between the centres matters
    p.update(over)
    r0 = gro.suspension(N, p["a"], seed=1600 + N)
    traj, integ = roller_trajectory(lib, scheme, r0, p, n_steps, True)
    traj0, _ = roller_trajectory(lib, scheme, r0, p, n_steps, False)
    apart = np.abs(traj[-1] - traj0[-1]).max() / np.abs(traj[-1] - traj[0]).max()
    print("  %-32s without the term: %.3e of the largest displacement away" % (name, apart), flush=True)
    assert apart > 100 * tol, (name, apart)
    data = {k: (np.asarray(v) if not isinstance(v, str) else v) for k, v in p.items()}
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), scheme=scheme, trajectory=traj, n_steps=n_steps,
                        wall_overlaps=integ.wall_overlaps, invalid_configuration_count=integ.invalid_configuration_count, **data)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--ref", required=True, help="checkout of the reference (RigidMultiblobsWall)")
  ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
  ap.add_argument("--only", default=None, choices=[None, "forces", "rigid", "rollers"])
  args = ap.parse_args()
  out_dir = os.path.abspath(args.out)
  lib = gro.load(args.ref)         # numba stub, the reference on sys.path, its modules
  if args.only in (None, "forces"):
    body_force_cases(lib[3], out_dir)
  if args.only in (None, "rollers"):
    roller_cases(lib, out_dir)
  if args.only in (None, "rigid"):
    gri.prepare(args.ref)          # + the gmres keyword shim the driver's solves need
    rigid_cases(args.ref, out_dir)


if __name__ == "__main__":
  main()
