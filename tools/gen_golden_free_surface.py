"""Golden data of rigid multiblobs above a free (stress-free) surface from the reference's OWN driver.  Build-container
only (needs the reference tree).

Writes, under tests/golden/:
  g15_free_surface_det_euler_shells.npz, _det_ab_shells.npz     8 twelve-blob shells (shell_N_12_Rg_0_7921_Rh_1.vertex,
                                a = 0.41642), 4 steps: one body shape, the whole-loop solver path
  g15_free_surface_slip_trapz_shells.npz                        the same bodies, stochastic_Slip_Trapz, kT > 0, seeded, 3 steps
  g15_free_surface_det_euler_mixed.npz                          one boomerang + two shells (a = 0.25), 3 steps: two body shapes
  g15_free_surface_operator.npz                                 multi_bodies.linear_operator_rigid applied to one fixed vector and
                                the per-blob product, on the start configuration of the 8 shells

Every deck: `mobility_vector_prod_implementation numba_free_surface`, `mobility_blobs_implementation python_no_wall`
(the blocks a reference deck can run above a free surface: its `C++_free_surface` names a function mobility.py does not
define), `domain single_wall`.  In every start configuration at least one blob sits below z = a, so the image's
overlapping-RPY branch (mobility_numba.py:1907-1915) is exercised; asserted here.

The trajectory fixtures have the format of the g9 ones (oracle/gen_golden_rigid_integrator.py: deck text, structure
arrays, start clones, saved trajectory, the driver's `.info` counters).  The reference runs unchanged, with the
accommodations of oracle/gen_golden_rigid_integrator.prepare (numba identity stub, empty `gmres` module, scipy's `tol`
keyword).

Usage:  python tools/gen_golden_free_surface.py [--ref /root/reference] [--out tests/golden] [--only NAME]
"""
import argparse
import glob
import os
import runpy
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_rigid_integrator as ggri  # noqa: E402

BLOCKS, PRODUCT, DOMAIN = "python_no_wall", "numba_free_surface", "single_wall"


def write_rows(path, rows):
  with open(path, "w") as fh:
    fh.write("%d\n" % len(rows))
    for x in rows:
      fh.write(" ".join("%.17g" % v for v in x) + "\n")


def blob_positions(bodies):
  """Blob coordinates of a list of (ID, vertex, locations, quaternions), through the reference's quaternion."""
  from quaternion_integrator.quaternion import Quaternion
  r = []
  for ID, vertex, loc, quat in bodies:
    for x, q in zip(loc, quat):
      R = Quaternion(np.array(q)).rotation_matrix()
      r.append(vertex @ R.T + x)
  return np.concatenate(r)


def check_start(bodies, a):
  z = blob_positions(bodies)[:, 2]
  assert z.min() > 0.0, "a blob below the surface: %g" % z.min()
  assert z.min() < a, "no blob below z = a (lowest %g, a = %g): the image's overlapping branch would not run" % (z.min(), a)
  return z.min()


def trajectory_case(ref, out_dir, name, scheme, bodies, n_steps, a, kT=0.0, dt=0.01, seed=1):
  t0 = time.time()
  lowest = check_start(bodies, a)
  work = tempfile.mkdtemp(prefix="ref_run_")
  data, lines = {}, []
  for ID, vertex, loc, quat in bodies:
    write_rows(os.path.join(work, ID + ".vertex"), vertex)
    write_rows(os.path.join(work, ID + ".clones"), np.hstack([loc, quat]))
    lines.append("structure %s.vertex %s.clones" % (ID, ID))
    data["vertex_" + ID], data["locations_" + ID], data["quaternions_" + ID] = np.asarray(vertex), np.asarray(loc), np.asarray(quat)
  deck = ggri.DECK.format(scheme=scheme, mobility_blobs=BLOCKS, mobility_vector_prod=PRODUCT, domain=DOMAIN, a=a, kT=kT, dt=dt,
                          n_steps=n_steps, update_PC=1, seed=seed, structures="\n".join(lines))
  with open(os.path.join(work, "deck.dat"), "w") as fh:
    fh.write(deck)
  cwd, argv = os.getcwd(), sys.argv
  os.chdir(work)
  try:
    sys.argv = ["multi_bodies.py", "--input-file", "deck.dat"]
    for m in [m for m in sys.modules if m.startswith("multi_bodies")]:      # (a fresh module namespace per run, as ggri.case)
      del sys.modules[m]
    runpy.run_path(os.path.join(ref, "multi_bodies", "multi_bodies.py"), run_name="__main__")
  finally:
    os.chdir(cwd)
    sys.argv = argv
  for ID in [b[0] for b in bodies]:
    files = sorted(glob.glob(os.path.join(work, "run.%s.*.clones" % ID)))
    assert len(files) == n_steps + 1, files
    traj = [ggri.read_clones(f) for f in files]
    data["trajectory_locations_" + ID] = np.array([t[0] for t in traj])
    data["trajectory_quaternions_" + ID] = np.array([t[1] for t in traj])
  with open(os.path.join(work, "run.info")) as fh:
    info = fh.read()
  np.savez_compressed(os.path.join(out_dir, name + ".npz"), deck=deck, IDs=np.array([b[0] for b in bodies]), scheme=scheme,
                      n_steps=n_steps, seed=seed, kT=kT, info=info, obstacles=np.array([], dtype=str), blob_radius=a,
                      lowest_blob=lowest, **data)
  shutil.rmtree(work)
  print("  %-40s %-30s steps=%d  lowest blob %.3f (a = %.3f)  %.1fs" % (name, scheme, n_steps, lowest, a, time.time() - t0), flush=True)


def operator_case(out_dir, name, bodies, a, eta):
  """multi_bodies.linear_operator_rigid with the free-surface product through the module's globals, one fixed vector."""
  import multi_bodies as MB
  from body import body
  from quaternion_integrator.quaternion import Quaternion
  t0 = time.time()
  lowest = check_start(bodies, a)
  (ID, vertex, loc, quat), = bodies
  objs = [body.Body(np.array(x), Quaternion(np.array(q)), vertex, a) for x, q in zip(loc, quat)]
  r = MB.get_blobs_r_vectors(objs, sum(b.Nblobs for b in objs))
  assert np.abs(r - blob_positions(bodies)).max() < 1e-14
  MB.mobility_vector_prod = MB.set_mobility_vector_prod(PRODUCT)
  n3 = r.size
  x = np.random.RandomState(1515).randn(n3 + 6 * len(objs))
  L = np.zeros(3)
  res = MB.linear_operator_rigid(x, objs, [], r, eta, a, periodic_length=L)
  product = MB.mobility_vector_prod(r, x[:n3], eta, a, periodic_length=L)
  np.savez_compressed(os.path.join(out_dir, name + ".npz"), vertex=vertex, locations=loc, quaternions=quat, blob_radius=a, eta=eta,
                      r_vectors=r, vector=x, operator=res, product=np.reshape(product, -1), lowest_blob=lowest)
  print("  %-40s %d blobs  lowest blob %.3f (a = %.3f)  %.1fs" % (name, len(r), lowest, a, time.time() - t0), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--ref", default="/root/reference")
  ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
  ap.add_argument("--only", default=None)
  args = ap.parse_args()
  out_dir = os.path.abspath(args.out)
  ggri.prepare(args.ref)
  S = os.path.join(args.ref, "multi_bodies", "Structures")
  from read_input import read_vertex_file     # the reference's own reader
  want = lambda name: args.only is None or args.only == name  # noqa: E731
  shell = read_vertex_file.read_vertex_file(os.path.join(S, "shell_N_12_Rg_0_7921_Rh_1.vertex"))[:, :3]
  a_shell = 0.41642
  rng = np.random.RandomState(1500)
  # 8 shells on a 3 x 3 grid (one site empty), centres at height 1.0 +- 0.05: the lowest blobs sit near z = 0.21 .. 0.4
  loc = np.array([[2.4 * (k % 3) + 0.1 * rng.rand(), 2.4 * (k // 3) + 0.1 * rng.rand(), 1.0 + 0.1 * (rng.rand() - 0.5)] for k in range(8)])
  shells = [("shell", shell, loc, ggri.random_quaternions(rng, 8))]
  kT = 0.0041
  if want("g15_free_surface_operator"):
    operator_case(out_dir, "g15_free_surface_operator", shells, a_shell, 1.1)
  for name, scheme, n_steps, kw in (("g15_free_surface_det_euler_shells", "deterministic_forward_euler", 4, {}),
                                    ("g15_free_surface_det_ab_shells", "deterministic_adams_bashforth", 4, {}),
                                    ("g15_free_surface_slip_trapz_shells", "stochastic_Slip_Trapz", 3, dict(kT=kT, seed=15))):
    if want(name):
      trajectory_case(args.ref, out_dir, name, scheme, shells, n_steps, a_shell, **kw)
  # two body shapes: one boomerang + two of the small shells of the g9 fixtures (one blob radius for both)
  boomerang = read_vertex_file.read_vertex_file(os.path.join(S, "boomerang_N_15.vertex"))[:, :3]
  small = read_vertex_file.read_vertex_file(os.path.join(S, "shell_N_12_Rg_0.3960_Rh_0.5.vertex"))[:, :3]
  mixed = [("boomerang", boomerang, np.array([[0.0, 0.0, 2.2]]), ggri.random_quaternions(rng, 1)),
           ("shell", small, np.array([[2.6, 0.3, 0.55], [0.4, 2.7, 0.6]]), ggri.random_quaternions(rng, 2))]
  if want("g15_free_surface_det_euler_mixed"):
    trajectory_case(args.ref, out_dir, "g15_free_surface_det_euler_mixed", "deterministic_forward_euler", mixed, 3, 0.25)


if __name__ == "__main__":
  main()
