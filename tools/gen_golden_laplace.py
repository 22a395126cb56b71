"""Golden data of phoretic bodies from the reference's OWN code.  Build-container only (needs the reference tree).

Writes, under tests/golden/:
  g12_laplace_operators.npz     the six operators of Laplace_kernels/Laplace_kernels_numba.py on a cloud of 200 nodes
                                above the wall (random fields, weights, unit normals), wall = 0 and wall = 1; the
                                source -> target pair has one target that coincides with a source
  g12_laplace_slip_*.npz        multi_bodies.calc_slip at one configuration: slip, concentration, GMRES iterations
                                (the solve is observed through a counting wrapper around utils.gmres)
  g13_phoretic_*.npz            trajectories of multi_bodies.py on decks with .Laplace files, the format of the g9
                                fixtures (oracle/gen_golden_rigid_integrator.py) plus the .Laplace array per structure

The reference runs unchanged, with the accommodations of oracle/gen_golden_rigid_integrator.prepare (numba identity
stub, empty `gmres` module, scipy's `tol` keyword).  The Janus shell's .Laplace data is written here.

Usage:  python tools/gen_golden_laplace.py [--ref /root/reference] [--out tests/golden] [--only NAME]
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

DECK = """scheme                                   {scheme}
mobility_blobs_implementation            {impl}
mobility_vector_prod_implementation      {impl}
blob_blob_force_implementation           None
body_body_force_torque_implementation    None
domain                                   {domain}
eta                                      {eta}
blob_radius                              {a}
g                                        {g}
kT                                       {kT}
solver_tolerance                         1e-10
rf_delta                                 1e-3
repulsion_strength_wall                  {rep_wall}
debye_length_wall                        0.2
dt                                       {dt}
n_steps                                  {n_steps}
n_save                                   1
seed                                     {seed}
background_Laplace                       {background}
diffusion_coefficient                    {Dc}
save_clones                              one_file_per_step
output_name                              run
{structures}
"""


def janus_laplace(vertex, front=(0.5, 1.0, 1.0), back=(0.2, 0.0, 0.5), radius=1.0):
  """(n, 7) .Laplace rows of a Janus shell (the layout of examples/Laplace_sphere/create_laplace_file_janus_sphere.py):
  radial normals, (reaction rate, emitting rate, surface mobility) = front for z > 0 else back, equal weights
  4 pi radius^2 / n."""
  n = len(vertex)
  normals = vertex / np.linalg.norm(vertex, axis=1)[:, None]
  rows = np.zeros((n, 7))
  rows[:, 0:3] = normals
  rows[:, 3:6] = np.where(vertex[:, 2:3] > 0, np.array(front)[None, :], np.array(back)[None, :])
  rows[:, 6] = 4 * np.pi * radius ** 2 / n
  return rows


def write_array(path, rows, header=None):
  with open(path, "w") as fh:
    if header is not None:
      fh.write(header)
    for x in rows:
      fh.write(" ".join("%.17g" % v for v in x) + "\n")


def operators(out_dir):
  from Laplace_kernels import Laplace_kernels_numba as LK
  rng = np.random.RandomState(1212)
  n = 200
  r = np.column_stack([6 * rng.rand(n), 6 * rng.rand(n), 0.5 + 2.5 * rng.rand(n)])
  nrm = rng.randn(n, 3)
  nrm /= np.linalg.norm(nrm, axis=1)[:, None]
  f = rng.randn(n)
  w = 0.2 + rng.rand(n)
  nt = 120
  tgt = np.column_stack([6 * rng.rand(nt), 6 * rng.rand(nt), 0.3 + 3 * rng.rand(nt)])
  tgt[17] = r[5]                       # coincides with a source: the source -> target operators skip that pair
  data = dict(r=r, normals=nrm, field=f, weights=w, target=tgt)
  for wall in (0, 1):
    data["single_layer_wall%d" % wall] = LK.Laplace_single_layer_operator_numba(r, f, w, wall=wall)
    data["double_layer_wall%d" % wall] = LK.Laplace_double_layer_operator_numba(r, f, w, nrm, wall=wall)
    data["deriv_double_layer_wall%d" % wall] = LK.Laplace_deriv_double_layer_operator_numba(r, f, w, nrm, wall=wall)
    data["dipole_wall%d" % wall] = LK.Laplace_dipole_operator_numba(r, f, w, wall=wall)
    data["single_layer_st_wall%d" % wall] = LK.Laplace_single_layer_operator_source_target_numba(r, tgt, f, w, wall=wall)
    data["double_layer_st_wall%d" % wall] = LK.Laplace_double_layer_operator_source_target_numba(r, tgt, f, w, nrm, wall=wall)
  np.savez_compressed(os.path.join(out_dir, "g12_laplace_operators.npz"), **data)
  print("  g12_laplace_operators", flush=True)


def slip_case(out_dir, name, vertex, laplace, locations, quaternions, a, domain, background, Dc, tol=1e-10):
  """multi_bodies.calc_slip through the module's globals, at one configuration."""
  import multi_bodies as MB
  from body import body
  from quaternion_integrator.quaternion import Quaternion
  t0 = time.time()
  bodies = []
  for loc, q in zip(locations, quaternions):
    b = body.Body(np.array(loc), Quaternion(np.array(q)), vertex, a)
    MB.multi_bodies_functions.set_slip_by_ID(b, None)
    b.normals = np.copy(laplace[:, 0:3])
    b.reaction_rate = np.copy(laplace[:, 3])
    b.emitting_rate = np.copy(laplace[:, 4])
    b.surface_mobility = np.copy(laplace[:, 5])
    b.weights = np.copy(laplace[:, 6])
    bodies.append(b)
  nblobs = sum(b.Nblobs for b in bodies)

  class Read(object):
    solver_tolerance = tol
  MB.read = Read()
  MB.background_Laplace = np.asarray(background, dtype=np.float64)
  MB.diffusion_coefficient = float(Dc)
  MB.print_residual = False
  seen = []
  original = MB.utils.gmres

  def counting_gmres(A, b, **kw):
    box = [0]
    cb = kw.get("callback")

    def count(rk=None):
      box[0] += 1
      if cb is not None:
        cb(rk)
    kw["callback"] = count
    x, info = original(A, b, **kw)
    seen.append((np.copy(x), box[0], info))
    return x, info
  MB.utils.gmres = counting_gmres
  try:
    slip = MB.calc_slip(bodies, nblobs, implementation="numba", blob_radius=a, eta=1.0, g=0.0, Laplace_flag=True,
                        domain=domain)
  finally:
    MB.utils.gmres = original
  assert len(seen) == 1 and seen[0][2] == 0, [s[1:] for s in seen]
  np.savez_compressed(os.path.join(out_dir, name + ".npz"), vertex=vertex, laplace=laplace, locations=np.asarray(locations),
                      quaternions=np.asarray(quaternions), blob_radius=a, domain=domain, background=np.asarray(background),
                      diffusion_coefficient=Dc, tolerance=tol, slip=slip, concentration=seen[0][0], iterations=seen[0][1])
  print("  %-40s iterations=%d  %.1fs" % (name, seen[0][1], time.time() - t0), flush=True)


def trajectory_case(ref, out_dir, name, scheme, ID, vertex, laplace, loc, quat, n_steps, a, domain, background="1", Dc=1.0,
                    kT=0.0, dt=0.01, seed=1, eta=1.0, g=0.0, rep_wall=0.0):
  """multi_bodies.py on a deck with one phoretic structure (vertex + clones + .Laplace); g9 fixture format + laplace_<ID>."""
  t0 = time.time()
  work = tempfile.mkdtemp(prefix="ref_run_")
  write_array(os.path.join(work, ID + ".vertex"), vertex, "%d\n" % len(vertex))
  write_array(os.path.join(work, ID + ".clones"), np.hstack([loc, quat]), "%d\n" % len(loc))
  write_array(os.path.join(work, ID + ".Laplace"), laplace, "# Columns: normals, reaction rate, emitting rate, surface mobility, weights\n")
  wall = domain == "single_wall"
  deck = DECK.format(scheme=scheme, impl="python" if wall else "python_no_wall", domain=domain, eta=eta, a=a, g=g, kT=kT,
                     rep_wall=rep_wall, dt=dt, n_steps=n_steps, seed=seed, background=background, Dc=Dc,
                     structures="structure %s.vertex %s.clones %s.Laplace" % (ID, ID, ID))
  with open(os.path.join(work, "deck.dat"), "w") as fh:
    fh.write(deck)
  cwd, argv = os.getcwd(), sys.argv
  os.chdir(work)
  try:
    sys.argv = ["multi_bodies.py", "--input-file", "deck.dat"]
    for m in [m for m in sys.modules if m.startswith("multi_bodies")]:
      del sys.modules[m]
    runpy.run_path(os.path.join(ref, "multi_bodies", "multi_bodies.py"), run_name="__main__")
  finally:
    os.chdir(cwd)
    sys.argv = argv
  files = sorted(glob.glob(os.path.join(work, "run.%s.*.clones" % ID)))
  assert len(files) == n_steps + 1, files
  traj = [ggri.read_clones(f) for f in files]
  with open(os.path.join(work, "run.info")) as fh:
    info = fh.read()
  np.savez_compressed(os.path.join(out_dir, name + ".npz"), deck=deck, IDs=np.array([ID]), scheme=scheme, n_steps=n_steps,
                      seed=seed, kT=kT, info=info, obstacles=np.array([], dtype=str), **{
                          "vertex_" + ID: np.asarray(vertex), "locations_" + ID: np.asarray(loc),
                          "quaternions_" + ID: np.asarray(quat), "laplace_" + ID: np.asarray(laplace),
                          "trajectory_locations_" + ID: np.array([t[0] for t in traj]),
                          "trajectory_quaternions_" + ID: np.array([t[1] for t in traj])})
  shutil.rmtree(work)
  print("  %-40s %-30s steps=%d  %.1fs" % (name, scheme, n_steps, time.time() - t0), flush=True)


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
  if want("g12_laplace_operators"):
    operators(out_dir)
  sprinkler = read_vertex_file.read_vertex_file(os.path.join(S, "sprinkler_N_72_La_5_00_Lb_5_00_W_1_00.vertex"))[:, :3]
  sprinkler_lap = np.loadtxt(os.path.join(S, "sprinkler_N_72_La_5_00_Lb_5_00_W_1_00_k_0_00_alpha_1_00_surf_mob_1_00.Laplace"))
  sp_clones = np.loadtxt(os.path.join(S, "two_sprinklers.clones"), skiprows=1)
  sp_loc, sp_quat = sp_clones[:, 0:3], sp_clones[:, 3:7]
  shell = read_vertex_file.read_vertex_file(os.path.join(S, "shell_N_42_Rg_0_8913_Rh_1.vertex"))[:, :3]
  janus = janus_laplace(shell)
  a_shell = 0.243553056072          # examples/Laplace_sphere/inputfile.dat
  rng = np.random.RandomState(1313)
  full_bg = np.array([1.0, 0.2, -0.1, 0.05, 0.02, 0.01, -0.03, 0.015, 0.01])
  # the two sprinklers of examples/chiral_phoretic_particle, lifted above the wall for the wall case and turned a little
  sp_loc_wall = sp_loc + np.array([0.0, 0.0, 6.0])
  sp_quat_turned = ggri.random_quaternions(rng, 2) * 0.15 + sp_quat
  sp_quat_turned /= np.linalg.norm(sp_quat_turned, axis=1)[:, None]
  if want("g12_laplace_slip_sprinklers_no_wall"):
    slip_case(out_dir, "g12_laplace_slip_sprinklers_no_wall", sprinkler, sprinkler_lap, sp_loc, sp_quat_turned, 0.5, "no_wall",
              np.array([1.0] + [0.0] * 8), 1.0)
  if want("g12_laplace_slip_sprinklers_wall"):
    slip_case(out_dir, "g12_laplace_slip_sprinklers_wall", sprinkler, sprinkler_lap, sp_loc_wall, sp_quat_turned, 0.5,
              "single_wall", np.array([1.0] + [0.0] * 8), 1.0)
  if want("g12_laplace_slip_janus_wall"):
    slip_case(out_dir, "g12_laplace_slip_janus_wall", shell, janus, np.array([[0.3, -0.2, 1.6]]), ggri.random_quaternions(rng, 1),
              a_shell, "single_wall", full_bg, 0.7)
  # trajectories
  if want("g13_phoretic_chiral_det_euler"):
    trajectory_case(args.ref, out_dir, "g13_phoretic_chiral_det_euler", "deterministic_forward_euler", "sprinkler", sprinkler,
                    sprinkler_lap, sp_loc, sp_quat, 2, 0.5, "no_wall", dt=0.01)
  shells_loc = np.array([[0.0, 0.0, 1.7], [2.6, 0.3, 1.9], [0.4, 2.7, 1.8]])
  shells_quat = ggri.random_quaternions(rng, 3)
  if want("g13_phoretic_janus_wall_det_ab"):
    trajectory_case(args.ref, out_dir, "g13_phoretic_janus_wall_det_ab", "deterministic_adams_bashforth", "janus", shell, janus,
                    shells_loc, shells_quat, 3, a_shell, "single_wall", background=" ".join("%.17g" % v for v in full_bg),
                    Dc=0.8, dt=0.02, g=0.3, rep_wall=0.5)
  if want("g13_phoretic_janus_wall_slip_trapz"):
    trajectory_case(args.ref, out_dir, "g13_phoretic_janus_wall_slip_trapz", "stochastic_Slip_Trapz", "janus", shell, janus,
                    shells_loc[:2], shells_quat[:2], 2, a_shell, "single_wall", background="1 0.1", Dc=1.0, dt=0.01,
                    kT=0.05, seed=17, g=0.3, rep_wall=0.5)


if __name__ == "__main__":
  main()
