"""Metropolis sampler of rigid-body configurations -- many_bodyMCMC/many_body_MCMC.py on MI355X.

    python -m rigidmultiblobswall_amd.mcmc [inputfile] [--device N] [--potential soft|yukawa] [--rng reference|batched]
                                           [--moves all|single] [--body-potential none|deck|EPS,B] [--gr RMAX,BINS]
                                           [--pair-table FILE]

Same decks, same outputs (.inputfile, .random_state, .clones per saved step or one appended .config, .time, .MCMC_info)
and, with rng="reference", the same chain as the reference script for the same seed: the draws come from a
numpy.random.RandomState in the reference's call order (per free body uniform(3) then normal(3); one uniform per step).
The legacy generator caches a Gaussian between calls, so that interleaving cannot be vectorised and the per-body loop of
draws stays on the host; rng="batched" draws one (n, 3) uniform and one (n, 3) normal block per step -- the same
distribution on another stream, for large decks.

State on the device: body locations, quaternions and the structures' reference configurations.  Per step the host
uploads one (n_bodies, 6) array of draws, one launch composes the proposal and writes the proposed blob coordinates
(rmb_mcmc_propose_device), the energy sweep runs (rmb_blob_potential), one pair of doubles comes back; an accepted
proposal becomes current by swapping the two sets of tensors.

`moves="single"` (beyond the reference, which moves every free body in one proposal): one step of the deck is one SWEEP of
single-body moves over the free bodies in index order.  Per sweep the host draws, per free body, uniform(-t, t, 3),
normal(0, 1, 3) and uniform(0, 1) (rng="batched": the three blocks (n, 3), (n, 3), (n,)) and uploads them once as (n_free, 7);
rmb_mcmc_sweep_device then runs two launches per body -- proposal + energy difference of that body in O(n_body N), decision +
commit in place -- without a host synchronisation in between, and the host reads the flags and the running energy.  The
acceptance recursion is applied once per flag, the +-2 % rule once per step; at every save the full energy is recomputed
(energy_drift) and the running value reset to it.

`body_potential=(eps, b)` (beyond the reference, whose body potentials are empty): the energy gains the Yukawa repulsion
between body locations, U_body = sum_{i<j} eps exp(-r_ij/b) / r_ij in the minimal image of every periodic direction -- the
energy of the steppers' body-body forces, so that the chain samples what a Brownian deck with
`body_body_force_torque_implementation python|hip` relaxes to; "deck" takes the two numbers the steppers would take from
this deck.  The locations are the resident points of a second context: moves="all" adds rmb_body_body_potential of the
proposed locations to every proposal's energy, moves="single" runs rmb_mcmc_sweep_bb_device with a running energy of three
doubles.  None (the default) is the reference's sampler: the deck option is ignored.

`gr=(r_max, n_bins)` (beyond the reference, which post-processes its `.config` with gr_pseudo2D_single_blob.cpp): at every
saved step the body locations, already on the device, go through the batch entry of the HIP pair-distance histogram
(rmb_pair_histogram_frames_device, one frame; the resident configuration of the energy sweeps is not touched), and at the end
`<output_name>.gr.dat` holds `r g hist` in that program's format (correlation.py; normalisation "3d" when all three periods are
positive, else "pseudo2d").  With an energy= function the locations are uploaded for it.  Off by default; off, nothing the
sampler does or writes changes.

`MCMCSampler(..., energy=f)` runs the same chain with f(r_vectors) -> float as the energy and numpy state instead (the
host tests replay the reference's fixtures with the numpy restatement that way); without it the energy is the HIP one --
there is no silent fall-back in either direction.
"""
import argparse
import os
import shutil
import sys
import time

import numpy as np

from .read_input import ReadInput
from .structures import read_clones_file, read_vertex_file

USER_POTENTIAL_FILE = "potential_pycuda_user_defined.py"


class UserDefinedPotentialError(RuntimeError):
  pass


def refuse_user_defined_potential(directory="."):
  """The reference swaps its potential module for `potential_pycuda_user_defined.py` when that file lies in the working
  directory (many_body_MCMC.py:35-43).  A CUDA string cannot run here, and sampling another potential without saying so
  is the one thing a sampler must not do."""
  path = os.path.join(directory, USER_POTENTIAL_FILE)
  if os.path.isfile(path):
    raise UserDefinedPotentialError(
        "%s found: CUDA-string potentials are not supported by the HIP sampler.  The Yukawa potential of the reference's "
        "boomerang_suspension example is built in: run with --potential yukawa (MCMCSampler(potential='yukawa')) from a "
        "directory without that file; any other radial pair potential runs as a table: --pair-table FILE "
        "(MCMCSampler(pair_table=PairTable...), pair_table.py); any other user-defined potential is not implemented." % path)


def body_length(reference_configuration, blob_radius):
  """Body.calc_body_length (body/body.py:218-231): the furthest blob pair plus 2a."""
  r = np.asarray(reference_configuration, dtype=np.float64)[:, :3]
  d = np.linalg.norm(r[:, None, :] - r[None, :, :], axis=-1)
  return float(d.max()) + 2.0 * blob_radius


def rotation_matrices(quat):
  """(n, 3, 3) rotation matrices of unit quaternions (s, p) (quaternion.py:42-51)."""
  s, p = quat[:, 0], quat[:, 1:]
  diag = s * s - 0.5
  R = p[:, :, None] * p[:, None, :]
  R[:, 0, 0] += diag; R[:, 1, 1] += diag; R[:, 2, 2] += diag
  R[:, 0, 1] -= s * p[:, 2]; R[:, 0, 2] += s * p[:, 1]
  R[:, 1, 0] += s * p[:, 2]; R[:, 1, 2] -= s * p[:, 0]
  R[:, 2, 0] -= s * p[:, 1]; R[:, 2, 1] += s * p[:, 0]
  return 2.0 * R


def body_body_energy(loc, periodic_length, repulsion_strength, debye_length):
  """numpy twin of rmb_body_body_potential: sum_{i<j} eps exp(-r/b) / r between the rows of loc, minimal image in every
  direction with a positive period (project_to_periodic_image: the image count is truncated after adding half away from
  zero)."""
  x = np.asarray(loc, dtype=np.float64).reshape(-1, 3)
  i, j = np.triu_indices(len(x), 1)
  d = x[j] - x[i]
  for k in range(3):
    Lk = float(periodic_length[k])
    if Lk > 0:
      d[:, k] -= np.trunc(d[:, k] / Lk + 0.5 * np.sign(d[:, k])) * Lk
  r = np.sqrt(np.sum(d * d, axis=1))
  with np.errstate(divide="ignore", invalid="ignore"):
    return float(np.sum(repulsion_strength * np.exp(-r / debye_length) / r))


def resolve_body_potential(body_potential, read):
  """None, or (eps, b) as two floats: a tuple as given, "deck" = the law the steppers apply to this deck."""
  if body_potential is None:
    return None
  if isinstance(body_potential, str):
    if body_potential != "deck":
      raise ValueError("body_potential must be None, 'deck' or (repulsion_strength, debye_length), got %r" % (body_potential,))
    if read.body_body_force_torque_implementation not in ("python", "hip"):
      raise ValueError("body_potential='deck': the deck does not switch body-body forces on "
                       "(body_body_force_torque_implementation %s; python or hip)" % (read.body_body_force_torque_implementation,))
    body_potential = (read.repulsion_strength, read.debye_length)
  try:
    eps, b = (float(x) for x in body_potential)
  except (TypeError, ValueError):
    raise ValueError("body_potential must be None, 'deck' or (repulsion_strength, debye_length), got %r" % (body_potential,))
  if not b > 0.0:
    raise ValueError("body_potential: debye_length must be positive, got %r" % (b,))
  return eps, b


def compose_proposal(loc, quat, draws, n_free, max_angle_shift):
  """numpy twin of rmb_mcmc_propose_device's first half: (loc_new, quat_new)."""
  loc_new, quat_new = loc.copy(), quat.copy()
  if n_free:
    loc_new[:n_free] += draws[:n_free, 0:3]
    phi = draws[:n_free, 3:6] * max_angle_shift
    nrm = np.linalg.norm(phi, axis=1)
    qs = np.cos(0.5 * nrm)
    with np.errstate(invalid="ignore", divide="ignore"):
      qp = np.where(nrm[:, None] != 0, np.sin(0.5 * nrm)[:, None] * (phi / nrm[:, None]), 0.0)
    s, p = quat[:n_free, 0], quat[:n_free, 1:]
    quat_new[:n_free, 0] = qs * s - np.einsum("ij,ij->i", qp, p)
    quat_new[:n_free, 1:] = qs[:, None] * p + s[:, None] * qp + np.cross(qp, p)
  return loc_new, quat_new


class _HostState(object):
  """Bodies as numpy arrays; the energy is the caller's function of the blob coordinates."""

  def __init__(self, sampler, energy):
    self.s, self.energy_fn = sampler, energy
    self.loc, self.quat = sampler.loc0.copy(), sampler.quat0.copy()
    self.running, self.decision_margin = None, np.inf      # moves="single"
    self.gr_ctx = None      # context of the g(r) hook, made on first use

  def _blobs(self, loc, quat):
    s = self.s
    R = rotation_matrices(quat)
    return np.einsum("bij,bj->bi", R[s.blob_body], s.ref_all[s.blob_ref]) + loc[s.blob_body]

  def _total(self, loc, quat):
    """The caller's energy of the blob coordinates, plus the body-body term of the locations when it is on."""
    e = self.energy_fn(self._blobs(loc, quat))
    law = self.s.body_potential
    if law is not None:
      e = e + body_body_energy(loc, self.s.periodic_length, law[0], law[1])
    return e

  def current_energy(self):
    return self._total(self.loc, self.quat)

  def propose(self, draws, max_angle_shift):
    self.loc_new, self.quat_new = compose_proposal(self.loc, self.quat, draws, self.s.n_free, max_angle_shift)
    return self._total(self.loc_new, self.quat_new)

  def accept(self):
    self.loc, self.quat = self.loc_new, self.quat_new

  def sweep(self, draws, max_angle_shift):
    """One sweep of single-body moves: dE = energy(new) - energy(old) with the caller's function, decided as the all-body
    step is.  -> (flags, energy after the sweep); decision_margin keeps the smallest |u - exp(-dE/kT)| of the run."""
    kT = np.float64(self.s.kT)
    if self.running is None:
      self.running = np.float64(self.current_energy())
    flags = []
    for k in range(self.s.n_free):
      loc_k, quat_k = compose_proposal(self.loc[k:k + 1], self.quat[k:k + 1], draws[k:k + 1, 0:6], 1, max_angle_shift)
      loc_new, quat_new = self.loc.copy(), self.quat.copy()
      loc_new[k], quat_new[k] = loc_k[0], quat_k[0]
      sample = np.float64(self._total(loc_new, quat_new))
      with np.errstate(over="ignore", invalid="ignore"):
        bound = np.exp(-(sample - self.running) / kT)
        ok = bool(draws[k, 6] < bound)
        margin = abs(draws[k, 6] - bound)
      if margin < self.decision_margin:        # a NaN bound compares false: it rejects, and no rounding changes that
        self.decision_margin = float(margin)
      flags.append(ok)
      if ok:
        self.loc, self.quat, self.running = loc_new, quat_new, sample
    return flags, float(self.running)

  def recompute_energy(self):
    """The full energy of the current configuration; the running value becomes it.  -> (running before, full)"""
    before = self.running
    self.running = np.float64(self.current_energy())
    return float(self.running if before is None else before), float(self.running)

  def configuration(self):
    return self.loc, self.quat

  def gr_add(self, r_max, n_bins, hist):
    """The pair histogram of the current locations added to hist (CUDA int64 tensor): an upload, then the batch entry."""
    import torch
    if self.gr_ctx is None:
      from .context import MobilityContext
      self.gr_ctx = MobilityContext(hist.device.index)
    with torch.cuda.device(hist.device):
      frame = torch.from_numpy(np.ascontiguousarray(self.loc, dtype=np.float64).reshape(1, -1, 3)).to(hist.device)
      self.gr_ctx.pair_histogram_frames_device(frame, self.s.periodic_length, r_max, n_bins, out=hist)

  def close(self):
    if self.gr_ctx is not None:
      self.gr_ctx.close()
      self.gr_ctx = None


class _DeviceState(object):
  """Bodies as CUDA tensors; proposal and energy are HIP launches on one context.  With a body potential a second context
  on the same device holds the body locations as its resident points (the blob view stays where it is)."""

  def __init__(self, sampler, device):
    import torch
    from .context import MobilityContext
    self.torch, self.s = torch, sampler
    self.dev = torch.device("cuda", int(device))
    self.ctx = MobilityContext(int(device))
    self.law = sampler.body_potential
    self.body_ctx = MobilityContext(int(device)) if self.law is not None else None
    self.u_body = torch.zeros(1, dtype=torch.float64, device=self.dev)
    t = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(self.dev)   # noqa: E731
    self.loc, self.quat = t(sampler.loc0), t(sampler.quat0)
    self.loc_new, self.quat_new = torch.empty_like(self.loc), torch.empty_like(self.quat)
    self.ref = t(sampler.ref_all)
    self.blob_body, self.blob_ref = t(sampler.blob_body, torch.int32), t(sampler.blob_ref, torch.int32)
    self.r_new = torch.empty((sampler.n_blobs, 3), dtype=torch.float64, device=self.dev)
    self.draws_host = torch.zeros((sampler.n_bodies, 6), dtype=torch.float64).pin_memory()
    self.draws = torch.zeros((sampler.n_bodies, 6), dtype=torch.float64, device=self.dev)
    if sampler.moves == "single":
      # r_new holds the CURRENT blob coordinates between sweeps: the finishing launch of an accepted move rewrites its rows
      self.body_first = np.ascontiguousarray(sampler.body_first, dtype=np.int64)
      self.draws7_host = torch.zeros((max(sampler.n_free, 1), 7), dtype=torch.float64).pin_memory()
      self.draws7 = torch.zeros((max(sampler.n_free, 1), 7), dtype=torch.float64, device=self.dev)
      # running {U_one, U_pair}, with a body potential {U_one, U_pair, U_body}
      self.energy = torch.zeros(2 if self.law is None else 3, dtype=torch.float64, device=self.dev)
      self.flags = torch.zeros(max(sampler.n_free, 1), dtype=torch.int32, device=self.dev)

  def _energy_terms(self, out=None):
    s = self.s
    with self.torch.cuda.device(self.dev):
      self.ctx.set_positions(self.r_new, s.blob_radius, s.periodic_length, wall=False)
      return self.ctx.blob_potential_device(s.repulsion_strength, s.debye_length, s.blob_radius,
                                            repulsion_strength_wall=s.repulsion_strength_wall, debye_length_wall=s.debye_length_wall,
                                            weight=s.weight, potential=s.potential, out=out, pair_table=s.pair_table)

  def _body_energy(self, loc, out):
    """U_body of the locations `loc` into out (one entry): the energy sweep on the second context."""
    s = self.s
    with self.torch.cuda.device(self.dev):
      self.body_ctx.set_positions(loc, s.blob_radius, s.periodic_length, wall=False)
      return self.body_ctx.body_body_potential_device(self.law[0], self.law[1], out=out)

  def recompute_energy(self):
    """The full energy of the current coordinates (the energy sweeps); the running sums on the device become it.
    -> (running before, full)"""
    before = float(self.energy.sum().item())
    self._energy_terms(out=self.energy[:2])
    if self.law is not None:
      self._body_energy(self.loc, self.energy[2:])
    return before, float(self.energy.sum().item())

  def sweep(self, draws, max_angle_shift):
    """One sweep of single-body moves (rmb_mcmc_sweep_device).  -> (flags, running energy after the sweep)"""
    s = self.s
    if s.n_free == 0:
      return [], float(self.energy.sum().item())
    self.draws7_host.numpy()[...] = draws[:s.n_free]
    self.draws7.copy_(self.draws7_host, non_blocking=True)
    with self.torch.cuda.device(self.dev):
      self.ctx.mcmc_sweep_device(self.body_first, self.blob_ref, self.ref, self.loc, self.quat, self.r_new, self.draws7, s.n_free,
                                 max_angle_shift, s.periodic_length, s.kT, self.energy, self.flags, s.repulsion_strength, s.debye_length,
                                 s.blob_radius, repulsion_strength_wall=s.repulsion_strength_wall, debye_length_wall=s.debye_length_wall,
                                 weight=s.weight, potential=s.potential, body_potential=self.law)
    flags = self.flags[:s.n_free].cpu().numpy()
    return [bool(f) for f in flags], float(self.energy.sum().item())

  def _energy(self):
    s = self.s
    with self.torch.cuda.device(self.dev):
      self.ctx.set_positions(self.r_new, s.blob_radius, s.periodic_length, wall=False)
      u_one, u_pair = self.ctx.blob_potential(s.repulsion_strength, s.debye_length, s.blob_radius,
                                              repulsion_strength_wall=s.repulsion_strength_wall, debye_length_wall=s.debye_length_wall,
                                              weight=s.weight, potential=s.potential, pair_table=s.pair_table)
    if self.law is not None:      # of the proposed locations (current_energy proposes the current ones)
      return u_one + u_pair + float(self._body_energy(self.loc_new, self.u_body).item())
    return u_one + u_pair

  def _propose(self, loc, quat, n_free, max_angle_shift):
    with self.torch.cuda.device(self.dev):
      self.ctx.mcmc_propose_device(self.blob_body, self.blob_ref, self.ref, loc, quat, self.draws, n_free, max_angle_shift,
                                   self.loc_new, self.quat_new, self.r_new)

  def current_energy(self):
    self._propose(self.loc, self.quat, 0, 0.0)       # no free body: the current configuration's blob coordinates
    if self.s.moves == "single":
      return self.recompute_energy()[1]
    return self._energy()

  def upload(self, draws):
    self.draws_host.numpy()[...] = draws
    self.draws.copy_(self.draws_host, non_blocking=True)

  def compose(self, max_angle_shift):
    self._propose(self.loc, self.quat, self.s.n_free, max_angle_shift)

  def propose(self, draws, max_angle_shift):
    self.upload(draws)
    self.compose(max_angle_shift)
    return self._energy()

  def accept(self):      # the proposed state becomes current: a swap of handles, no copy
    self.loc, self.loc_new = self.loc_new, self.loc
    self.quat, self.quat_new = self.quat_new, self.quat

  def configuration(self):
    return self.loc.cpu().numpy(), self.quat.cpu().numpy()

  def gr_add(self, r_max, n_bins, hist):
    """The pair histogram of the current locations added to hist (CUDA int64 tensor): the batch entry on the locations where
    they are; neither context's resident configuration is involved."""
    with self.torch.cuda.device(self.dev):
      self.ctx.pair_histogram_frames_device(self.loc.view(1, -1, 3), self.s.periodic_length, r_max, n_bins, out=hist)

  def close(self):
    self.ctx.close()
    if self.body_ctx is not None:
      self.body_ctx.close()


class MCMCSampler(object):
  """many_body_MCMC.py:100-304.  `read`: a ReadInput (or the path of a deck).  After run(): energy_log (the start energy,
  then every proposal's), accepted (one bool per step), accepted_moves, max_translation, max_angle_shift, and -- with
  keep_saved (default: only when no files are written) -- saved: step -> (locations, quaternions) of every save.
  moves="single": a step is one sweep of single-body moves over the free bodies; accepted holds one bool per MOVE,
  accepted_moves counts moves, energy_log the start energy and the running energy after every sweep, energy_drift: step ->
  (running energy, recomputed full energy) of every save."""

  def __init__(self, read, device=0, potential="soft", rng="reference", energy=None, write_files=True, verbose=False,
               check_user_potential=True, keep_saved=None, moves="all", body_potential=None, gr=None, pair_table=None):
    if check_user_potential:
      refuse_user_defined_potential(".")
    if potential not in ("soft", "yukawa"):
      raise ValueError("potential must be 'soft' or 'yukawa', got %r" % (potential,))
    if rng not in ("reference", "batched"):
      raise ValueError("rng must be 'reference' or 'batched', got %r" % (rng,))
    if moves not in ("all", "single"):
      raise ValueError("moves must be 'all' or 'single', got %r" % (moves,))
    if moves == "single" and energy is None and not isinstance(device, (int, np.integer)):
      raise ValueError("moves='single' takes a device index, not %r" % (device,))
    self.moves = moves
    # a user-defined radial pair law (pair_table.PairTable, or the path of its file): replaces the pair term of `potential`,
    # whose one-blob form stays; moves="all" only
    if isinstance(pair_table, str):
      from .pair_table import PairTable
      pair_table = PairTable.load(pair_table)
    if pair_table is not None:
      from .pair_table import PairTable
      if not isinstance(pair_table, PairTable):
        raise ValueError("pair_table must be a PairTable or the path of its file, got %r" % (type(pair_table).__name__,))
      if moves == "single":
        raise ValueError("moves='single' does not serve a pair table: the single-body energy difference has no table variant; use moves='all'")
      if energy is not None:
        raise ValueError("pair_table goes with the HIP energy; a caller's energy= function is the whole potential")
    self.pair_table = pair_table
    self.gr = None
    if gr is not None:
      try:
        r_max, n_bins = gr
        self.gr = (float(r_max), int(n_bins))
      except (TypeError, ValueError):
        raise ValueError("gr must be None or (r_max, n_bins), got %r" % (gr,))
      if not self.gr[0] > 0.0 or not 1 <= self.gr[1] <= 8192 or self.gr[1] != n_bins:
        raise ValueError("gr: r_max must be positive and n_bins an integer 1 ... 8192, got %r" % (gr,))
      if not isinstance(device, (int, np.integer)):
        raise ValueError("gr takes a device index, not %r" % (device,))
    self.device = device
    self.read = read = ReadInput(read) if isinstance(read, str) else read
    self.potential, self.rng_mode, self.write_files, self.verbose = potential, rng, write_files, verbose
    if read.n_steps <= read.initial_step:
      raise ValueError("n_steps (%d) must exceed initial_step (%d)" % (read.n_steps, read.initial_step))
    if read.save_clones not in ("one_file_per_step", "one_file"):
      raise ValueError("save_clones = %s is not implemented: use one_file_per_step or one_file" % read.save_clones)
    self.blob_radius = float(read.blob_radius)
    self.periodic_length = np.asarray(read.periodic_length, dtype=np.float64)
    self.weight = 1.0 * read.g
    self.kT = read.kT
    self.repulsion_strength, self.debye_length = read.repulsion_strength, read.debye_length
    # None: the reference's sampler (the deck's body-body option is ignored); (eps, b): the Yukawa energy between locations
    self.body_potential = resolve_body_potential(body_potential, read)
    self.repulsion_strength_wall, self.debye_length_wall = read.repulsion_strength_wall, read.debye_length_wall
    # bodies, structure after structure (many_body_MCMC.py:107-125)
    refs, locs, quats, blob_body, blob_ref = [], [], [], [], []
    self.body_types, n_free, max_len, row0, body0 = [], 0, 0.0, 0, 0
    for k, structure in enumerate(read.structures):
      ref = read_vertex_file(read.resolve(structure[0]))[:, :3]
      nb, loc, quat = read_clones_file(read.resolve(structure[1]))
      self.body_types.append(nb)
      if nb > 0:
        max_len = max(max_len, body_length(ref, self.blob_radius))
      if k < read.num_free_bodies:
        n_free += nb
      refs.append(ref); locs.append(loc); quats.append(quat)
      blob_body.append(np.repeat(body0 + np.arange(nb), len(ref)))
      blob_ref.append(np.tile(row0 + np.arange(len(ref)), nb))
      row0 += len(ref); body0 += nb
    self.ref_all = np.concatenate(refs) if refs else np.zeros((0, 3))
    self.loc0 = np.concatenate(locs).reshape(-1, 3)
    self.quat0 = np.concatenate(quats).reshape(-1, 4)
    self.blob_body = np.concatenate(blob_body).astype(np.int64)
    self.blob_ref = np.concatenate(blob_ref).astype(np.int64)
    # body k owns the blobs [body_first[k], body_first[k + 1])
    self.body_first = np.concatenate([[0], np.cumsum(np.bincount(self.blob_body, minlength=body0))]).astype(np.int64)
    self.n_bodies, self.n_free, self.n_blobs = body0, n_free, self.blob_body.size
    self.max_body_length = max_len
    self.max_translation = self.blob_radius * 0.1
    self.max_angle_shift = self.max_translation / self.max_body_length
    self.accepted_moves, self.acceptance_ratio = 0, 0.5
    self.energy_log, self.accepted, self.saved, self.energy_drift = [], [], {}, {}
    # saved configurations stay in memory only when asked for, or when no file receives them
    self.keep_saved = (not write_files) if keep_saved is None else bool(keep_saved)
    self.draw_seconds = 0.0
    self.gr_frames, self._gr_hist = 0, None
    if self.gr is not None:      # refuses a box the normalisation cannot serve before anything runs
      from . import correlation
      self.gr_normalisation = "3d" if np.all(self.periodic_length > 0) else "pseudo2d"
      correlation.normalise(np.zeros(1), 1, max(self.n_bodies, 1), self.periodic_length, self.gr[0], self.gr_normalisation)
    self.state = _HostState(self, energy) if energy is not None else _DeviceState(self, device)

  def close(self):
    self.state.close()

  # ---- draws -------------------------------------------------------------------------------------------------------------
  def _draws(self, rng):
    d = np.zeros((self.n_bodies, 6))
    t = self.max_translation
    if self.rng_mode == "reference":
      for k in range(self.n_free):          # the legacy generator caches a Gaussian: this order cannot be vectorised
        d[k, 0:3] = rng.uniform(-t, t, 3)
        d[k, 3:6] = rng.normal(0, 1, 3)
    else:
      d[:self.n_free, 0:3] = rng.uniform(-t, t, (self.n_free, 3))
      d[:self.n_free, 3:6] = rng.normal(0, 1, (self.n_free, 3))
    return d

  def _sweep_draws(self, rng):
    """(n_free, 7) of one sweep: displacement, rotation vector / max_angle_shift, the uniform of the decision."""
    d = np.zeros((self.n_free, 7))
    t = self.max_translation
    if self.rng_mode == "reference":
      for k in range(self.n_free):
        d[k, 0:3] = rng.uniform(-t, t, 3)
        d[k, 3:6] = rng.normal(0, 1, 3)
        d[k, 6] = rng.uniform(0.0, 1.0)
    else:
      d[:, 0:3] = rng.uniform(-t, t, (self.n_free, 3))
      d[:, 3:6] = rng.normal(0, 1, (self.n_free, 3))
      d[:, 6] = rng.uniform(0.0, 1.0, self.n_free)
    return d

  # ---- output ------------------------------------------------------------------------------------------------------------
  def _save(self, step):
    if self.moves == "single":      # the running energy against a full evaluation, which it then restarts from
      self.energy_drift[step] = self.state.recompute_energy()
    if self.gr is not None:
      self._gr_add()
    loc, quat = self.state.configuration()
    if self.keep_saved:
      self.saved[step] = (np.array(loc), np.array(quat))
    if not self.write_files:
      return
    read, offset = self.read, 0
    for i, ID in enumerate(read.structures_ID):
      if read.save_clones == "one_file_per_step":
        name, status = read.output_name + "." + ID + "." + str(step).zfill(8) + ".clones", "w"
      else:
        name, status = read.output_name + "." + ID + ".config", ("w" if step == 0 else "a")
      with open(name, status) as f:
        f.write(str(self.body_types[i]) + "\n")
        for j in range(self.body_types[i]):
          x, q = loc[offset + j], quat[offset + j]
          f.write("%s %s %s %s %s %s %s\n" % (float(x[0]), float(x[1]), float(x[2]), float(q[0]), float(q[1]), float(q[2]), float(q[3])))
      offset += self.body_types[i]

  # ---- g(r) of the saved configurations ------------------------------------------------------------------------------------
  def _gr_add(self):
    if self._gr_hist is None:
      import torch
      self._gr_hist = torch.zeros(self.gr[1], dtype=torch.int64, device=torch.device("cuda", int(self.device)))
    self.state.gr_add(self.gr[0], self.gr[1], self._gr_hist)
    self.gr_frames += 1

  @property
  def gr_counts(self):
    """unordered pairs per bin over the saved configurations so far (numpy uint64); None with gr off"""
    if self.gr is None:
      return None
    return np.zeros(self.gr[1], dtype=np.uint64) if self._gr_hist is None else self._gr_hist.cpu().numpy().astype(np.uint64)

  def gr_text(self):
    """`r g hist` of the saved configurations in the reference program's format"""
    from . import correlation
    counts = self.gr_counts
    r = (np.arange(self.gr[1]) + 0.5) * (self.gr[0] / self.gr[1])
    g = correlation.normalise(counts, max(self.gr_frames, 1), self.n_bodies, self.periodic_length, self.gr[0], self.gr_normalisation)
    return correlation.format_gr(r, g, counts)

  def info_lines(self, last_step):
    lines = self._info_lines(last_step)
    if self.body_potential is not None:
      lines.append("body_potential = yukawa repulsion_strength %s debye_length %s" % self.body_potential)
    return lines

  def _info_lines(self, last_step):
    if self.moves == "single":      # per move
      return ["acceptance ratio = " + str(self.accepted_moves / max(1.0, float(len(self.accepted)))),
              "accepted_moves = " + str(self.accepted_moves),
              "final max_translation = " + str(self.max_translation),
              "final max_angle_shift = " + str(self.max_angle_shift)]
    return ["acceptance ratio = " + str(self.accepted_moves / (last_step + 2.0 - self.read.initial_step)),
            "accepted_moves = " + str(self.accepted_moves),
            "final max_translation = " + str(self.max_translation),
            "final max_angle_shift = " + str(self.max_angle_shift)]

  # ---- the chain -----------------------------------------------------------------------------------------------------------
  def run(self, rng=None):
    read = self.read
    if self.write_files:
      shutil.copyfile(read.input_file, read.output_name + ".inputfile")
    if rng is None:
      rng = read.random_generator(save=self.write_files)
    start = time.time()
    current = np.float64(self.state.current_energy())
    self.energy_log.append(float(current))
    kT = np.float64(self.kT)
    step = read.initial_step
    for step in range(read.initial_step, read.n_steps):
      t0 = time.perf_counter()
      draws = self._sweep_draws(rng) if self.moves == "single" else self._draws(rng)
      self.draw_seconds += time.perf_counter() - t0
      if self.moves == "single":
        flags, running = self.state.sweep(draws, self.max_angle_shift)
        self.energy_log.append(running)
        for ok in flags:        # the recursion once per move, in move order
          self.accepted.append(ok)
          self.accepted_moves += int(ok)
          self.acceptance_ratio = self.acceptance_ratio * 0.95 + (0.05 if ok else 0.0)
      else:
        sample = np.float64(self.state.propose(draws, self.max_angle_shift))
        self.energy_log.append(float(sample))
        with np.errstate(over="ignore", invalid="ignore"):        # numpy's comparison: a NaN or inf energy rejects
          ok = bool(rng.uniform(0.0, 1.0) < np.exp(-(sample - current) / kT))
        self.accepted.append(ok)
        if ok:
          current = sample
          self.accepted_moves += 1
          self.acceptance_ratio = self.acceptance_ratio * 0.95 + 0.05
          self.state.accept()
        else:
          self.acceptance_ratio = self.acceptance_ratio * 0.95
      # step size: +-2 % during the first half of the negative steps
      if step < 0 and step < read.initial_step // 2:
        self.max_translation = self.max_translation * (1.02 if self.acceptance_ratio > 0.5 else 0.98)
        self.max_angle_shift = self.max_translation / self.max_body_length
      if (step % read.n_save) == 0 and step >= 0:
        if self.verbose:
          print("MCMC, step = ", step, ", wallclock time = ", time.time() - start, ", acceptance ratio = ",
                self.accepted_moves / ((step + 1.0 - read.initial_step) * (max(self.n_free, 1) if self.moves == "single" else 1)))
        self._save(step)
    if ((step + 1) % read.n_save) == 0 and step >= 0:         # the "final" save of the reference
      self._save(step + 1)
    self.last_step = step
    if self.verbose:
      if self.moves == "single":
        print("\n" + self.info_lines(step)[0])
      else:
        print("\nacceptance ratio = ", self.accepted_moves / (step + 2.0 - read.initial_step))
      print("accepted_moves = ", self.accepted_moves)
      print("Total time = ", time.time() - start)
    if self.write_files:
      with open(read.output_name + ".time", "w") as f:
        f.write(str(time.time() - start) + "\n")
      with open(read.output_name + ".MCMC_info", "w") as f:
        f.write("\n".join(self.info_lines(step)) + "\n")
      if self.gr is not None:
        with open(read.output_name + ".gr.dat", "w") as f:
          f.write(self.gr_text())
    return self


def main(argv=None):
  ap = argparse.ArgumentParser(prog="python -m rigidmultiblobswall_amd.mcmc", description=__doc__.split("\n\n")[0])
  ap.add_argument("inputfile", nargs="?", default="data.main")
  ap.add_argument("--device", type=int, default=0)
  ap.add_argument("--potential", choices=("soft", "yukawa"), default="soft")
  ap.add_argument("--rng", choices=("reference", "batched"), default="reference")
  ap.add_argument("--moves", choices=("all", "single"), default="all",
                  help="all: every free body in one proposal (the reference); single: a step is one sweep of single-body moves")
  ap.add_argument("--body-potential", default="none", metavar="none|deck|EPS,B",
                  help="Yukawa repulsion between body locations: none (the reference), deck (the steppers' law for this deck: "
                       "repulsion_strength, debye_length; needs body_body_force_torque_implementation python|hip) or two numbers")
  ap.add_argument("--pair-table", default=None, metavar="FILE",
                  help="a radial pair potential as a table (text: r U dU/dr on a uniform grid) instead of the pair term of --potential; "
                       "--moves all only")
  ap.add_argument("--gr", default=None, metavar="RMAX,BINS",
                  help="accumulate the pair-distance histogram of the body locations at every saved step and write <output_name>.gr.dat")
  args = ap.parse_args(argv)
  gr = None
  if args.gr is not None:
    try:
      r_max, n_bins = args.gr.split(",")
      gr = (float(r_max), int(n_bins))
    except ValueError:
      ap.error("--gr takes RMAX,BINS (a number and an integer), got %r" % (args.gr,))
  body_potential = None if args.body_potential == "none" else args.body_potential
  if body_potential not in (None, "deck"):
    try:
      body_potential = tuple(float(x) for x in body_potential.split(","))
    except ValueError:
      ap.error("--body-potential takes none, deck or EPS,B (two numbers), got %r" % (args.body_potential,))
  sampler = MCMCSampler(args.inputfile, device=args.device, potential=args.potential, rng=args.rng, verbose=True, moves=args.moves,
                        body_potential=body_potential, gr=gr, pair_table=args.pair_table)
  try:
    sampler.run()
  finally:
    sampler.close()
  return 0


if __name__ == "__main__":
  sys.exit(main())
