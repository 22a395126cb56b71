"""Shared by the host and GPU tests of the single-body Metropolis moves: the small decks (boomerangs and shells from the
g14_mcmc_* fixtures' vertex sets), the numpy statement of the energy-difference rule in long double, and a brute-force chain.

The rule: with E(r) = sum_i u1(z_i) + sum_{i<j, z_i>0} u2(r_ij) and r' = r except for the rows
[first, first + count) of one body, E(r') - E(r) is the sum over the touched terms, each subtracted (new - old):
  j < first            pair (j, i): gate z_j > 0, unchanged by the move
  j >= first + count   pair (i, j): gate z'_i > 0 for the new term, z_i > 0 for the old one
  both in the body     pair (i, j), i < j, once: gates as the row above
plus u1(z'_j) - u1(z_j) of the body's blobs."""
import os

import numpy as np

import _potential_numpy as potnp
from conftest import golden_files, load_golden

EXT = potnp.EXT


def vertex_sets():
  """(boomerang: 15 blobs, shell: 12 blobs) reference configurations of the recorded chains."""
  boom = load_golden([p for p in golden_files("g14_mcmc_*.npz") if "boomerang_periodic_soft" in p][0])["vertex_0"]
  shell = load_golden([p for p in golden_files("g14_mcmc_*.npz") if "shells_yukawa" in p][0])["vertex_0"]
  assert boom.shape == (15, 3) and shell.shape == (12, 3)
  return boom, shell


def random_quaternions(rng, n):
  q = rng.normal(size=(n, 4))
  return q / np.linalg.norm(q, axis=1)[:, None]


def rotate(q, ref):
  """R(q) ref for one unit quaternion (s, p), written out (quaternion.py:42-51)."""
  s, p = q[0], q[1:]
  R = 2.0 * (np.outer(p, p) + (s * s - 0.5) * np.eye(3) + s * np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]))
  return ref @ R.T


def quaternion_of_rotation_vector(phi):
  """quaternion.py:17-39"""
  nrm = np.linalg.norm(phi)
  return np.concatenate([[np.cos(0.5 * nrm)], np.sin(0.5 * nrm) * phi / nrm if nrm != 0 else np.zeros(3)])


def quaternion_product(a, b):
  return np.concatenate([[a[0] * b[0] - a[1:] @ b[1:]], a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:])])


class Deck(object):
  """Bodies = a list of (reference configuration, location, quaternion), in blob order."""

  def __init__(self, refs, loc, quat):
    self.refs, self.loc, self.quat = refs, np.array(loc, dtype=np.float64), np.array(quat, dtype=np.float64)
    self.first = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64)
    self.n = int(self.first[-1])

  def body_blobs(self, k, loc=None, quat=None):
    return rotate(self.quat[k] if quat is None else quat, self.refs[k]) + (self.loc[k] if loc is None else loc)

  def blobs(self):
    return np.concatenate([self.body_blobs(k) for k in range(len(self.refs))])


def layout(refs, spacing, height, seed, side=None):
  """Bodies on a square grid of pitch `spacing` (jittered), random orientations, centres at `height` (jittered)."""
  rng = np.random.RandomState(seed)
  nb = len(refs)
  m = int(np.ceil(np.sqrt(nb)))
  loc = np.array([[spacing * (k % m), spacing * (k // m), height] for k in range(nb)], dtype=np.float64)
  loc += rng.uniform(-0.15, 0.15, (nb, 3)) * spacing
  if side is not None:          # spread over the whole box and beyond one cell: pairs on both sides of the half box
    loc[:, 0] *= side / (spacing * m)
    loc[:, 1] *= side / (spacing * m)
    loc[::3, 0] += side
  return Deck(refs, loc, random_quaternions(rng, nb))


def deck_of(name, seed=0, periodic=False, far=None):
  """The decks of the parity tests, by blob count.  `far` (periodic decks of two bodies, which have ONE body pair): put that
  pair at 0.7 of the box in x (True: beyond the half box, met through the image) or at 0.3 (False)."""
  boom, shell = vertex_sets()
  one = np.zeros((1, 3))
  rng = np.random.RandomState(100 + seed)
  if name == 1:
    refs, spacing, height = [one], 1.0, 0.45
  elif name == 2:
    refs, spacing, height = [one, one], 0.35, 0.45
  elif name == 27:
    refs, spacing, height = [boom, shell], 1.1, 1.1
  elif name == 66:
    refs, spacing, height = [boom, boom, shell, shell, shell], 1.3, 1.2
  elif name == 267:
    refs, spacing, height = [boom] + [shell] * 21, 0.9, 0.9
  elif name == 600:
    big = rng.uniform(-1.0, 1.0, (300, 3)) * np.array([1.5, 1.5, 0.6])
    refs, spacing, height = [big, big[::-1].copy()], 1.6, 1.3
  else:
    raise ValueError(name)
  side = None
  if periodic:
    side = max(2.5, spacing * np.ceil(np.sqrt(len(refs))) * 0.9)
  d = layout(refs, spacing, height, seed, side)
  if periodic and far is not None and len(refs) == 2:
    d.loc[1, 0] = d.loc[0, 0] + (0.7 if far else 0.3) * side
  d.L = np.array([side, side, 0.0]) if periodic else np.zeros(3)
  return d


def moved_body(deck, k, seed, shift=0.08, angle=0.3):
  """A proposal for body k: displaced by up to `shift` per coordinate and rotated by a rotation vector of scale `angle`."""
  rng = np.random.RandomState(7000 + seed)
  loc = deck.loc[k] + rng.uniform(-shift, shift, 3)
  quat = quaternion_product(quaternion_of_rotation_vector(angle * rng.normal(size=3)), deck.quat[k])
  return deck.body_blobs(k, loc, quat)


def delta_rule(r, first, body_new, **kw):
  """The difference rule in EXT: (dU_one, dU_pair, S_one, S_pair), S = sum(|new term| + |old term|) over the touched terms."""
  L, eps, b, eps_w, b_w, w, a, form = potnp._params(kw)
  r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
  new_body = np.asarray(body_new, dtype=np.float64).reshape(-1, 3)
  n, count = r.shape[0], new_body.shape[0]
  end = first + count
  x_old = r.astype(EXT)
  x_new = x_old.copy()
  x_new[first:end] = new_body.astype(EXT)
  u_new = potnp.one_blob_terms(x_new[first:end, 2], eps_w, b_w, w, a, form)
  u_old = potnp.one_blob_terms(x_old[first:end, 2], eps_w, b_w, w, a, form)
  d_one, S_one = (u_new - u_old).sum(dtype=EXT), (np.abs(u_new) + np.abs(u_old)).sum(dtype=EXT)
  d_pair, S_pair = EXT(0), EXT(0)
  zero = EXT(0)
  for i in range(first, end):
    for lo, hi, low_is_j in ((0, first, True), (i + 1, n, False)):       # j below the body; j above i (in the body or beyond)
      if hi <= lo:
        continue
      j = np.arange(lo, hi)
      t_new = potnp.pair_terms(x_new[i][None, :] - x_new[j], L, eps, b, a, form)
      t_old = potnp.pair_terms(x_old[i][None, :] - x_old[j], L, eps, b, a, form)
      if low_is_j:
        g_new = g_old = r[j, 2] > 0
      else:
        g_new, g_old = np.full(j.size, new_body[i - first, 2] > 0), np.full(j.size, r[i, 2] > 0)
      t_new, t_old = np.where(g_new, t_new, zero), np.where(g_old, t_old, zero)
      d_pair = d_pair + (t_new - t_old).sum(dtype=EXT)
      S_pair = S_pair + (np.abs(t_new) + np.abs(t_old)).sum(dtype=EXT)
  return d_one, d_pair, S_one, S_pair


GATE_CASES = ("before_only", "after_only", "lower_body_not_moved", "moved_body_lower_index", "moved_body_higher_index")


def gate_case(name, periodic=False, seed=3):
  """66-blob deck, body 2 (blobs 30 ... 41) moved, one blob put behind the wall (z <= 0).  -> (deck, r, first, body_new)"""
  deck = deck_of(66, seed=seed, periodic=periodic)
  r, k = deck.blobs(), 2
  first, count = int(deck.first[k]), len(deck.refs[k])
  new = moved_body(deck, k, seed)
  if name == "before_only":
    r[first + 4, 2] = -0.03
  elif name == "after_only":
    new[4, 2] = -0.02
  elif name == "lower_body_not_moved":
    r[7, 2] = -0.05          # blob 7 of body 0: the lower index of its pairs with every blob of the moved body
    r[20, 2] = 0.0           # z = 0 counts as behind the wall too
  elif name == "moved_body_lower_index":
    r[first, 2], new[0, 2] = -0.04, -0.01          # the body's first blob: lower index of every intra-body pair it is in
  elif name == "moved_body_higher_index":
    r[first + count - 1, 2], new[count - 1, 2] = -0.04, -0.06      # its last blob: the higher index of every intra-body pair
  else:
    raise ValueError(name)
  return deck, r, first, new


def potential_kw(form, L=None, wall_terms=True, a=0.2):
  kw = dict(repulsion_strength=0.35, debye_length=0.45 * a, blob_radius=a, weight=0.6 if wall_terms else 0.0, potential=form,
            periodic_length=np.zeros(3) if L is None else L)
  if wall_terms:
    kw.update(repulsion_strength_wall=0.8, debye_length_wall=0.6 * a)
  return kw


def write_deck(directory, deck, structures, lines):
  """`structures`: list of (keyword, name, body indices) -- bodies of one structure share a reference configuration.
  -> path of the deck file."""
  text = ""
  for keyword, name, bodies in structures:
    ref = deck.refs[bodies[0]]
    with open(os.path.join(directory, name + ".vertex"), "w") as f:
      f.write("%d\n" % len(ref) + "".join("%.17g %.17g %.17g\n" % tuple(x) for x in ref))
    with open(os.path.join(directory, name + ".clones"), "w") as f:
      f.write("%d\n" % len(bodies) + "".join("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" % (tuple(deck.loc[k]) + tuple(deck.quat[k])) for k in bodies))
    text += "%s %s.vertex %s.clones\n" % (keyword, name, name)
  path = os.path.join(directory, "data.main")
  with open(path, "w") as f:
    f.write(lines + text)
  return path


def energy_fn(read, form):
  kw = dict(periodic_length=read.periodic_length, debye_length_wall=read.debye_length_wall, repulsion_strength_wall=read.repulsion_strength_wall,
            debye_length=read.debye_length, repulsion_strength=read.repulsion_strength, weight=1.0 * read.g, blob_radius=read.blob_radius,
            potential=form)
  return lambda r: potnp.total(r, **kw), kw


def brute_force_chain(deck, n_free, rng, n_sweeps, max_translation, max_angle_shift, kT, energy, rng_mode="reference"):
  """Single-body moves written out: per sweep and free body the draws in the sampler's order, the proposal of that body
  alone, dE = energy(new) - energy(old), u < exp(-dE/kT).  -> (flags, list of (loc, quat) after every sweep, energies)"""
  loc, quat = deck.loc.copy(), deck.quat.copy()
  blobs = lambda lo, qu: np.concatenate([rotate(qu[k], deck.refs[k]) + lo[k] for k in range(len(deck.refs))])   # noqa: E731
  current = np.float64(energy(blobs(loc, quat)))
  flags, states, energies = [], [], [float(current)]
  for _ in range(n_sweeps):
    t = max_translation
    if rng_mode == "reference":
      draws = []
      for k in range(n_free):
        draws.append((rng.uniform(-t, t, 3), rng.normal(0, 1, 3), rng.uniform(0.0, 1.0)))
    else:
      du, dphi, u = rng.uniform(-t, t, (n_free, 3)), rng.normal(0, 1, (n_free, 3)), rng.uniform(0.0, 1.0, n_free)
      draws = [(du[k], dphi[k], u[k]) for k in range(n_free)]
    for k, (du, dphi, u) in enumerate(draws):
      loc_new, quat_new = loc.copy(), quat.copy()
      loc_new[k] = loc[k] + du
      quat_new[k] = quaternion_product(quaternion_of_rotation_vector(dphi * max_angle_shift), quat[k])
      sample = np.float64(energy(blobs(loc_new, quat_new)))
      with np.errstate(over="ignore", invalid="ignore"):
        ok = bool(u < np.exp(-(sample - current) / np.float64(kT)))
      flags.append(ok)
      if ok:
        loc, quat, current = loc_new, quat_new, sample
    states.append((loc.copy(), quat.copy()))
    energies.append(float(current))
  return flags, states, energies
