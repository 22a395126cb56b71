"""Block extraction from the HIP source -> target kernels and the element-wise comparison with the extended-precision
restatement (tests/_source_target_numpy.py) -- shared by tests/test_gpu_source_target_blocks.py and
tools/source_target_blocks_report.py.

The 3 ns one-hot force vectors (one-hot `vector` for the double layers) are fed to an entry point: every other source
contributes exact zeros, so each output column IS the kernel's block.  The kernel of every device launch is pinned with
`last_path` (0 = one-sided sweep, 1 = symmetric per wave, 3 = workgroup-cooperative) and `last_launch()["chunks"]`; the
host wrappers run on the library's default context, which has no getter -- with sources != targets the entry point has
only the one-sided sweep to take.

Forced chunks: the launcher gives a chunk at least 128 sources (choose_chunks of rmb_plan.hip, restated in `chunk_plan`),
so the 64 sources of the designed clouds are ONE chunk whatever is forced (asserted); chunk edges are pinned by the
one-hot sources of the whole products at the edge shapes."""
import ctypes

import numpy as np

import _source_target_numpy as sn
from _source_target_numpy import ETA, EXT, MARGIN

EPS = {64: 2.0 ** -53, 32: 2.0 ** -24}
RESULTS = {}        # (family, operator) -> worst ratio seen, in units of C
ST_HOST = {0: "no_wall_mobility_trans_times_force_source_target_hip", 1: "single_wall_mobility_trans_times_force_source_target_hip",
           2: "free_surface_mobility_trans_times_force_source_target_hip"}
WAVE, COOP = {"sym_coop": 0, "sym_two_targets": 0}, {"sym_coop": 2}

# sources == targets, N = 200: (options, expected last_path, precision, clouds, modes).  The dispatch of SX_RADII has a
# per-wave, a cooperative and a float instance; no two-target and no ordered ("deterministic" = 2) one: what those
# options fall back to is asserted.  The free surface (mode 2) has no symmetric instance at all.
SAME_FAMILIES = {
    "radii_sym_wave": (WAVE, 1, 64, ("open", "odd", "pow2"), (0, 1)),
    "radii_sym_coop": (COOP, 3, 64, ("open", "odd", "pow2"), (0, 1)),
    "radii_two_targets_falls_back_to_wave": ({"sym_coop": 0, "sym_two_targets": 2}, 1, 64, ("open", "pow2"), (0, 1)),
    "radii_deterministic2_falls_back_to_sweep": ({"deterministic": 2}, 0, 64, ("open",), (0, 1)),
    "radii_symmetric0_sweep": ({"symmetric": 0}, 0, 64, ("open", "odd"), (0, 1)),
    "radii_deterministic1_sweep": ({"deterministic": 1}, 0, 64, ("open", "pow2"), (0, 1)),
    "radii_free_surface_sweep": ({}, 0, 64, ("open", "odd"), (2,)),
    "radii_f32": ({"precision": 32}, 1, 32, ("open",), (0, 1)),
}


def same_cases():
  return [(f, c, m) for f, (_, _, _, clouds, modes) in SAME_FAMILIES.items() for c in clouds for m in modes]


def chunk_plan(ns, forced):
  """(chunks, chunk length) of a one-sided sweep with "chunks" = forced > 0."""
  c = max(1, min(forced, (ns + 127) // 128))
  length = 4 * ((((ns + c - 1) // c) + 3) // 4)
  return (ns + length - 1) // length, length


def dev(x):
  import torch
  return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64).reshape(-1), device="cuda")


def vp(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _lp(L):
  L = np.zeros(3) if L is None else np.ascontiguousarray(L, dtype=np.float64)
  return L, ctypes.c_void_p(L.ctypes.data)


class Device(object):
  """A context plus the library handle; launched() asserts the path and the chunk count of the last launch."""

  def __init__(self, Ctx, options=()):
    from rigidmultiblobswall_amd import _lib
    self.lib, self.check = _lib.load(), _lib.check
    self.ctx = Ctx(0)
    for key, val in dict(options).items():
      self.ctx.set_option(key, val)

  def close(self):
    self.ctx.close()

  def launched(self, path, chunks=None):
    got = self.ctx.get_option("last_path")
    assert got == path, "last_path %d, expected %d" % (got, path)
    if chunks is not None:
      assert self.ctx.last_launch()["chunks"] == chunks, (self.ctx.last_launch(), chunks)

  def st(self, mode, src, rs, tgt, rt, f, L, out):
    Lh, Lp = _lp(L)
    self.check(self.lib.rmb_mobility_source_target_device(self.ctx._h, src.numel() // 3, vp(src), vp(rs), tgt.numel() // 3, vp(tgt), vp(rt),
                                                          vp(f), ETA, Lp, mode, vp(out)))

  def pressure(self, wall, src, tgt, f, out):
    self.check(self.lib.rmb_pressure_stokeslet_device(self.ctx._h, src.numel() // 3, vp(src), tgt.numel() // 3, vp(tgt), vp(f), None, wall, vp(out)))

  def dl(self, variant, src, tgt, nrm, v, w, out):
    self.check(self.lib.rmb_double_layer_device(self.ctx._h, src.numel() // 3, vp(src), tgt.numel() // 3, vp(tgt), vp(nrm), vp(v), vp(w),
                                                1 if variant == "wall" else 0, sn.A_RPY if variant == "rpy" else -1.0, vp(out)))


# ---------------------------------------------------------------------------------------------------------------------
# extraction
# ---------------------------------------------------------------------------------------------------------------------
def extract_st_device(d, mode, src, rs, tgt, rt, L, path, chunks=None, same=False):
  """(nt, ns, 3, 3).  same: the SAME device pointers on both sides (what selects the symmetric path)."""
  import torch
  ns, nt = len(src), len(tgt)
  eye = torch.eye(3 * ns, dtype=torch.float64, device="cuda")
  sd, rsd = dev(src), dev(rs)
  td, rtd = (sd, rsd) if same else (dev(tgt), dev(rt))
  out = torch.empty((3 * ns, 3 * nt), dtype=torch.float64, device="cuda")
  for k in range(3 * ns):
    d.st(mode, sd, rsd, td, rtd, eye[k], L, out[k])
    d.launched(path, chunks)
  torch.cuda.synchronize()
  return out.cpu().numpy().reshape(ns, 3, nt, 3).transpose(2, 0, 3, 1)


def extract_st_host(mode, src, rs, tgt, rt, L, same=False):
  from rigidmultiblobswall_amd import mobility as mob
  fn = getattr(mob, ST_HOST[mode])
  ns, nt = len(src), len(tgt)
  kw = {} if L is None else {"periodic_length": np.asarray(L, dtype=np.float64)}
  out = np.empty((nt, ns, 3, 3))
  e = np.zeros((ns, 3))
  for j in range(ns):
    for q in range(3):
      e[j, q] = 1.0
      out[:, j, :, q] = (fn(src, src, e, rs, rs, ETA, **kw) if same else fn(src, tgt, e, rs, rt, ETA, **kw)).reshape(nt, 3)
      e[j, q] = 0.0
  return out


def extract_aux_device(d, op, src, nrm, w, tgt, chunks=None):
  """pressure: (nt, ns, 3) rows;  double layer: (nt, ns, 3, 3) blocks acting on `vector`."""
  import torch
  ns, nt = len(src), len(tgt)
  eye = torch.eye(3 * ns, dtype=torch.float64, device="cuda")
  sd, td, nd, wd = dev(src), dev(tgt), dev(nrm), dev(w)
  width = nt if op[0] == "p" else 3 * nt
  out = torch.empty((3 * ns, width), dtype=torch.float64, device="cuda")
  for k in range(3 * ns):
    if op[0] == "p":
      d.pressure(op[1], sd, td, eye[k], out[k])
    else:
      d.dl(op[1], sd, td, nd, eye[k], wd, out[k])
    d.launched(0, chunks)
  torch.cuda.synchronize()
  out = out.cpu().numpy()
  return out.reshape(ns, 3, nt).transpose(2, 0, 1) if op[0] == "p" else out.reshape(ns, 3, nt, 3).transpose(2, 0, 3, 1)


def extract_aux_host(op, src, nrm, w, tgt):
  from rigidmultiblobswall_amd import mobility as mob
  ns, nt = len(src), len(tgt)
  out = np.empty((nt, ns, 3) if op[0] == "p" else (nt, ns, 3, 3))
  e = np.zeros((ns, 3))
  for j in range(ns):
    for q in range(3):
      e[j, q] = 1.0
      if op[0] == "p":
        out[:, j, q] = (mob.single_wall_pressure_Stokeslet_hip if op[1] else mob.no_wall_pressure_Stokeslet_hip)(src, tgt, e)
      elif op[1] == "rpy":
        out[:, j, :, q] = mob.no_wall_double_layer_source_target_hip(src, tgt, nrm, e, w, sn.A_RPY).reshape(nt, 3)
      else:
        out[:, j, :, q] = mob.double_layer_source_target_hip(src, tgt, nrm, e, w, wall=1 if op[1] == "wall" else 0).reshape(nt, 3)
      e[j, q] = 0.0
  return out


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def compare(family, op, got, E, s, c, precision=64, one_hot_rows=False, note=""):
  """Assert |got - EXT| <= MARGIN c eps s element by element -- every block, except where EXT is non-finite: there (and
  only there) the kernel's must be non-finite too.  one_hot_rows (pressure): a target that coincides with ANY source is
  0 x inf in every one-hot column, in the oracle as in the kernel.  Where the scale is zero (a blob at z = 0 under the wall
  mode, a skipped pair without image) the block must be exactly zero.  Returns the worst ratio in units of c eps s."""
  got = np.asarray(got)
  assert got.shape == E.shape, (got.shape, E.shape)
  bad = ~np.isfinite(np.asarray(E, dtype=np.float64))
  if one_hot_rows:
    bad = np.broadcast_to(bad.reshape(len(E), -1).any(axis=1).reshape((-1,) + (1,) * (E.ndim - 1)), E.shape)
  assert np.array_equal(~np.isfinite(got), bad), "%s %s %s: non-finite entries at %s, expected at %s" % (
      family, op, note, np.argwhere(~np.isfinite(got))[:4].tolist(), np.argwhere(bad)[:4].tolist())
  E = np.where(bad, EXT(0), E)
  got = np.where(bad, 0.0, got)
  zero = np.broadcast_to((np.asarray(s) == 0).reshape(s.shape + (1,) * (E.ndim - s.ndim)), E.shape)
  assert np.all(got[zero] == 0), "%s %s %s: a block of zero scale is not exactly zero" % (family, op, note)
  ratio, where = sn.worst(got, E, s, c * EPS[precision])
  RESULTS[family, op] = max(RESULTS.get((family, op), 0.0), ratio)
  print("%-44s %-14s %-8s worst %.3f C at %s" % (family, op, note, ratio, where))
  assert ratio <= MARGIN, ("family %s operator %s %s: element %s is off by %.2f C = %.1f units of 2^-%d s (bound %g C); got %.17g, "
                           "extended precision %s" % (family, op, note, where, ratio, ratio * c, 53 if precision == 64 else 24, MARGIN,
                                                      got[where], np.format_float_scientific(E[where], precision=20)))
  return ratio
