"""Persistent device context: positions resident across the matvecs of a solve.

Semantic list of SURVEY.md section 8(b): create/destroy, set_positions (upload + height clamp + B
on device), matvec(kind), blob_blob_forces, timing.  The reference has no such object -- every
pycuda call re-allocates and re-uploads (mobility/mobility_pycuda.py:2249-2266).
"""
import ctypes

import numpy as np

from . import _lib
from ._lagged import counts_per_lag


def _as_f64(x, n3=None):
  x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
  if n3 is not None and x.size != n3:
    raise ValueError("expected %d values, got %d" % (n3, x.size))
  return x


def _ptr(x):
  return ctypes.c_void_p(x.ctypes.data)


def _lag_origins(n_frames, n_series, n_lags, origins, o_begin=0, o_end=None):
  """(counts, o_begin, o_end) of a lag entry: counts is counts_per_lag (which checks n_lags and origins) of the whole range;
  o_end=None is the last origin of the convention `origins`."""
  counts = counts_per_lag(n_frames, n_series, n_lags, origins)
  if o_end is None:
    o_end = max(n_frames - n_lags + 1, 0) if origins == "window" else n_frames
  return counts, int(o_begin), int(o_end)


def _cuda_out(out, shape, named, dtype, device, what="out", zero=True):
  """The out= rules of the entries whose result has a shape: a contiguous CUDA tensor of dtype `dtype` ("float64", "int64") and
  shape `shape` (`named` in the refusal); None makes one, of zeros where the entry ADDS to it."""
  import torch
  if out is None:
    return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, dtype), device=device)
  if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == getattr(torch, dtype) and out.is_contiguous() and
          tuple(out.shape) == tuple(shape)):
    raise ValueError("%s must be a contiguous CUDA %s tensor of shape %s" % (what, dtype, named))
  return out


POTENTIAL_FORMS = {"soft": 0, "yukawa": 1}   # rmb_blob_potential's `form`
VAN_HOVE_PLANES = {"xyz": 0, "xy": 1}        # rmb_van_hove_*'s `plane`


class MobilityContext(object):
  """One context = one GPU.  Host (numpy) and device (torch tensor) entry points."""

  def __init__(self, device=0):
    self._lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(self._lib.rmb_ctx_create(int(device), ctypes.byref(h)))
    self._h = h
    self.device = int(device)
    self.n = 0
    self.n_targets = 0
    self.target_range = (0, 0)
    self._keepalive = None
    self._stream_handle = None  # hipStream_t the C context currently enqueues on
    self._user_stream = False   # True once set_stream() pinned a caller-owned stream
    self._options_set = {}      # every option set through this wrapper (launch_signature)
    self._geometry = None       # (n, a, L, wall) of the bound configuration

  def close(self):
    if getattr(self, "_h", None) is not None and self._h.value:
      self._lib.rmb_ctx_destroy(self._h)
      self._h = ctypes.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  # --- configuration ---------------------------------------------------------------------------
  def set_stream(self, stream_ptr):
    """Pin the context to a caller-owned hipStream_t (otherwise device-path calls follow torch's current stream)."""
    _lib.check(self._lib.rmb_ctx_set_stream(self._h, ctypes.c_void_p(int(stream_ptr) if stream_ptr else 0)))
    self._user_stream = True

  def release_stream(self):
    """Call BEFORE destroying a stream this context is bound to: waits for the context's work on it and forgets the
    handle (rmb_ctx_release_stream).  The next device call follows torch's current stream again unless set_stream()
    pins another one."""
    _lib.check(self._lib.rmb_ctx_release_stream(self._h))
    self._stream_handle = 0
    self._user_stream = False

  # Ordering of the device path against PyTorch: every *_device call is enqueued on the stream that is
  # torch's CURRENT stream at call time (handle passed through the C ABI), so it is ordered after the
  # torch kernels that produced its inputs and before those that consume its outputs -- no events, no
  # host synchronisation.  (Measured alternative: a private stream + wait_stream fences costs ~24 us per
  # call, 11 % of a 1e4-blob matvec.)
  def _follow_torch_stream(self):
    if self._user_stream:
      return
    h = _current_raw_stream(self.device)
    if h != self._stream_handle:
      _lib.check(self._lib.rmb_ctx_set_stream(self._h, ctypes.c_void_p(h)))
      self._stream_handle = h

  def set_option(self, key, value):
    _lib.check(self._lib.rmb_ctx_set_option(self._h, key.encode(), int(value)))
    self._options_set[key] = int(value)

  def launch_signature(self):
    """Everything that decides WHICH launches a product of this context turns into, as far as this wrapper knows: the
    number of blobs, radius, box and wall of the bound configuration and every option set through set_option().  A
    captured hipGraph of device-path calls stays valid while this is unchanged (positions may move: the packed
    coordinates are rewritten in place) -- RigidSuspension keys its captured Arnoldi iterations (krylov._ArnoldiGraphs) on it."""
    return (self._geometry, tuple(self.target_range), tuple(sorted(self._options_set.items())))

  def buffers_signature(self):
    """Hash of the addresses of every device buffer the library owns for this context (read-only option
    "buffers_signature").  A captured graph holds those addresses by value: it may be replayed only while this is what it
    was at capture time (a buffer that grows is freed and reallocated)."""
    return self.get_option("buffers_signature")

  def get_option(self, key):
    v = ctypes.c_long()
    _lib.check(self._lib.rmb_ctx_get_option(self._h, key.encode(), ctypes.byref(v)))
    return int(v.value)

  supports_free_surface = True     # set_positions(wall="free_surface"), see there
  supports_free_surface_rotation = True   # option "free_surface_rotation": tr / rt / rr / tt_tr and the multi-block operations there

  def set_positions(self, r_vectors, a, periodic_length=None, wall=True):
    """r_vectors: numpy (N,3)/(3N,) or a CUDA torch float64 tensor (stays on device).
    wall: True (no-slip wall at z = 0: clamped heights, B damping), False (unbounded) or "free_surface": a stress-free
    surface at z = 0 (context option "free_surface" + wall = 1 in the C ABI).  On such a configuration kind "tt" is the
    free-surface product and the dense blocks and the rigid-body solver calls carry its image; "tr" / "rt" / "rr" /
    "tt_tr", in_plane and the multi-block operations raise (RMB_ERR_STATE) -- the reference has no such products.
    set_option("free_surface_rotation", 1) serves them from the mirror-image system (a force mirrors as S f, a torque
    as -S tau, S = diag(1, 1, -1)): beyond the reference, fp64, periodic_length[2] = 0, no in_plane, no matvec2_device."""
    free_surface = isinstance(wall, str)
    if free_surface and wall != "free_surface":
      raise ValueError("wall must be True, False or \"free_surface\"")
    if free_surface != bool(self._options_set.get("free_surface", 0)) and wall:
      self.set_option("free_surface", 1 if free_surface else 0)
    L = _as_f64(np.zeros(3) if periodic_length is None else periodic_length, 3)
    if _is_torch_cuda(r_vectors):
      r = r_vectors.contiguous().view(-1)
      n = r.numel() // 3
      self._follow_torch_stream()
      _lib.check(self._lib.rmb_set_positions_device(self._h, ctypes.c_void_p(r.data_ptr()), n, float(a), _ptr(L),
                                                    int(bool(wall))))
      self._keepalive = r
    else:
      r = _as_f64(r_vectors)
      n = r.size // 3
      _lib.check(self._lib.rmb_set_positions(self._h, _ptr(r), n, float(a), _ptr(L), int(bool(wall))))
    self.n = n
    self.n_targets = n
    self.target_range = (0, n)
    self._geometry = (int(n), float(a), tuple(float(x) for x in L), wall if free_surface else bool(wall))

  def set_target_range(self, begin, end):
    _lib.check(self._lib.rmb_set_target_range(self._h, int(begin), int(end)))
    self.target_range = (int(begin), int(end))
    self.n_targets = int(end) - int(begin)

  # --- products --------------------------------------------------------------------------------
  def matvec(self, kind, vec, eta, vec2=None, in_plane=False):
    """Host path: numpy in, new numpy (3*n_targets,) out; synchronous."""
    k = _lib.KINDS[kind] if isinstance(kind, str) else int(kind)
    v = _as_f64(vec, 3 * self.n)
    v2 = _as_f64(vec2, 3 * self.n) if vec2 is not None else None
    out = np.empty(3 * self.n_targets)
    _lib.check(self._lib.rmb_matvec(self._h, k, int(bool(in_plane)), _ptr(v), _ptr(v2) if v2 is not None else None,
                                    float(eta), _ptr(out)))
    return out

  def matvec_device(self, kind, vec, eta, vec2=None, in_plane=False, out=None):
    """Device path: CUDA float64 torch tensors; asynchronous on the context's stream."""
    import torch
    k = _lib.KINDS[kind] if isinstance(kind, str) else int(kind)
    if not _is_torch_cuda(vec) or vec.numel() != 3 * self.n or not vec.is_contiguous():
      raise ValueError("vec must be a contiguous CUDA float64 tensor with 3*n entries")
    if vec2 is not None and (not _is_torch_cuda(vec2) or vec2.numel() != 3 * self.n or not vec2.is_contiguous()):
      raise ValueError("vec2 must be a contiguous CUDA float64 tensor with 3*n entries")
    if out is None:
      out = torch.empty(3 * self.n_targets, dtype=torch.float64, device=vec.device)
    elif not _is_torch_cuda(out) or out.numel() != 3 * self.n_targets or not out.is_contiguous():
      raise ValueError("out must be a contiguous CUDA float64 tensor with 3*n_targets entries")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_matvec_device(self._h, k, int(bool(in_plane)), ctypes.c_void_p(vec.data_ptr()),
                                           ctypes.c_void_p(vec2.data_ptr()) if vec2 is not None else None,
                                           float(eta), ctypes.c_void_p(out.data_ptr())))
    return out

  def matvec_pairshard_device(self, kind, vec, eta, shard, nshards, out=None):
    """Contribution of pair-shard `shard` of `nshards` to ALL targets (3n entries): tt / tr / rt / rr / tt_free."""
    import torch
    k = _lib.KINDS[kind] if isinstance(kind, str) else int(kind)
    if not _is_torch_cuda(vec) or vec.numel() != 3 * self.n or not vec.is_contiguous():
      raise ValueError("vec must be a contiguous CUDA float64 tensor with 3*n entries")
    if out is None:
      out = torch.empty(3 * self.n, dtype=torch.float64, device=vec.device)
    elif not _is_torch_cuda(out) or out.numel() != 3 * self.n or not out.is_contiguous():
      raise ValueError("out must be a contiguous CUDA float64 tensor with 3*n entries")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_matvec_pairshard_device(self._h, k, ctypes.c_void_p(vec.data_ptr()), float(eta),
                                                     ctypes.c_void_p(out.data_ptr()), int(shard), int(nshards)))
    return out

  def matvec2_device(self, kind, vec_a, vec_b, eta, out_a=None, out_b=None, shard=0, nshards=1):
    """Two tt products in one pass over the pairs: returns (M vec_a, M vec_b) (rmb_matvec2_device; with nshards > 1
    the contribution of one pair shard, to be summed over shards).  out_a / out_b: optional contiguous 3n tensors."""
    import torch
    k = _lib.KINDS[kind] if isinstance(kind, str) else int(kind)
    for v in (vec_a, vec_b):
      if not _is_torch_cuda(v) or v.numel() != 3 * self.n or not v.is_contiguous():
        raise ValueError("vectors must be contiguous CUDA float64 tensors with 3*n entries")
    outs = []
    for o in (out_a, out_b):
      if o is None:
        o = torch.empty(3 * self.n, dtype=torch.float64, device=vec_a.device)
      elif not _is_torch_cuda(o) or o.numel() != 3 * self.n or not o.is_contiguous():
        raise ValueError("outputs must be contiguous CUDA float64 tensors with 3*n entries")
      outs.append(o)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_matvec2_pairshard_device(self._h, k, ctypes.c_void_p(vec_a.data_ptr()),
                                                      ctypes.c_void_p(vec_b.data_ptr()), float(eta),
                                                      ctypes.c_void_p(outs[0].data_ptr()),
                                                      ctypes.c_void_p(outs[1].data_ptr()), int(shard), int(nshards)))
    return outs[0], outs[1]

  def matvec_op_device(self, op, vecs, eta, in_plane=False, outs=None, shard=0, nshards=1):
    """Several blocks of the grand mobility from one pass over the pairs (rmb_matvec_op_device):
      "velocity_from_force_torque"  (f, tau) -> (M_tt f + M_tr tau,)
      "grand"                       (f, tau) -> (M_tt f + M_tr tau, M_rt f + M_rr tau)
      "force_column"                (f,)     -> (M_tt f, M_rt f)
      "tt_multi" (tr_ / rt_ / rr_)  k vectors -> the block applied to each (k = 1..4)
    vecs / outs: sequences of contiguous CUDA float64 tensors with 3n (outs: 3*n_targets) entries; returns the tuple
    of outputs.  With nshards > 1: the contribution of one pair shard to all n targets (to be summed over shards)."""
    import torch
    code, n_in, n_out = _lib.OPS[op]
    if n_in is None:
      n_in = n_out = len(vecs)
    if len(vecs) != n_in:
      raise ValueError("%s takes %d input vectors" % (op, n_in))
    for v in vecs:
      if not _is_torch_cuda(v) or v.numel() != 3 * self.n or not v.is_contiguous():
        raise ValueError("vectors must be contiguous CUDA float64 tensors with 3*n entries")
    n_res = 3 * (self.n if nshards > 1 else self.n_targets)
    if outs is None:
      outs = [torch.empty(n_res, dtype=torch.float64, device=vecs[0].device) for _ in range(n_out)]
    outs = list(outs)
    if len(outs) != n_out:
      raise ValueError("%s produces %d output vectors" % (op, n_out))
    for o in outs:
      if not _is_torch_cuda(o) or o.numel() != n_res or not o.is_contiguous():
        raise ValueError("outputs must be contiguous CUDA float64 tensors with %d entries" % n_res)
    ins_p = (ctypes.c_void_p * n_in)(*[v.data_ptr() for v in vecs])
    outs_p = (ctypes.c_void_p * n_out)(*[o.data_ptr() for o in outs])
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_matvec_op_pairshard_device(self._h, code, int(bool(in_plane)), n_in,
                                                        ctypes.cast(ins_p, ctypes.c_void_p), n_out,
                                                        ctypes.cast(outs_p, ctypes.c_void_p), float(eta), int(shard),
                                                        int(nshards)))
    return tuple(outs)

  def body_mobility_dense_device(self, first_blob, n_b, eta, out=None):
    """Dense (3 n_b x 3 n_b) tt mobility of every listed body (int64 CUDA tensor of first-blob indices)."""
    import torch
    if not (isinstance(first_blob, torch.Tensor) and first_blob.is_cuda and first_blob.dtype == torch.int64):
      raise ValueError("first_blob must be a CUDA int64 tensor")
    first_blob = first_blob.contiguous()
    nb = first_blob.numel()
    if out is None:
      out = torch.empty((nb, 3 * n_b, 3 * n_b), dtype=torch.float64, device=first_blob.device)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_body_mobility_dense_device(self._h, ctypes.c_void_p(first_blob.data_ptr()), nb, int(n_b),
                                                        float(eta), ctypes.c_void_p(out.data_ptr())))
    return out

  # --- O(N) helpers of the rigid-body solve (csrc/rmb_krylov.hip) -------------------------------
  @staticmethod
  def _block(t, transpose=False):
    """rmb_block of a (batch, rows, cols) CUDA float64 tensor (any strides), or of its transpose per batch entry."""
    if t is None:
      return None
    assert t.dim() == 3 and t.dtype.itemsize == 8
    bs, rs, cs = t.stride()
    return _lib.Block(t.data_ptr(), bs, cs if transpose else rs, rs if transpose else cs)

  def block_apply_device(self, a11, a12, a21, a22, x1, x2, y1, y2, alpha=1.0, beta1=0.0, beta2=0.0, transpose=(False,) * 4):
    """y1_b = beta1 y1_b + alpha (A11_b x1_b + A12_b x2_b), y2_b likewise with A21, A22, for every batch entry b, in one
    launch (rmb_block_apply_device).  a..: (batch, rows, cols) tensors or None (zero block); x1 (batch, c1), x2 (batch, c2),
    y1 (batch, r1), y2 (batch, r2) contiguous views.  transpose[k]: use the k-th block transposed."""
    nb, c1, c2, r1, r2 = x1.shape[0], x1.shape[1], x2.shape[1], y1.shape[1], y2.shape[1]
    blocks = [self._block(t, tr) for t, tr in zip((a11, a12, a21, a22), transpose)]
    refs = [ctypes.byref(b) if b is not None else None for b in blocks]
    assert x1.is_contiguous() and x2.is_contiguous() and y1.is_contiguous() and y2.is_contiguous()
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_block_apply_device(self._h, nb, r1, c1, r2, c2, refs[0], refs[1], refs[2], refs[3],
                                                ctypes.c_void_p(x1.data_ptr()), ctypes.c_void_p(x2.data_ptr()), float(alpha),
                                                float(beta1), ctypes.c_void_p(y1.data_ptr()), float(beta2),
                                                ctypes.c_void_p(y2.data_ptr())))

  def rigid_configuration_device(self, ref, loc, quat, r, rel=None, K=None):
    """Blob coordinates, body-frame offsets and K of every body in one launch (rmb_rigid_configuration_device).
    ref (nb, n_b, 3), loc (nb, 3), quat (nb, 4); outputs r (nb n_b, 3), rel (nb, n_b, 3), K (nb, 3 n_b, 6), contiguous."""
    nb, n_b = ref.shape[0], ref.shape[1]
    for t in (ref, loc, quat, r, rel, K):
      assert t is None or (t.is_contiguous() and t.dtype.itemsize == 8)
    assert loc.numel() == 3 * nb and quat.numel() == 4 * nb and r.numel() == 3 * nb * n_b
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_configuration_device(self._h, nb, n_b, p(ref), p(loc), p(quat), p(r), p(rel), p(K)))

  def rigid_advance_device(self, loc, quat, U, dt):
    """(loc + U[:, :3] dt, quaternion(U[:, 3:] dt) * quat) as new tensors, one launch (rmb_rigid_advance_device).
    dt: a float, or a per-body (nb,) / (nb, 1) tensor."""
    import torch
    nb = loc.shape[0]
    U = U.reshape(nb, 6)
    assert loc.is_contiguous() and quat.is_contiguous() and U.is_contiguous()
    per_body = dt.reshape(-1).contiguous() if isinstance(dt, torch.Tensor) else None
    assert per_body is None or per_body.numel() == nb
    loc_out, quat_out = torch.empty_like(loc), torch.empty_like(quat)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_advance_device(self._h, nb, ctypes.c_void_p(loc.data_ptr()), ctypes.c_void_p(quat.data_ptr()),
                                                  ctypes.c_void_p(U.data_ptr()), 0.0 if per_body is not None else float(dt),
                                                  ctypes.c_void_p(per_body.data_ptr()) if per_body is not None else None,
                                                  ctypes.c_void_p(loc_out.data_ptr()), ctypes.c_void_p(quat_out.data_ptr())))
    return loc_out, quat_out

  def rigid_preconditioner_device(self, Mb, K, Lchol, Linv, Minv, Nbody, A11, A12, A21, A22, info):
    """Per-body Cholesky factor, inverses and the preconditioner's four blocks in one launch
    (rmb_rigid_preconditioner_device).  Mb (nb, n, n), K (nb, n, 6), outputs contiguous; info: int32 tensor of one entry."""
    nb, n = Mb.shape[0], Mb.shape[1]
    outs = (Lchol, Linv, Minv, Nbody, A11, A12, A21, A22)
    assert all(t.is_contiguous() for t in (Mb, K) + outs) and n % 3 == 0 and info.dtype.itemsize == 4
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_preconditioner_device(self._h, nb, n // 3, ctypes.c_void_p(Mb.data_ptr()),
                                                         ctypes.c_void_p(K.data_ptr()), *[ctypes.c_void_p(t.data_ptr()) for t in outs],
                                                         ctypes.c_void_p(info.data_ptr())))

  def krylov_orthogonalize_device(self, V, rows, w, col, v_next, col_mapped=0):
    """Two classical Gram-Schmidt passes of w against V[:rows] (row-major (m, n) tensor), in place; col[:rows] = the
    coefficients, col[rows] = |w|, v_next = w / |w| (rmb_krylov_orthogonalize2_device).  col_mapped: device address of
    rows + 1 doubles of mapped host memory (MappedHostArray.dev_ptr + offset) that receive the column too, or 0."""
    n = w.numel()
    assert V.stride(1) == 1 and V.shape[1] == n and w.is_contiguous() and col.is_contiguous() and v_next.is_contiguous()
    assert col.numel() >= rows + 1 and v_next.numel() == n
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_krylov_orthogonalize2_device(self._h, n, int(rows), ctypes.c_void_p(V.data_ptr()), V.stride(0),
                                                          ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(col.data_ptr()),
                                                          ctypes.c_void_p(v_next.data_ptr()),
                                                          ctypes.c_void_p(col_mapped) if col_mapped else None))

  def rigid_arnoldi_step_device(self, A11, A12, A21, A22, K, V, j, eta, z, w, col, col_mapped=0):
    """One Arnoldi step of the rigid-body GMRES enqueued by one call (rmb_rigid_arnoldi_step_device): z = P^-1 V[j],
    w = A z, Gram-Schmidt against V[:j + 1], column -> col (and the mapped host address), V[j + 1] = w / |w|."""
    nb, n_b = K.shape[0], K.shape[1] // 3
    for t in (A11, A12, A21, A22, K, z, w, col):
      assert t.is_contiguous()
    assert V.stride(1) == 1 and V.shape[1] == z.numel() == w.numel() == 3 * nb * n_b + 6 * nb and col.numel() >= j + 2
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_arnoldi_step_device(self._h, nb, n_b, p(A11), p(A12), p(A21), p(A22), p(K), p(V), V.stride(0), int(j),
                                                       float(eta), p(z), p(w), p(col), ctypes.c_void_p(col_mapped) if col_mapped else None))

  # ---- single steps of the native loops (the step-level tests): each enqueues one iteration's launches and returns --------
  def krylov_orthogonalize3_device(self, V, rows, w, col, v_next, col_mapped=0, low_sync=True, blocks=None, z=None, r1=0, r2=0,
                                   transpose=(False,) * 4):
    """Any form of the Gram-Schmidt ending (rmb_krylov_orthogonalize3_device): as krylov_orthogonalize_device, with the
    low-synchronisation ending when low_sync, and -- z given -- z = blocks * v_next written by the last launch: blocks =
    (a11, a12, a21, a22) of (n_bodies, r, c) tensors or None, the vector laid out as [n_bodies x r1; n_bodies x r2].
    V: (m, n) view with unit column stride (the row stride may exceed n)."""
    n = w.numel()
    assert V.stride(1) == 1 and w.is_contiguous() and col.is_contiguous() and v_next.is_contiguous()
    refs, nb = [None] * 4, 0
    if z is not None:
      assert z.is_contiguous()
      keep = [self._block(t, tr) for t, tr in zip(blocks, transpose)]
      refs = [ctypes.byref(b) if b is not None else None for b in keep]
      nb = n // (r1 + r2) if r1 + r2 > 0 and n % (r1 + r2) == 0 else 0
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_krylov_orthogonalize3_device(self._h, n, int(rows), ctypes.c_void_p(V.data_ptr()), V.stride(0),
                                                          ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(col.data_ptr()),
                                                          ctypes.c_void_p(v_next.data_ptr()), ctypes.c_void_p(col_mapped) if col_mapped else None,
                                                          int(bool(low_sync)), nb, int(r1), int(r2), refs[0], refs[1], refs[2], refs[3],
                                                          ctypes.c_void_p(z.data_ptr()) if z is not None else None))

  def krylov_lincomb_device(self, y, V, coef, k):
    """y += V[:k]^T coef in one launch (rmb_krylov_lincomb_device); V: (m, n) view with unit column stride, k <= 256."""
    assert V.stride(1) == 1 and y.is_contiguous() and coef.is_contiguous()
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_krylov_lincomb_device(self._h, ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(V.data_ptr()), V.stride(0),
                                                   ctypes.c_void_p(coef.data_ptr()), int(k), y.numel()))

  def krylov_norm_device(self, v, out):
    """out[0] = |v| in one launch of one workgroup (rmb_krylov_norm_device)."""
    assert v.is_contiguous() and out.is_contiguous()
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_krylov_norm_device(self._h, ctypes.c_void_p(v.data_ptr()), v.numel(), ctypes.c_void_p(out.data_ptr())))

  def rigid_arnoldi_step2_device(self, A11, A12, A21, A22, K, V, j, eta, z, w, col, col_mapped=0, z_ready=False, fuse_pc=False):
    """rigid_arnoldi_step_device in the native loop's forms (rmb_rigid_arnoldi_step2_device): z_ready -- z already holds
    P^-1 V[j]; fuse_pc -- the ending also leaves P^-1 V[j + 1] in z."""
    nb, n_b = K.shape[0], K.shape[1] // 3
    for t in (A11, A12, A21, A22, K, z, w, col):
      assert t.is_contiguous()
    assert V.stride(1) == 1
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_arnoldi_step2_device(self._h, nb, n_b, p(A11), p(A12), p(A21), p(A22), p(K), p(V), V.stride(0), int(j),
                                                        float(eta), p(z), p(w), p(col), ctypes.c_void_p(col_mapped) if col_mapped else None,
                                                        int(bool(z_ready)), int(bool(fuse_pc))))

  def rigid_lanczos_step_device(self, Linv, V, i, eta, pv, mw, d, col, col_mapped=0, pv_ready=False, fuse_next=False):
    """One iteration of rigid_lanczos_device's loop (rmb_rigid_lanczos_step_device): pv = P V[i] (unless pv_ready), mw = the
    sweep's result, d = P^T M pv orthogonalised against V[:i + 1], V[i + 1] = d / |d|; fuse_next: pv = P V[i + 1] after it."""
    nb, n_b = Linv.shape[0], Linv.shape[1] // 3
    for t in (Linv, pv, mw, d, col):
      assert t.is_contiguous()
    assert V.stride(1) == 1
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_lanczos_step_device(self._h, nb, n_b, p(Linv), p(V), V.stride(0), int(i), float(eta), p(pv), p(mw), p(d),
                                                       p(col), ctypes.c_void_p(col_mapped) if col_mapped else None, int(bool(pv_ready)),
                                                       int(bool(fuse_next))))

  def lanczos_step_device(self, product, V, i, eta, x1, col, col_mapped=0, in_plane=False):
    """One iteration of lanczos_device's loop (rmb_lanczos_step_device): x1 = M V[i] for product "tt" / "grand", orthogonalised
    against V[:i + 1], V[i + 1] = x1 / |x1|."""
    assert V.stride(1) == 1 and x1.is_contiguous() and col.is_contiguous()
    code = product if isinstance(product, int) else {"tt": 0, "grand": 1}[product]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_lanczos_step_device(self._h, code, int(bool(in_plane)), p(V), V.stride(0), int(i), float(eta), p(x1), p(col),
                                                 ctypes.c_void_p(col_mapped) if col_mapped else None))

  def rigid_gmres_device(self, A11, A12, A21, A22, K, b, tol, restart, maxiter, eta):
    """The whole right-preconditioned GMRES of the rigid-body problem in one library call (rmb_rigid_gmres_device); b is
    the RAW right-hand side (scaled to unit norm inside, the solution scaled back).  Returns (x tensor, info dict as
    krylov.gmres_right_preconditioned, plus rhs_norm)."""
    import torch
    nb, n_b = K.shape[0], K.shape[1] // 3
    for t in (A11, A12, A21, A22, K, b):
      assert t.is_contiguous()
    assert b.numel() == 3 * nb * n_b + 6 * nb
    x = torch.empty_like(b)
    its, disc, prod = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
    res, nrm = ctypes.c_double(0.0), ctypes.c_double(0.0)
    cap = int(maxiter) + 1
    hist = (ctypes.c_double * cap)()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_gmres_device(self._h, nb, n_b, p(A11), p(A12), p(A21), p(A22), p(K), p(b), float(tol), int(restart),
                                                int(maxiter), float(eta), p(x), ctypes.byref(its), ctypes.byref(res), ctypes.byref(disc),
                                                ctypes.byref(prod), hist, cap, ctypes.byref(nrm)))
    k = min(its.value, cap)
    return x, dict(iterations=int(its.value), residual=float(res.value), converged=bool(res.value <= tol), history=list(hist[:k]),
                   discarded_sweeps=int(disc.value), operator_applications=int(prod.value), rhs_norm=float(nrm.value))

  def rigid_lanczos_device(self, Linv, Lchol, z, factor, tol, max_iter, max_rows, eta):
    """The whole preconditioned Lanczos forcing in one library call (rmb_rigid_lanczos_device).  Returns (noise, iterations,
    products) or (None, status, products) when the library hands the forcing back (breakdown, more basis rows needed)."""
    import torch
    nb, n_b = Linv.shape[0], Linv.shape[1] // 3
    assert Linv.is_contiguous() and Lchol.is_contiguous() and z.is_contiguous() and z.numel() == 3 * nb * n_b
    noise = torch.empty_like(z)
    its, prod, status = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_int(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_lanczos_device(self._h, nb, n_b, p(Linv), p(Lchol), p(z), float(factor), float(tol), int(max_iter),
                                                  int(max_rows), float(eta), p(noise), ctypes.byref(its), ctypes.byref(prod),
                                                  ctypes.byref(status)))
    if status.value != 0:
      return None, int(status.value), int(prod.value)
    return noise, int(its.value), int(prod.value)

  def lanczos_device(self, product, z, factor, tol, max_iter, max_rows, eta, in_plane=False):
    """factor * M^{1/2} z in one library call (rmb_lanczos_device): product "tt" (3n entries; in_plane: its in-plane variant) or
    "grand" (6n entries: the grand mobility on [z_f; z_tau]).  Returns (noise, iterations, products), or (None, status,
    products) when the library hands the forcing back (breakdown, more basis rows needed)."""
    import torch
    code = {"tt": 0, "grand": 1}[product]
    assert _is_torch_cuda(z) and z.is_contiguous() and z.numel() == (6 if code else 3) * self.n
    noise = torch.empty_like(z)
    its, prod, status = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_int(0)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_lanczos_device(self._h, code, int(bool(in_plane)), ctypes.c_void_p(z.data_ptr()), float(factor), float(tol),
                                            int(max_iter), int(max_rows), float(eta), ctypes.c_void_p(noise.data_ptr()), ctypes.byref(its),
                                            ctypes.byref(prod), ctypes.byref(status)))
    if status.value != 0:
      return None, int(status.value), int(prod.value)
    return noise, int(its.value), int(prod.value)

  def rigid_operator_device(self, K, x, eta, out):
    """out = [M_tt lambda - K U; -K^T lambda] for x = [lambda; U] on the resident configuration (all bodies free, one body
    shape; rmb_rigid_operator_device): the pair sweep + one finishing launch.  K (n_bodies, 3 n_b, 6) contiguous."""
    nb, n_b = K.shape[0], K.shape[1] // 3
    assert K.is_contiguous() and x.is_contiguous() and out.is_contiguous() and x.numel() == 3 * nb * n_b + 6 * nb == out.numel()
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_rigid_operator_device(self._h, nb, n_b, ctypes.c_void_p(K.data_ptr()), ctypes.c_void_p(x.data_ptr()),
                                                   float(eta), ctypes.c_void_p(out.data_ptr())))
    return out

  def _laplace_args(self, r, weights, p, q, normals):
    import torch
    n = r.numel() // 3
    for name, t, size in (("r", r, 3 * n), ("weights", weights, n), ("p", p, n), ("q", q, n), ("normals", normals, 3 * n)):
      if t is not None and (not _is_torch_cuda(t) or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != size):
        raise ValueError("%s must be a contiguous CUDA float64 tensor with %d entries" % (name, size))
    if p is None and q is None:
      raise ValueError("p and q are both None")
    if p is not None and normals is None:
      raise ValueError("the p term needs the normals")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    return n, ptr(r), ptr(normals), ptr(weights), ptr(p), ptr(q)

  @staticmethod
  def _laplace_out(out, size):
    """A caller's out= goes straight to the kernel: refuse any tensor it could not write in place (as matvec_device)."""
    if not _is_torch_cuda(out) or not out.is_contiguous() or out.numel() != size:
      raise ValueError("out must be a contiguous CUDA float64 tensor with %d entries" % size)

  def laplace_operator_device(self, r, weights, p=None, q=None, normals=None, alpha=0.0, wall=False, out=None):
    """out = alpha p - D[p] + S[q] on the nodes r (3n tensor; Laplace layer operators, rmb_laplace_operator_device) in one
    pass; a None field drops its term (alpha goes with p).  Independent of the bound configuration."""
    import torch
    n, rp, np_, wp, pp, qp = self._laplace_args(r, weights, p, q, normals)
    if out is None:
      out = torch.empty(n, dtype=torch.float64, device=r.device)
    else:
      self._laplace_out(out, n)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_laplace_operator_device(self._h, n, rp, np_, wp, pp, qp, float(alpha), 1 if wall else 0,
                                                     ctypes.c_void_p(out.data_ptr())))
    return out

  def laplace_gradient_device(self, r, weights, p=None, q=None, normals=None, wall=False, out=None):
    """out (3n) = 2 G[p] - 2 P[q] on the nodes r: gradient of the double layer and dipole (rmb_laplace_gradient_device) in
    one pass; a None field drops its term."""
    import torch
    n, rp, np_, wp, pp, qp = self._laplace_args(r, weights, p, q, normals)
    if out is None:
      out = torch.empty(3 * n, dtype=torch.float64, device=r.device)
    else:
      self._laplace_out(out, 3 * n)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_laplace_gradient_device(self._h, n, rp, np_, wp, pp, qp, 1 if wall else 0,
                                                     ctypes.c_void_p(out.data_ptr())))
    return out

  def blob_blob_force(self, repulsion_strength, debye_length, blob_radius):
    out = np.empty(3 * self.n_targets)
    _lib.check(self._lib.rmb_blob_blob_force(self._h, float(repulsion_strength), float(debye_length),
                                             float(blob_radius), _ptr(out)))
    return out.reshape(self.n_targets, 3)

  def blob_blob_force_radii(self, radius_blobs, repulsion_strength, debye_length):
    """One radius per blob (contact distance a_i + a_j, forces_numba.py:73-137); host arrays."""
    rad = _as_f64(radius_blobs, self.n)
    out = np.empty(3 * self.n_targets)
    _lib.check(self._lib.rmb_blob_blob_force_radii(self._h, _ptr(rad), float(repulsion_strength), float(debye_length),
                                                   _ptr(out)))
    return out.reshape(self.n_targets, 3)

  def blob_blob_force_radii_device(self, radius_blobs, repulsion_strength, debye_length, out=None):
    import torch
    if not _is_torch_cuda(radius_blobs) or radius_blobs.numel() != self.n or not radius_blobs.is_contiguous():
      raise ValueError("radius_blobs must be a contiguous CUDA float64 tensor with n entries")
    if out is None:
      out = torch.empty(3 * self.n_targets, dtype=torch.float64, device=radius_blobs.device)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_blob_blob_force_radii_device(self._h, ctypes.c_void_p(radius_blobs.data_ptr()),
                                                          float(repulsion_strength), float(debye_length),
                                                          ctypes.c_void_p(out.data_ptr())))
    return out

  def blob_blob_force_device(self, repulsion_strength, debye_length, blob_radius, out=None, device=None):
    import torch
    if out is None:
      out = torch.empty(3 * self.n_targets, dtype=torch.float64, device=device or ("cuda:%d" % self.device))
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_blob_blob_force_device(self._h, float(repulsion_strength), float(debye_length),
                                                    float(blob_radius), ctypes.c_void_p(out.data_ptr())))
    return out

  def body_body_force(self, repulsion_strength, debye_length):
    """(n, 3) Yukawa forces between the resident points, which the caller has set to the body locations
    (set_positions(..., wall=False)): F_i = sum_j -(eps/b + eps/r) exp(-r/b) (x_j - x_i)/r^2, minimal image in every
    periodic direction (multi_bodies_functions.py:359-408; rmb_body_body_force).  The sweep is always fp64: the
    "force_precision" / "precision" options do not apply."""
    out = np.empty(3 * self.n)
    _lib.check(self._lib.rmb_body_body_force(self._h, float(repulsion_strength), float(debye_length), _ptr(out)))
    return out.reshape(self.n, 3)

  def body_body_force_device(self, repulsion_strength, debye_length, out=None, device=None):
    """The same as a CUDA float64 tensor of 3 n entries, asynchronous on the context's stream
    (rmb_body_body_force_device); a caller's out= goes straight to the kernel.  Always fp64, whatever "force_precision"
    says."""
    import torch
    if out is None:
      out = torch.empty(3 * self.n, dtype=torch.float64, device=device or ("cuda:%d" % self.device))
    elif not _is_torch_cuda(out) or out.dtype != torch.float64 or out.numel() != 3 * self.n or not out.is_contiguous():
      raise ValueError("out must be a contiguous CUDA float64 tensor with 3*n entries")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_body_body_force_device(self._h, float(repulsion_strength), float(debye_length),
                                                    ctypes.c_void_p(out.data_ptr())))
    return out

  def body_body_potential(self, repulsion_strength, debye_length):
    """U_body = sum_{i<j} eps exp(-r_ij/b) / r_ij of the resident points, which the caller has set to the body locations
    (set_positions(..., wall=False)): the energy whose gradient body_body_force is, minimal image in every periodic
    direction (z included), no wall gate, always fp64 (rmb_body_body_potential)."""
    out = np.empty(1)
    _lib.check(self._lib.rmb_body_body_potential(self._h, float(repulsion_strength), float(debye_length), _ptr(out)))
    return float(out[0])

  def body_body_potential_device(self, repulsion_strength, debye_length, out=None, device=None):
    """The same as a CUDA float64 tensor of one entry, asynchronous on the context's stream
    (rmb_body_body_potential_device).  A caller's out= goes straight to the kernel."""
    import torch
    if out is None:
      out = torch.empty(1, dtype=torch.float64, device=device or ("cuda:%d" % self.device))
    elif not _is_torch_cuda(out) or out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 1:
      raise ValueError("out must be a contiguous CUDA float64 tensor with 1 entry")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_body_body_potential_device(self._h, float(repulsion_strength), float(debye_length),
                                                        ctypes.c_void_p(out.data_ptr())))
    return out

  def set_pair_table(self, table):
    """Copies a PairTable (pair_table.py: a radial pair law as K cubics) into the context, replacing the one that was
    there; None clears it (rmb_ctx_set_pair_table).  pair_table_force and blob_potential(..., pair_table=...) run on it."""
    from .pair_table import PairTable
    if table is None:
      _lib.check(self._lib.rmb_ctx_set_pair_table(self._h, 0.0, 1.0, 0, None))
    else:
      if not isinstance(table, PairTable):
        raise ValueError("set_pair_table takes a PairTable or None, got %r" % (type(table).__name__,))
      c = np.ascontiguousarray(table.coeff, dtype=np.float64)
      _lib.check(self._lib.rmb_ctx_set_pair_table(self._h, table.r0, table.h, table.K, _ptr(c)))
    self._pair_table = table

  def _use_pair_table(self, table):
    """pair_table= of a call: make `table` the context's (a copy only when it is not already)."""
    if table is not getattr(self, "_pair_table", None):
      self.set_pair_table(table)

  def pair_table_force(self):
    """(n, 3) blob-blob forces of the context's pair table on the resident raw positions (set_positions(..., wall=False)):
    F_i = sum_j (U'(r)/r) (x_j - x_i), minimal image in every periodic direction; always the symmetric fp64 sweep
    (rmb_pair_table_force)."""
    out = np.empty(3 * self.n)
    _lib.check(self._lib.rmb_pair_table_force(self._h, _ptr(out)))
    return out.reshape(self.n, 3)

  def pair_table_force_device(self, out=None, device=None):
    """The same as a CUDA float64 tensor of 3 n entries, asynchronous on the context's stream
    (rmb_pair_table_force_device); a caller's out= goes straight to the kernel."""
    import torch
    if out is None:
      out = torch.empty(3 * self.n, dtype=torch.float64, device=device or ("cuda:%d" % self.device))
    elif not _is_torch_cuda(out) or out.dtype != torch.float64 or out.numel() != 3 * self.n or not out.is_contiguous():
      raise ValueError("out must be a contiguous CUDA float64 tensor with 3*n entries")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_pair_table_force_device(self._h, ctypes.c_void_p(out.data_ptr())))
    return out

  def pair_histogram(self, r_max, n_bins):
    """Counts of the unordered pairs i < j of the resident points (set_positions(..., wall=False)) per distance bin:
    r < r_max lands in bin int(r / (r_max / n_bins)), r in the minimal image of every periodic direction (z included), fp64
    (rmb_pair_histogram).  numpy uint64 array of n_bins entries: the counts behind g(r) (correlation.RadialDistribution)."""
    out = np.zeros(int(n_bins), dtype=np.uint64)
    _lib.check(self._lib.rmb_pair_histogram(self._h, float(r_max), int(n_bins), _ptr(out) if out.size else None))
    return out

  def _hist_out(self, n_bins, out, device):
    """The out= rules of the histogram entries: a contiguous CUDA int64 tensor of n_bins entries, which is ADDED to (zeros
    when it is made here)."""
    import torch
    if out is None:
      return torch.zeros(max(int(n_bins), 0), dtype=torch.int64, device=device or ("cuda:%d" % self.device))
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() == int(n_bins)):
      raise ValueError("out must be a contiguous CUDA int64 tensor with n_bins entries")
    return out

  def pair_histogram_device(self, r_max, n_bins, out=None, device=None):
    """The same counts ADDED to a CUDA int64 tensor of n_bins entries (out=None: a new tensor of zeros), asynchronous on the
    context's stream (rmb_pair_histogram_device): call it once per frame to accumulate.  A caller's out= goes straight to
    the kernel."""
    out = self._hist_out(n_bins, out, device)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_pair_histogram_device(self._h, float(r_max), int(n_bins), ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out

  def pair_histogram_frames_device(self, frames, periodic_length, r_max, n_bins, out=None):
    """The counts of every frame of `frames` -- a contiguous CUDA float64 tensor (n_frames, n, 3), or (n, 3) for one frame --
    ADDED to a CUDA int64 tensor of n_bins entries in one launch (rmb_pair_histogram_frames_device).  periodic_length:
    three periods (<= 0: open).  The resident configuration is neither read nor changed."""
    if not _is_torch_cuda(frames) or not frames.is_contiguous() or frames.dim() not in (2, 3) or frames.shape[-1] != 3:
      raise ValueError("frames must be a contiguous CUDA float64 tensor of shape (n_frames, n, 3) or (n, 3)")
    n_frames, n = (1, frames.shape[0]) if frames.dim() == 2 else (frames.shape[0], frames.shape[1])
    L = _as_f64(periodic_length, 3)
    out = self._hist_out(n_bins, out, frames.device)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_pair_histogram_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None, int(n_frames),
                                                          int(n), _ptr(L), float(r_max), int(n_bins),
                                                          ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out

  def msd_frames_device(self, frames, n_lags, offsets=None, origins="window", out=None, origin_chunk=0):
    """Sums behind the 6 x 6 mean-square displacement of `frames`, a contiguous CUDA float64 tensor (n_frames, n_bodies, 7) of
    rows x y z s p1 p2 p3 (rmb_msd_frames_device): for every origin o, lag l < n_lags and body, Delta Delta^T with Delta =
    [c(o + l) - c(o); u], c = x + R(q) p_b the tracked point (offsets: (n_bodies, 3) body-frame offsets, CUDA tensor or
    array; None: the body's location) and u the reference's rotational displacement.  Quaternions are used as they are and
    never renormalised.  origins="window": only origins for which all n_lags lags exist (the reference's); "all": lag l uses
    every origin with o + l < n_frames.  The sums are ADDED to out=, a contiguous CUDA float64 tensor (n_lags, 6, 6) (None: a
    new tensor of zeros).  origin_chunk: origins per staged window, 0 = planned.  Returns (sums, counts): counts is a numpy
    int64 array of the number of terms per lag, computed from the shapes.  Asynchronous on torch's stream; the resident
    configuration is neither read nor changed."""
    import torch
    if not _is_torch_cuda(frames) or frames.dtype != torch.float64 or not frames.is_contiguous() or frames.dim() != 3 or frames.shape[-1] != 7:
      raise ValueError("frames must be a contiguous CUDA float64 tensor of shape (n_frames, n_bodies, 7)")
    n_frames, n_bodies, n_lags = int(frames.shape[0]), int(frames.shape[1]), int(n_lags)
    counts, _, o_end = _lag_origins(n_frames, n_bodies, n_lags, origins)
    if offsets is not None:
      if not isinstance(offsets, torch.Tensor):
        offsets = torch.from_numpy(_as_f64(offsets, 3 * n_bodies)).to(frames.device)
      if not (offsets.is_cuda and offsets.dtype == torch.float64 and offsets.is_contiguous() and offsets.numel() == 3 * n_bodies):
        raise ValueError("offsets must hold (n_bodies, 3) float64 values")
    out = _cuda_out(out, (n_lags, 6, 6), "(n_lags, 6, 6)", "float64", frames.device)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_msd_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None, n_frames, n_bodies,
                                               ctypes.c_void_p(offsets.data_ptr()) if offsets is not None and offsets.numel() else None,
                                               n_lags, 0, o_end, int(origin_chunk), ctypes.c_void_p(out.data_ptr())))
    return out, counts

  @staticmethod
  def _scattering_frames(frames):
    import torch
    if not _is_torch_cuda(frames) or frames.dtype != torch.float64 or not frames.is_contiguous() or frames.dim() != 3 or frames.shape[-1] != 3:
      raise ValueError("frames must be a contiguous CUDA float64 tensor of shape (n_frames, n, 3)")
    return int(frames.shape[0]), int(frames.shape[1])

  @staticmethod
  def _scattering_wavevectors(periodic_length, wavevectors):
    L = _as_f64(periodic_length, 3)
    k = np.asarray(wavevectors)
    if k.dtype.kind not in "iu" or k.ndim != 2 or k.shape[1] != 3:
      raise ValueError("wavevectors must be an integer array of shape (K, 3)")
    return L, np.ascontiguousarray(np.clip(k, -2 ** 30, 2 ** 30), dtype=np.int32)      # beyond int32: still beyond what the entry accepts

  def density_modes_frames_device(self, frames, periodic_length, wavevectors, out=None):
    """Density modes rho_k(f) = sum_j exp(-i k . x_j(f)) of `frames`, a contiguous CUDA float64 tensor (n_frames, n, 3)
    (rmb_density_modes_frames_device).  wavevectors: integer array (K, 3) of n, k = 2 pi n_d / L_d; periodic_length: the three
    L_d (a period, or any reference length of an open direction; <= 0 only where every n_d = 0).  Returns a CUDA float64 tensor
    (n_frames, K, 2) of (Re, Im) = (sum cos, -sum sin); out= (that shape, contiguous) is OVERWRITTEN.  Asynchronous on torch's
    stream; the resident configuration is neither read nor changed."""
    n_frames, n = self._scattering_frames(frames)
    L, k = self._scattering_wavevectors(periodic_length, wavevectors)
    K = int(k.shape[0])
    out = _cuda_out(out, (n_frames, K, 2), "(n_frames, K, 2)", "float64", frames.device, zero=False)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_density_modes_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None, n_frames, n,
                                                         _ptr(L), ctypes.c_void_p(k.ctypes.data) if K else None, K,
                                                         ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out

  def scattering_lags_device(self, modes, n_lags, origins="window", out=None, o_begin=0, o_end=None):
    """Collective lag sums C[l, k] = sum_o Re(rho_k(o + l) conj rho_k(o)) of `modes`, a contiguous CUDA float64 tensor
    (n_frames, K, 2) (rmb_scattering_lags_device).  origins="window": only origins for which all n_lags lags exist; "all": lag
    l uses every origin with o + l < n_frames; o_begin / o_end narrow the origins to [o_begin, o_end) (o_end=None: the
    convention's last origin).  The sums are ADDED to out=, a contiguous CUDA float64 tensor (n_lags, K) (None: a new tensor of
    zeros).  Returns (sums, counts): counts is msd.counts_per_lag for ONE point, the number of origins per lag of the whole
    range (the caller's own count where o_begin / o_end are given).  Asynchronous on torch's stream."""
    import torch
    if not _is_torch_cuda(modes) or modes.dtype != torch.float64 or not modes.is_contiguous() or modes.dim() != 3 or modes.shape[-1] != 2:
      raise ValueError("modes must be a contiguous CUDA float64 tensor of shape (n_frames, K, 2)")
    n_frames, K, n_lags = int(modes.shape[0]), int(modes.shape[1]), int(n_lags)
    counts, o_begin, o_end = _lag_origins(n_frames, 1, n_lags, origins, o_begin, o_end)
    out = _cuda_out(out, (n_lags, K), "(n_lags, K)", "float64", modes.device)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_scattering_lags_device(self._h, ctypes.c_void_p(modes.data_ptr()) if modes.numel() else None, n_frames, K, n_lags,
                                                    o_begin, o_end, ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out, counts

  def self_scattering_frames_device(self, frames, periodic_length, wavevectors, n_lags, origins="window", out=None, o_begin=0, o_end=None):
    """Self lag sums Sf[l, k] = sum_o sum_j cos(k . (x_j(o + l) - x_j(o))) of `frames`, a contiguous CUDA float64 tensor
    (n_frames, n, 3) (rmb_self_scattering_frames_device); wavevectors and periodic_length as density_modes_frames_device,
    origins, o_begin, o_end and out= (n_lags, K), ADDED to, as scattering_lags_device.  Returns (sums, counts), counts the
    origins per lag as there (a lag's sum has n times as many terms).  Asynchronous on torch's stream; the resident configuration is neither
    read nor changed."""
    n_frames, n = self._scattering_frames(frames)
    L, k = self._scattering_wavevectors(periodic_length, wavevectors)
    K, n_lags = int(k.shape[0]), int(n_lags)
    counts, o_begin, o_end = _lag_origins(n_frames, 1, n_lags, origins, o_begin, o_end)
    out = _cuda_out(out, (n_lags, K), "(n_lags, K)", "float64", frames.device)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_self_scattering_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None, n_frames, n,
                                                           _ptr(L), ctypes.c_void_p(k.ctypes.data) if K else None, K, n_lags, o_begin,
                                                           o_end, ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out, counts

  def _van_hove_args(self, frames, n_lags, r_max, n_bins, origins, plane, out, o_begin, o_end):
    """Checks shared by the two van Hove entries -> (n_frames, n, n_lags, plane index, out, o_begin, o_end)."""
    n_frames, n = self._scattering_frames(frames)
    n_lags, n_bins = int(n_lags), int(n_bins)
    _, o_begin, o_end = _lag_origins(n_frames, 1, n_lags, origins, o_begin, o_end)
    if plane not in VAN_HOVE_PLANES:
      raise ValueError("plane must be one of %s, got %r" % (sorted(VAN_HOVE_PLANES), plane))
    out = _cuda_out(out, (n_lags, max(n_bins, 0)), "(n_lags, n_bins)", "int64", frames.device)
    return n_frames, n, n_lags, VAN_HOVE_PLANES[plane], out, o_begin, o_end

  def van_hove_self_frames_device(self, frames, n_lags, r_max, n_bins, origins="window", plane="xyz", out=None, moments=None, o_begin=0,
                                  o_end=None):
    """Counts behind the self part G_s(r, t) of the van Hove function of `frames`, a contiguous CUDA float64 tensor
    (n_frames, n, 3), possibly unwrapped (rmb_van_hove_self_frames_device): hist[l, b] = number of (origin o, point j) whose
    displacement |x_j(o + l) - x_j(o)| -- as it is, no minimal image -- falls in bin int(r n_bins / r_max), r < r_max; and
    moments[l] = (sum r^2, sum r^4) over ALL terms, those beyond r_max included.  plane="xy" ignores the z component.
    origins, o_begin and o_end as scattering_lags_device.  Both are ADDED to out= (contiguous CUDA int64 (n_lags, n_bins)) and
    moments= (contiguous CUDA float64 (n_lags, 2)); None: new tensors of zeros.  Returns (hist, moments).  Asynchronous on
    torch's stream; the resident configuration is neither read nor changed."""
    n_frames, n, n_lags, pl, out, o_begin, o_end = self._van_hove_args(frames, n_lags, r_max, n_bins, origins, plane, out, o_begin, o_end)
    moments = _cuda_out(moments, (n_lags, 2), "(n_lags, 2)", "float64", frames.device, what="moments")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_van_hove_self_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None, n_frames, n,
                                                         n_lags, o_begin, o_end, pl, float(r_max), int(n_bins),
                                                         ctypes.c_void_p(out.data_ptr()) if out.numel() else None,
                                                         ctypes.c_void_p(moments.data_ptr())))
    return out, moments

  def van_hove_distinct_frames_device(self, frames, periodic_length, n_lags, r_max, n_bins, origins="window", plane="xyz", out=None, o_begin=0,
                                      o_end=None):
    """Counts behind the distinct part G_d(r, t): hist[l, b] = number of (origin o, ORDERED pair i != j) whose separation
    x_i(o + l) - x_j(o), in the minimal image of every direction with a positive period (periodic_length: three periods, <= 0:
    open), has its length in bin b (rmb_van_hove_distinct_frames_device).  Binning, plane, origins, o_begin, o_end and out= as
    van_hove_self_frames_device; hist[0] summed over origins is twice pair_histogram_frames_device's counts.  Returns hist."""
    n_frames, n, n_lags, pl, out, o_begin, o_end = self._van_hove_args(frames, n_lags, r_max, n_bins, origins, plane, out, o_begin, o_end)
    L = _as_f64(periodic_length, 3)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_van_hove_distinct_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None, n_frames,
                                                             n, _ptr(L), n_lags, o_begin, o_end, pl, float(r_max), int(n_bins),
                                                             ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out

  def bond_order_frames_device(self, frames, periodic_length, r_cut, orders=(6,), plane="xy", out=None, source_chunk=0):
    """Neighbour sums behind the bond-orientational order psi_m(i) of `frames`, a contiguous CUDA float64 tensor (n_frames, n, 3),
    possibly unwrapped (rmb_bond_order_frames_device).  The neighbours of point i are the j with d_ij < r_cut -- in the minimal
    image of every direction with a positive period (periodic_length: three periods, <= 0: open), d the in-plane distance under
    plane="xy" and the 3-D one under "xyz" -- and rho_ij > 0 (a point stacked on i has no bond angle).  orders: 1 ... 4 values m
    in 1 ... 16.  Returns a CUDA float64 tensor (n_frames, n, 1 + 2 K) of [N_i, Re sum z^m1, Im sum z^m1, ...], z = (dx + i dy) /
    rho; out= (that shape, contiguous) is OVERWRITTEN.  psi_m(i) = sum / N_i.  source_chunk: sources per chunk of the sweep, 0 =
    planned.  Asynchronous on torch's stream; the resident configuration is neither read nor changed."""
    n_frames, n = self._scattering_frames(frames)
    L = _as_f64(periodic_length, 3)
    if plane not in VAN_HOVE_PLANES:
      raise ValueError("plane must be one of %s, got %r" % (sorted(VAN_HOVE_PLANES), plane))
    m = np.asarray(orders).reshape(-1)
    if m.dtype.kind not in "iu" or not 1 <= m.size <= 4 or np.any(m < 1) or np.any(m > 16):
      raise ValueError("orders must be 1 ... 4 integers in 1 ... 16, got %r" % (orders,))
    m = np.ascontiguousarray(m, dtype=np.int32)
    K = int(m.size)
    out = _cuda_out(out, (n_frames, n, 1 + 2 * K), "(n_frames, n, 1 + 2 K)", "float64", frames.device, zero=False)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_bond_order_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None, n_frames, n,
                                                      _ptr(L), float(r_cut), VAN_HOVE_PLANES[plane], ctypes.c_void_p(m.ctypes.data), K,
                                                      int(source_chunk), ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out

  def pair_field_correlation_frames_device(self, frames, field, periodic_length, r_max, n_bins, plane="xy", counts=None, sums=None):
    """Pair correlation of a quantised per-point field over the unordered pairs of every frame (rmb_pair_field_frames_device).
    frames: contiguous CUDA float64 (n_frames, n, 3); field: contiguous CUDA int32 (n_frames, n, 2) of (a, b) = rint(psi 2^30),
    |a|, |b| <= 2^30 (bondorder.quantise).  For every pair with r < r_max (plane and periodic_length as
    bond_order_frames_device, binning as pair_histogram_frames_device): counts[bin] += 1, sums[bin] += (a_i a_j + b_i b_j +
    2^29) >> 30.  Both are contiguous CUDA int64 tensors of n_bins entries, ADDED to (None: new tensors of zeros); n_bins <=
    4096.  Returns (counts, sums): integer sums, the same bits for every point order and every cut of the trajectory.
    Asynchronous on torch's stream; the resident configuration is neither read nor changed."""
    import torch
    n_frames, n = self._scattering_frames(frames)
    if not (isinstance(field, torch.Tensor) and field.is_cuda and field.dtype == torch.int32 and field.is_contiguous() and tuple(field.shape) == (n_frames, n, 2)):
      raise ValueError("field must be a contiguous CUDA int32 tensor of shape (n_frames, n, 2)")
    L = _as_f64(periodic_length, 3)
    if plane not in VAN_HOVE_PLANES:
      raise ValueError("plane must be one of %s, got %r" % (sorted(VAN_HOVE_PLANES), plane))
    n_bins = int(n_bins)
    counts = _cuda_out(counts, (max(n_bins, 0),), "(n_bins,)", "int64", frames.device, what="counts")
    sums = _cuda_out(sums, (max(n_bins, 0),), "(n_bins,)", "int64", frames.device, what="sums")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_pair_field_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None,
                                                      ctypes.c_void_p(field.data_ptr()) if field.numel() else None, n_frames, n, _ptr(L),
                                                      VAN_HOVE_PLANES[plane], float(r_max), n_bins,
                                                      ctypes.c_void_p(counts.data_ptr()) if counts.numel() else None,
                                                      ctypes.c_void_p(sums.data_ptr()) if sums.numel() else None))
    return counts, sums

  @staticmethod
  def _cluster_args(n_frames, n, plane, select, labels, sizes, device, shape, named):
    """Checks shared by the two cluster entries -> (plane index, select as uint8 or None, labels, sizes)."""
    import torch
    if plane not in VAN_HOVE_PLANES:
      raise ValueError("plane must be one of %s, got %r" % (sorted(VAN_HOVE_PLANES), plane))
    if n_frames * n > 2 ** 31 - 1:
      raise ValueError("n_frames * n must not exceed 2^31 - 1 per call, got %d" % (n_frames * n))
    if select is not None:
      if not (isinstance(select, torch.Tensor) and select.is_cuda and select.dtype in (torch.bool, torch.uint8) and select.is_contiguous() and
              tuple(select.shape) == tuple(shape)):
        raise ValueError("select must be a contiguous CUDA bool or uint8 tensor of shape %s" % named)
      if select.dtype == torch.bool:
        select = select.view(torch.uint8)      # one byte per point, 0 or 1: no copy
    labels = _cuda_out(labels, shape, named, "int32", device, what="labels", zero=False)
    sizes = _cuda_out(sizes, shape, named, "int32", device, what="sizes", zero=False)
    return VAN_HOVE_PLANES[plane], select, labels, sizes

  def cluster_labels_frames_device(self, frames, periodic_length, r_cut, plane="xyz", select=None, labels=None, sizes=None):
    """Connected components of the bond graph of every frame of `frames` -- a contiguous CUDA float64 tensor (n_frames, n, 3), or
    (n, 3) for one frame, possibly unwrapped (rmb_cluster_labels_frames_device).  Points i and j of a frame are bonded when
    d_ij < r_cut, strictly, in the minimal image of every direction with a positive period (periodic_length: three periods, <= 0:
    open); plane="xyz": the 3-D distance, "xy": the in-plane one (z and L_z ignored).  Coincident, and under "xy" stacked, points
    are bonded.  select: a CUDA bool or uint8 tensor (n_frames, n) ((n,) for one frame), non-zero = selected; only bonds between
    two selected points exist.  Returns (labels, sizes), CUDA int32 tensors of that shape, OVERWRITTEN when given: labels[f, i] =
    the smallest index of the cluster of point i (-1: unselected), sizes[f, l] = the size of the cluster labelled l (0 where l is
    nobody's label).  Integers that do not depend on the launch plan, the point order or the cut of the trajectory; n_frames * n
    <= 2^31 - 1 per call (clusters.Clusters cuts its batches).  Asynchronous on torch's stream; the resident configuration is
    neither read nor changed."""
    if not _is_torch_cuda(frames) or not frames.is_contiguous() or frames.dim() not in (2, 3) or frames.shape[-1] != 3:
      raise ValueError("frames must be a contiguous CUDA float64 tensor of shape (n_frames, n, 3) or (n, 3)")
    shape = tuple(int(s) for s in frames.shape[:-1])
    n_frames, n = (1, shape[0]) if frames.dim() == 2 else shape
    L = _as_f64(periodic_length, 3)
    pl, select, labels, sizes = self._cluster_args(n_frames, n, plane, select, labels, sizes, frames.device, shape,
                                                   "(n_frames, n)" if frames.dim() == 3 else "(n,)")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_cluster_labels_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None,
                                                          ctypes.c_void_p(select.data_ptr()) if select is not None and select.numel() else None,
                                                          n_frames, n, _ptr(L), float(r_cut), pl,
                                                          ctypes.c_void_p(labels.data_ptr()) if labels.numel() else None,
                                                          ctypes.c_void_p(sizes.data_ptr()) if sizes.numel() else None))
    return labels, sizes

  def cluster_labels_device(self, r_cut, plane="xyz", select=None, labels=None, sizes=None):
    """The same for the resident points (set_positions(..., wall=False); rmb_cluster_labels_device), with the context's periods:
    (labels, sizes), CUDA int32 tensors of n entries in the caller's order.  The sweep runs on the Morton-sorted copy and skips
    tile pairs further apart than r_cut (options "force_sort", "force_cull"; under "xy" the gap ignores z), which changes no
    label."""
    n = int(self.n)
    pl, select, labels, sizes = self._cluster_args(1, n, plane, select, labels, sizes, "cuda:%d" % self.device, (n,), "(n,)")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_cluster_labels_device(self._h, ctypes.c_void_p(select.data_ptr()) if select is not None and select.numel() else None,
                                                   float(r_cut), pl, ctypes.c_void_p(labels.data_ptr()) if labels.numel() else None,
                                                   ctypes.c_void_p(sizes.data_ptr()) if sizes.numel() else None))
    return labels, sizes

  @staticmethod
  def _hydro_args(a, periodic_length, wavevectors, polarisation, in_plane, shard, nshards):
    """Checks shared by the two hydrodynamic-function entries -> (L, kint (K, 3) int32, pol (K, 3) float64)."""
    if in_plane:
      raise ValueError("the hydrodynamic function has no in_plane variant")
    if int(shard) != 0 or int(nshards) != 1:
      raise ValueError("the hydrodynamic function does not take pair shards (shard = 0, nshards = 1)")
    if a is not None and np.ndim(a) != 0:
      raise ValueError("the hydrodynamic function takes one radius, not per-blob radii")
    L, k = MobilityContext._scattering_wavevectors(periodic_length, wavevectors)
    pol = np.ascontiguousarray(polarisation, dtype=np.float64)
    if pol.shape != (k.shape[0], 3):
      raise ValueError("polarisation must be a float array of shape (K, 3), one vector per wavevector")
    return L, k, pol

  def hydrodynamic_function_frames_device(self, frames, a, eta, periodic_length, wavevectors, polarisation, wall=True,
                                          mobility_periodic_length=None, out=None, in_plane=False, shard=0, nshards=1):
    """Raw sums behind the hydrodynamic function H(k; e) = (1 / (N mu0)) sum_ij e^T M_ij e cos(k . (x_i - x_j)) of every frame of
    `frames`, a contiguous CUDA float64 tensor (n_frames, n, 3) (rmb_hydro_function_frames_device).  M is the matrix of the tt
    product for blobs of radius `a` in a fluid of viscosity `eta`: wall=True the single-wall block (heights clamped to a, blobs
    below a damped by z / a, as set_positions packs them), False the unbounded RPY block; mobility_periodic_length: the three
    pseudo-periodic lengths of the mobility (None or <= 0: open).  wavevectors: integer array (K, 3) of n, k = 2 pi n_d /
    L_d with periodic_length = the three L_d, as density_modes_frames_device; where the mobility is periodic its period must be
    that L_d.  polarisation: (K, 3) floats, the vector e of every wavevector (hydrofunction.polarisations makes unit vectors).
    Returns a CUDA float64 tensor (n_frames, K, 2) of (S_self, S_dist) = (sum_i b_i^2 e^T M_ii e, 2 sum_{i<j} b_i b_j e^T M_ij e
    cos(theta_i - theta_j)); out= (that shape, contiguous) is OVERWRITTEN.  H = (S_self + S_dist) 6 pi eta a / n.  The same
    call gives the same bits.  fp64, one radius; no in_plane variant, no pair shards, no free surface.  Asynchronous on torch's
    stream; the resident configuration is neither read nor changed."""
    if isinstance(wall, str):
      raise ValueError("the hydrodynamic function knows a no-slip wall (True) or none (False), not %r" % (wall,))
    n_frames, n = self._scattering_frames(frames)
    L, k, pol = self._hydro_args(a, periodic_length, wavevectors, polarisation, in_plane, shard, nshards)
    mob_L = _as_f64(np.zeros(3) if mobility_periodic_length is None else mobility_periodic_length, 3)
    K = int(k.shape[0])
    out = _cuda_out(out, (n_frames, K, 2), "(n_frames, K, 2)", "float64", frames.device, zero=False)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_hydro_function_frames_device(self._h, ctypes.c_void_p(frames.data_ptr()) if frames.numel() else None, n_frames, n,
                                                          float(a), float(eta), int(bool(wall)), _ptr(mob_L), _ptr(L),
                                                          ctypes.c_void_p(k.ctypes.data) if K else None,
                                                          ctypes.c_void_p(pol.ctypes.data) if K else None, K,
                                                          ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out

  def hydrodynamic_function(self, eta, periodic_length, wavevectors, polarisation, in_plane=False, shard=0, nshards=1):
    """The same two sums for the resident configuration (set_positions with wall True or False), with its own radius, boundary
    and periods, through the same kernel as one frame (rmb_hydro_function_device): a numpy array (K, 2).  Synchronous.  A
    free-surface configuration, a target sub-range and option "precision" = 32 are refused."""
    import torch
    L, k, pol = self._hydro_args(None, periodic_length, wavevectors, polarisation, in_plane, shard, nshards)
    K = int(k.shape[0])
    out = torch.empty((K, 2), dtype=torch.float64, device="cuda:%d" % self.device)
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_hydro_function_device(self._h, float(eta), _ptr(L), ctypes.c_void_p(k.ctypes.data) if K else None,
                                                   ctypes.c_void_p(pol.ctypes.data) if K else None, K,
                                                   ctypes.c_void_p(out.data_ptr()) if out.numel() else None))
    return out.cpu().numpy()

  @staticmethod
  def _body_law(body_potential):
    """(eps, b) of the body_potential= keyword of the single-body moves, as two floats."""
    try:
      eps, b = (float(x) for x in body_potential)
    except (TypeError, ValueError):
      raise ValueError("body_potential must be (repulsion_strength, debye_length), got %r" % (body_potential,))
    if not b > 0.0:
      raise ValueError("body_potential: debye_length must be positive, got %r" % (b,))
    return eps, b

  def _potential_args(self, repulsion_strength, debye_length, repulsion_strength_wall, debye_length_wall, weight, blob_radius, potential):
    if potential not in POTENTIAL_FORMS:
      raise ValueError("potential must be one of %s, got %r" % (sorted(POTENTIAL_FORMS), potential))
    eps_w = float(repulsion_strength_wall or 0.0)
    return (float(repulsion_strength), float(debye_length), eps_w, float(debye_length_wall) if eps_w != 0.0 else 1.0, float(weight),
            float(blob_radius), POTENTIAL_FORMS[potential])

  def blob_potential(self, repulsion_strength, debye_length, blob_radius, repulsion_strength_wall=0.0, debye_length_wall=1.0, weight=0.0,
                     potential="soft", pair_table=None):
    """(U_one_blob, U_pair) of the resident raw positions (set_positions(..., wall=False)): the equilibrium sampler's energy,
    many_body_potential_pycuda.py:15-119 ("soft") or the boomerang example's Yukawa form ("yukawa"); rmb_blob_potential.
    pair_table=T (a PairTable): the pair term is T's (repulsion_strength and debye_length are not read), `potential`
    still chooses the one-blob form; T becomes the context's table (rmb_blob_potential_table)."""
    out = np.empty(2)
    if pair_table is not None:
      self._use_pair_table(pair_table)
      args = self._potential_args(0.0, 1.0, repulsion_strength_wall, debye_length_wall, weight, blob_radius, potential)
      _lib.check(self._lib.rmb_blob_potential_table(self._h, *args[2:], _ptr(out)))
      return float(out[0]), float(out[1])
    _lib.check(self._lib.rmb_blob_potential(self._h, *self._potential_args(repulsion_strength, debye_length, repulsion_strength_wall,
                                                                          debye_length_wall, weight, blob_radius, potential), _ptr(out)))
    return float(out[0]), float(out[1])

  def blob_potential_device(self, repulsion_strength, debye_length, blob_radius, repulsion_strength_wall=0.0, debye_length_wall=1.0,
                            weight=0.0, potential="soft", out=None, device=None, pair_table=None):
    """The same two sums as a CUDA float64 tensor of two entries, asynchronous on the context's stream
    (rmb_blob_potential_device; pair_table=T: rmb_blob_potential_table_device).  A caller's out= goes straight to the kernel."""
    import torch
    if pair_table is not None:
      repulsion_strength, debye_length = 0.0, 1.0
    args = self._potential_args(repulsion_strength, debye_length, repulsion_strength_wall, debye_length_wall, weight, blob_radius, potential)
    if out is None:
      out = torch.empty(2, dtype=torch.float64, device=device or ("cuda:%d" % self.device))
    elif not _is_torch_cuda(out) or not out.is_contiguous() or out.numel() != 2:
      raise ValueError("out must be a contiguous CUDA float64 tensor with 2 entries")
    self._follow_torch_stream()
    if pair_table is not None:
      self._use_pair_table(pair_table)
      _lib.check(self._lib.rmb_blob_potential_table_device(self._h, *args[2:], ctypes.c_void_p(out.data_ptr())))
      return out
    _lib.check(self._lib.rmb_blob_potential_device(self._h, *args, ctypes.c_void_p(out.data_ptr())))
    return out

  def mcmc_propose_device(self, blob_body, blob_ref, ref, loc, quat, draws, n_free, max_angle_shift, loc_new, quat_new, r_new):
    """One Metropolis proposal for every body and the proposed blob coordinates in one launch (rmb_mcmc_propose_device)."""
    import torch
    for name, t in (("blob_body", blob_body), ("blob_ref", blob_ref)):
      if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous CUDA int32 tensor" % name)
    for name, t in (("ref", ref), ("loc", loc), ("quat", quat), ("draws", draws), ("loc_new", loc_new), ("quat_new", quat_new), ("r_new", r_new)):
      if not _is_torch_cuda(t) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous CUDA float64 tensor" % name)
    nb, n_blobs = loc.numel() // 3, blob_body.numel()
    sizes = (("blob_ref", blob_ref, n_blobs), ("loc", loc, 3 * nb), ("quat", quat, 4 * nb), ("draws", draws, 6 * nb), ("loc_new", loc_new, 3 * nb),
             ("quat_new", quat_new, 4 * nb), ("r_new", r_new, 3 * n_blobs))
    for name, t, size in sizes:
      if t.numel() != size:
        raise ValueError("%s must have %d entries, has %d" % (name, size, t.numel()))
    if ref.numel() % 3 or not 0 <= int(n_free) <= nb:
      raise ValueError("ref must be (rows, 3) and 0 <= n_free <= n_bodies")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_mcmc_propose_device(self._h, nb, int(n_free), n_blobs, p(blob_body), p(blob_ref), p(ref), p(loc), p(quat), p(draws),
                                                 float(max_angle_shift), p(loc_new), p(quat_new), p(r_new)))

  def mcmc_body_delta_device(self, r, first, count, body_new, periodic_length, repulsion_strength, debye_length, blob_radius,
                             repulsion_strength_wall=0.0, debye_length_wall=1.0, weight=0.0, potential="soft", out=None,
                             body_potential=None, locations=None, body=None, location_new=None):
    """{U_one(r') - U_one(r), U_pair(r') - U_pair(r)} as a CUDA float64 tensor of two entries, r' = r (n x 3 CUDA tensor, the
    caller's coordinates -- the resident configuration is not involved) with the rows [first, first + count) replaced by
    body_new (count x 3): rmb_mcmc_body_delta_device, asynchronous on the context's stream.
    body_potential=(eps, b) with locations= (n_bodies x 3 CUDA tensor), body= (index of the moved body) and location_new=
    (3 entries, CUDA): three entries, the third the difference of the body-body energy of the locations
    (rmb_mcmc_body_delta_bb_device)."""
    import torch
    n_out = 2 if body_potential is None else 3
    args = self._potential_args(repulsion_strength, debye_length, repulsion_strength_wall, debye_length_wall, weight, blob_radius, potential)
    for name, t in (("r", r), ("body_new", body_new)):
      if not _is_torch_cuda(t) or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() % 3:
        raise ValueError("%s must be a contiguous CUDA float64 tensor of (rows, 3)" % name)
    n, first, count = r.numel() // 3, int(first), int(count)
    if not (0 <= first and 0 < count and first + count <= n) or body_new.numel() != 3 * count:
      raise ValueError("the body's blob range [first, first + count) must lie inside r and body_new must have count rows")
    if out is None:
      out = torch.empty(n_out, dtype=torch.float64, device=r.device)
    elif not _is_torch_cuda(out) or out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != n_out:
      raise ValueError("out must be a contiguous CUDA float64 tensor with %d entries" % n_out)
    L = _as_f64(np.zeros(3) if periodic_length is None else periodic_length, 3)
    self._follow_torch_stream()
    if body_potential is not None:
      body_eps, body_b = self._body_law(body_potential)
      for name, t in (("locations", locations), ("location_new", location_new)):
        if not _is_torch_cuda(t) or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() % 3 or t.numel() == 0:
          raise ValueError("%s must be a contiguous CUDA float64 tensor of (rows, 3)" % name)
      nb = locations.numel() // 3
      if body is None or not 0 <= int(body) < nb or location_new.numel() != 3:
        raise ValueError("body must index a row of locations and location_new must have 3 entries")
      _lib.check(self._lib.rmb_mcmc_body_delta_bb_device(self._h, n, ctypes.c_void_p(r.data_ptr()), first, count, ctypes.c_void_p(body_new.data_ptr()),
                                                         nb, ctypes.c_void_p(locations.data_ptr()), int(body),
                                                         ctypes.c_void_p(location_new.data_ptr()), _ptr(L), *args, body_eps, body_b,
                                                         ctypes.c_void_p(out.data_ptr())))
      return out
    _lib.check(self._lib.rmb_mcmc_body_delta_device(self._h, n, ctypes.c_void_p(r.data_ptr()), first, count, ctypes.c_void_p(body_new.data_ptr()),
                                                    _ptr(L), *args, ctypes.c_void_p(out.data_ptr())))
    return out

  def mcmc_sweep_device(self, body_first, blob_ref, ref, loc, quat, r, draws, n_free, max_angle_shift, periodic_length, kT, energy, accepted,
                        repulsion_strength, debye_length, blob_radius, repulsion_strength_wall=0.0, debye_length_wall=1.0, weight=0.0,
                        potential="soft", body_potential=None):
    """One sweep of single-body Metropolis moves over bodies 0 ... n_free - 1, decided and committed on the device
    (rmb_mcmc_sweep_device): loc, quat, r (current blob coordinates) and energy = {U_one, U_pair} (running) are updated in
    place, accepted[k] (int32) is the flag of move k; draws is (n_free, 7).  body_first: host table of n_bodies + 1 blob
    offsets.  Asynchronous on the context's stream: read the flags and the energy afterwards.
    body_potential=(eps, b): the body-body energy of the locations `loc` takes part (rmb_mcmc_sweep_bb_device) and energy is
    {U_one, U_pair, U_body}, three entries."""
    import torch
    n_energy = 2 if body_potential is None else 3
    args = self._potential_args(repulsion_strength, debye_length, repulsion_strength_wall, debye_length_wall, weight, blob_radius, potential)
    body_first = np.ascontiguousarray(body_first, dtype=np.int64).reshape(-1)
    nb, n_blobs, n_free = loc.numel() // 3, r.numel() // 3, int(n_free)
    if body_first.size != nb + 1 or not 0 <= n_free <= nb:
      raise ValueError("body_first must have n_bodies + 1 entries and 0 <= n_free <= n_bodies")
    if not (isinstance(blob_ref, torch.Tensor) and blob_ref.is_cuda and blob_ref.dtype == torch.int32 and blob_ref.is_contiguous()):
      raise ValueError("blob_ref must be a contiguous CUDA int32 tensor")
    if not (isinstance(accepted, torch.Tensor) and accepted.is_cuda and accepted.dtype == torch.int32 and accepted.is_contiguous()):
      raise ValueError("accepted must be a contiguous CUDA int32 tensor")
    for name, t in (("ref", ref), ("loc", loc), ("quat", quat), ("r", r), ("draws", draws), ("energy", energy)):
      if not _is_torch_cuda(t) or t.dtype != torch.float64 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous CUDA float64 tensor" % name)
    sizes = (("blob_ref", blob_ref, n_blobs, False), ("loc", loc, 3 * nb, False), ("quat", quat, 4 * nb, False), ("r", r, 3 * n_blobs, False),
             ("draws", draws, 7 * n_free, True), ("energy", energy, n_energy, False), ("accepted", accepted, n_free, True))
    for name, t, size, at_least in sizes:
      if t.numel() < size or (not at_least and t.numel() != size):
        raise ValueError("%s must have %d entries, has %d" % (name, size, t.numel()))
    if ref.numel() % 3:
      raise ValueError("ref must be (rows, 3)")
    L = _as_f64(np.zeros(3) if periodic_length is None else periodic_length, 3)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    self._follow_torch_stream()
    if body_potential is not None:
      body_eps, body_b = self._body_law(body_potential)
      _lib.check(self._lib.rmb_mcmc_sweep_bb_device(self._h, nb, n_free, n_blobs, _ptr(body_first), p(blob_ref), p(ref), p(loc), p(quat), p(r), p(draws),
                                                    float(max_angle_shift), _ptr(L), *args, body_eps, body_b, float(kT), p(energy), p(accepted)))
      return
    _lib.check(self._lib.rmb_mcmc_sweep_device(self._h, nb, n_free, n_blobs, _ptr(body_first), p(blob_ref), p(ref), p(loc), p(quat), p(r), p(draws),
                                               float(max_angle_shift), _ptr(L), *args, float(kT), p(energy), p(accepted)))

  def one_blob_force_device(self, r, blob_radius, weight, eps_wall, debye_wall, out=None):
    """(0, 0, -weight + wall repulsion) per blob on the caller's coordinates r (n x 3 CUDA tensor; rmb_one_blob_force_device);
    `out` given = accumulate into it, None = a new tensor."""
    import torch
    assert _is_torch_cuda(r) and r.is_contiguous() and r.dtype == torch.float64
    n = r.numel() // 3
    acc = out is not None
    if out is None:
      out = torch.empty(3 * n, dtype=torch.float64, device=r.device)
    assert out.is_contiguous() and out.numel() == 3 * n
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_one_blob_force_device(self._h, n, ctypes.c_void_p(r.data_ptr()), float(blob_radius), float(weight), float(eps_wall),
                                                   float(debye_wall) if eps_wall != 0.0 else 1.0, 1 if acc else 0, ctypes.c_void_p(out.data_ptr())))
    return out

  def blob_blob_force_pairshard_device(self, repulsion_strength, debye_length, blob_radius, shard, nshards, out=None, device=None):
    """Contribution of pair shard `shard` of `nshards` to the forces on ALL blobs (3n entries; sum over shards = forces)."""
    import torch
    if out is None:
      out = torch.empty(3 * self.n, dtype=torch.float64, device=device or ("cuda:%d" % self.device))
    elif not _is_torch_cuda(out) or out.numel() != 3 * self.n or not out.is_contiguous():
      raise ValueError("out must be a contiguous CUDA float64 tensor with 3*n entries")
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_blob_blob_force_pairshard_device(self._h, float(repulsion_strength), float(debye_length),
                                                              float(blob_radius), ctypes.c_void_p(out.data_ptr()), int(shard),
                                                              int(nshards)))
    return out

  # --- measurement -----------------------------------------------------------------------------
  def timing_collect(self, max_n=8192):
    buf = (ctypes.c_double * max_n)()
    n = self._lib.rmb_timing_collect(self._h, buf, max_n)
    if n < 0:
      _lib.check(n)
    return np.array(buf[:n])

  def wave_clock_collect(self, max_waves=8192):
    """(n_waves, 2) array of start/end wall-clock stamps (100 MHz ticks) of the last symmetric launch."""
    buf = np.zeros((max_waves, 2), dtype=np.int64)
    n = self._lib.rmb_wave_clock_collect(self._h, ctypes.c_void_p(buf.ctypes.data), max_waves)
    if n < 0:
      _lib.check(n)
    return buf[:n]

  def ubench_fp64_issue(self, launches=40):
    """G wave-instructions/s of independent v_fma_f64 on this chip right now (rmb_ubench_fp64_issue)."""
    out = ctypes.c_double()
    self._follow_torch_stream()
    _lib.check(self._lib.rmb_ubench_fp64_issue(self._h, int(launches), ctypes.byref(out)))
    return float(out.value)

  def last_host_timing(self):
    """Host wall clock (us) of the last matvec() on this context: upload, launch, wait + download, whole C call."""
    buf = (ctypes.c_double * 4)()
    _lib.check(self._lib.rmb_last_host_timing(self._h, buf))
    return dict(upload_us=buf[0], launch_us=buf[1], wait_and_download_us=buf[2], c_call_us=buf[3])

  def timing_reset(self):
    _lib.check(self._lib.rmb_timing_reset(self._h))

  def last_launch(self):
    t, c, w = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    _lib.check(self._lib.rmb_last_launch(self._h, ctypes.byref(t), ctypes.byref(c), ctypes.byref(w)))
    return dict(tiles=t.value, chunks=c.value, workgroups=w.value)

  def synchronize(self):
    _lib.check(self._lib.rmb_ctx_synchronize(self._h))


_raw_stream = None


def _current_raw_stream(device_index):
  """hipStream_t of torch's current stream on `device_index`, as an int.  Every *_device call asks for it, so the cheap
  accessor is used when this torch has it (0.3 us; torch.cuda.current_stream() builds a Stream object: 3.5 us, a third
  of a small product's launch cost)."""
  global _raw_stream
  if _raw_stream is None:
    import torch
    fast = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if fast is not None:
      _raw_stream = fast
    else:
      _raw_stream = lambda idx: torch.cuda.current_stream(torch.device("cuda", idx)).cuda_stream   # noqa: E731
  return _raw_stream(device_index)


def _is_torch_cuda(x):
  try:
    import torch
  except ImportError:
    return False
  return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64


class MappedHostArray(object):
  """A float64 numpy array in page-locked host memory that is mapped into the device's address space
  (rmb_host_mapped_alloc): kernels store into `dev_ptr`, the host reads `array` after one event / stream wait -- no copy
  command.  Freed with close() or when collected."""

  def __init__(self, shape):
    self._lib = _lib.load()
    n = int(np.prod(shape))
    h, d = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(self._lib.rmb_host_mapped_alloc(ctypes.c_size_t(8 * n), ctypes.byref(h), ctypes.byref(d)))
    self._host = h
    self.dev_ptr = int(d.value)
    self.array = np.ctypeslib.as_array((ctypes.c_double * n).from_address(h.value)).reshape(shape)

  def close(self):
    if self._host is not None:
      self.array = None
      self._lib.rmb_host_mapped_free(self._host)
      self._host = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass
