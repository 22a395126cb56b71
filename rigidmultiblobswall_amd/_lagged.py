"""What the trajectory analyses over lags share (msd.MeanSquareDisplacement, scattering.IntermediateScattering,
vanhove.VanHove): the origin conventions and their counts, and LagAccumulator, the streaming base -- a trajectory goes to
the device in pieces, and between calls only the records of the origins whose lags are not complete yet stay there."""
import numpy as np

ORIGINS = ("window", "all")
UPLOAD_BYTES = 64 << 20       # frames go to the device in pieces of at most this many bytes (and at least n_lags frames)


def counts_per_lag(n_frames, n_bodies, n_lags, origins="window"):
  """Number of terms of every lag's sum, int64 (n_lags,): bodies x origins of the convention `origins`."""
  n_frames, n_bodies, n_lags = int(n_frames), int(n_bodies), int(n_lags)
  if n_lags < 1:
    raise ValueError("n_lags must be at least 1, got %r" % (n_lags,))
  if origins not in ORIGINS:
    raise ValueError("origins must be one of %s, got %r" % (ORIGINS, origins))
  if n_frames < 0 or n_bodies < 0:
    raise ValueError("n_frames and n_bodies must not be negative")
  if origins == "window":
    return np.full(n_lags, n_bodies * max(n_frames - n_lags + 1, 0), dtype=np.int64)
  return n_bodies * np.maximum(n_frames - np.arange(n_lags, dtype=np.int64), 0)


def lengths(periodic_length):
  L = np.asarray(periodic_length, dtype=np.float64).reshape(-1)
  if L.size != 3:
    raise ValueError("periodic_length must hold three lengths, got %r" % (periodic_length,))
  return L.copy()


class ContextHolder(object):
  """What the streaming analyses share whether or not they have lags: the single-GPU context they run on.  A subclass sets
  `entry` (the context method it cannot do without) and `what` (the words of the refusal)."""
  entry = None
  what = None       # "<the analysis> run(s)": ... on a single-GPU MobilityContext
  ctx, _own_ctx = None, False

  def _open(self, device, ctx):
    """ctx: a single-GPU MobilityContext (its resident configuration is left alone); None makes one on `device`, closed by
    close()."""
    self._own_ctx = ctx is None
    if ctx is None:
      from .context import MobilityContext
      ctx = MobilityContext(int(device))
    if not hasattr(ctx, self.entry):
      if self._own_ctx:
        ctx.close()
      raise ValueError("%s on a single-GPU MobilityContext, got %r" % (self.what, type(ctx).__name__))
    self.ctx = ctx
    import torch
    self._torch = torch
    self._dev = torch.device("cuda", ctx.device)

  def close(self):
    if self._own_ctx and self.ctx is not None:
      self.ctx.close()
    self.ctx = None


class LagAccumulator(ContextHolder):
  """Streaming base of an analysis over n_lags lags (lag l = l frames = l dt) of frames (k, n, width).  add_frames(frames)
  takes a numpy array or a CUDA float64 tensor in any number of pieces; per frame the tensors of _records() are kept
  while the frame is an origin whose lags are not complete (at most n_lags - 1 frames: self._tail, a tuple of tensors, or
  None), and _call(records, "window") is handed every buffer that completes at least one origin.  finish() ends the
  trajectory: with origins="all" the frames still held are origins of the lags that exist for them.

  A subclass sets `width`, `entry` (the context method it cannot do without), `what` and `row` (the words of its refusals),
  validates its own arguments after LagAccumulator.__init__ and before _open() (which may create a context), and supplies
  _per(), _records(piece) and _call(records, origins)."""
  width = None      # numbers per row of a frame
  row = None        # (name of n, "%d <rows> x <width> <numbers>")

  def __init__(self, n, n_lags, dt, origins):
    self.n, self.n_lags, self.dt = int(n), int(n_lags), float(dt)
    if self.n < 0:
      raise ValueError("%s must not be negative" % self.row[0])
    counts_per_lag(0, 1, self.n_lags, origins)      # refuses what the kernel entries would
    self.origins = origins
    self.n_frames = 0
    self.ctx, self._own_ctx = None, False
    self._finished = False
    self._tail = None

  def _per(self):
    """frames per upload piece"""
    return max(self.n_lags, UPLOAD_BYTES // (8 * max(self.width * self.n, 1)))

  def _records(self, piece):
    """the tensors kept per frame of `piece`, a contiguous CUDA float64 tensor (k, n, width): a tuple, frames along axis 0"""
    return (piece,)

  def _call(self, records, origins):
    raise NotImplementedError

  def _add_device(self, piece):
    rec = self._records(piece)
    if self._tail is not None:
      rec = tuple(self._torch.cat([t, r]) for t, r in zip(self._tail, rec))
    complete = rec[0].shape[0] - self.n_lags + 1      # origins of the buffer that have every lag
    if complete > 0:
      self._call(rec, "window")
      rec = tuple(r[complete:].clone() for r in rec)
    self._tail = rec if rec[0].shape[0] else None
    self.n_frames += int(piece.shape[0])

  def add_frames(self, frames):
    if self._finished:
      raise ValueError("add_frames() after finish()")
    torch = self._torch
    on_device = isinstance(frames, torch.Tensor)
    if on_device and not (frames.is_cuda and frames.dtype == torch.float64):
      raise ValueError("frames must be a numpy array or a CUDA float64 tensor")
    f = frames if on_device else np.ascontiguousarray(frames, dtype=np.float64)
    size, row = (f.numel() if on_device else f.size), self.width * self.n
    if row == 0 or size % row:
      raise ValueError("frames must hold whole frames of %s, got shape %r" % (self.row[1] % self.n, tuple(f.shape)))
    f = f.reshape(-1, self.n, self.width)
    per = self._per()
    for k in range(0, f.shape[0], per):
      piece = f[k:k + per]
      if not on_device:      # torch refuses a read-only array
        piece = torch.from_numpy(piece if piece.flags.writeable else piece.copy()).to(self._dev)
      self._add_device(piece.contiguous())
    return self

  def finish(self):
    """End of the trajectory.  origins="all": the frames still held are origins of the lags that exist for them."""
    if not self._finished:
      if self.origins == "all" and self._tail is not None:
        self._call(self._tail, "all")
      self._tail = None
      self._finished = True
    return self

  def times(self):
    return self.dt * np.arange(self.n_lags)
