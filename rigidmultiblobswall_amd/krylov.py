"""The iteration machinery of the Krylov solvers, apart from what they are applied to.

  * `drive`: the one lockstep driver.  Every iteration here (GMRES: _gmres_steps; Lanczos: stochastic._lanczos_steps; the
    adapters RigidSuspension.solve_task / forcing_task) is a coroutine that YIELDS each vector it needs a product with and
    receives the product back.  drive advances any number of them and hands the pending requests of a round to ONE
    `serve` call -- a single solve, two solves on a two-vector pair sweep, a whole stochastic step on k-vector sweeps.
  * right-preconditioned restarted GMRES (general_application_utils.py:514-627): `gmres_right_preconditioned`,
    `gmres_pair_right_preconditioned`; the host bookkeeping runs one iteration behind the device.
  * the two static workspaces an owner can hand to GMRES, which then run the device side of an iteration themselves
    (`step(j)`): _ArnoldiNative (one library call) and _ArnoldiGraphs (one captured hipGraph per iteration index).
  * `switched_off`: the one reader of the RMB_* environment overrides that turn a solver path off.

PyTorch is used for device memory and small dense algebra only.
"""
import contextlib
import gc
import math
import os

import numpy as np
import torch


def switched_off(name):
  """Whether the environment override `name` (RMB_NATIVE_GMRES, RMB_GMRES_GRAPH, ...) is set to "0".  How that combines
  with the attribute of the same purpose is the caller's business (INTEGRATION.md lists the switches)."""
  return os.environ.get(name, "") == "0"


def drive(tasks, serve):
  """Advance the coroutines `tasks` in lockstep until all have ended.  Each round collects the pending request of every
  running task, in task order, calls serve(requests) ONCE and sends the answers back (answers in request order).  Each
  task sees exactly what it would see alone.  Returns the tasks' return values, in task order; a task that ends at its
  first `next` (a zero right-hand side) has its value recorded like any other."""
  results = [None] * len(tasks)
  live, requests = [], []
  for k, task in enumerate(tasks):
    try:
      requests.append(next(task))
      live.append(k)
    except StopIteration as done:
      results[k] = done.value
  while live:
    answers = serve(requests)
    still, requests = [], []
    for k, answer in zip(live, answers):
      try:
        requests.append(tasks[k].send(answer))
        still.append(k)
      except StopIteration as done:
        results[k] = done.value
    live = still
  return results


def pair_server(one, two):
  """serve() of two tasks on the same operator: two(u, v) -> (A u, A v) while both run (one pass over the blob pairs with
  two vectors), one(u) -> A u once one of them has ended."""
  def serve(requests):
    return two(requests[0], requests[1]) if len(requests) == 2 else (one(requests[0]),)
  return serve


class _ArnoldiNative(object):
  """Static workspace of GMRES(restart) whose device side of an iteration is ONE call into the library
  (rmb_rigid_arnoldi_step_device: preconditioner blocks, pair sweep, finishing launch with the K products, fused
  Gram-Schmidt -- 7 launches from one host call, no graph, no copy command).  Same surface as _ArnoldiGraphs towards
  _gmres_steps: n, m, V, cols, host_cols (here page-locked memory mapped into the device's address space: the
  Gram-Schmidt kernel stores the column there itself) and step(j)."""

  def __init__(self, n, restart, device):
    from .context import MappedHostArray
    self.n, self.m, self.device = int(n), int(restart), device
    self.V = torch.zeros((self.m + 1, self.n), dtype=torch.float64, device=device)
    self.cols = torch.zeros((self.m, self.m + 2), dtype=torch.float64, device=device)
    self.z = torch.empty(self.n, dtype=torch.float64, device=device)
    self.w = torch.empty(self.n, dtype=torch.float64, device=device)
    self.mapped = MappedHostArray((self.m, self.m + 2))
    self.host_cols = self.mapped.array
    self.steps = self.steps_this_solve = 0

  def bind(self, owner):
    """Once per solve: everything of the step call that does not change from one iteration to the next, as plain integers
    (building sixteen ctypes objects per iteration costs more host time than the GPU needs for the iteration), and the
    owner's product counter."""
    self.steps_this_solve = 0
    ctx, g = owner.ctx, owner.groups[0]
    for t in (g.A11, g.A12, g.A21, g.A22, g.K):
      assert t.is_contiguous()
    ctx._follow_torch_stream()                   # the solve stays on the stream that is current now
    self._count = owner._count_operator
    self._fn = ctx._lib.rmb_rigid_arnoldi_step_device
    self._head = (ctx._h, g.K.shape[0], g.K.shape[1] // 3, g.A11.data_ptr(), g.A12.data_ptr(), g.A21.data_ptr(), g.A22.data_ptr(),
                  g.K.data_ptr(), self.V.data_ptr(), self.V.stride(0))
    self._tail = (float(owner.eta), self.z.data_ptr(), self.w.data_ptr())
    self._cols_ptr, self._mapped_ptr, self._row = self.cols.data_ptr(), self.mapped.dev_ptr, 8 * (self.m + 2)

  def step(self, j):
    rc = self._fn(*self._head, j, *self._tail, self._cols_ptr + j * self._row, self._mapped_ptr + j * self._row)
    if rc != 0:
      from . import _lib
      _lib.check(rc)
    self._count()
    self.steps += 1
    self.steps_this_solve += 1

  def close(self):
    self._count = None
    if self.mapped is not None:
      self.host_cols = None
      self.mapped.close()
      self.mapped = None


class _ArnoldiGraphs(object):
  """Static workspace of GMRES(restart) on one system size and, per iteration index j, a captured hipGraph of everything
  the DEVICE does in that iteration (preconditioner, operator, Gram-Schmidt, normalisation, column to page-locked
  memory).  On systems of a few thousand blobs an iteration is ~16 small launches whose enqueueing costs more host time
  than they take to run (tools/experiments/exp_small_deck_gmres.py: ~200 us per iteration around a 10-20 us blob
  product); replaying a graph is one call.

  An index j runs eagerly the first time it is met, is captured once `capture_after` solves have been seen, and is
  replayed from then on.  The graphs hold pointers: to this workspace, to the operator's K and preconditioner blocks
  (rewritten in place by set_configuration / build_preconditioner), to the context's packed positions and accumulators.
  bind() drops them whenever the signature the owner hands over changes."""
  capture_after = 2

  def __init__(self, n, restart, device):
    self.n, self.m, self.device = int(n), int(restart), device
    self.V = torch.zeros((self.m + 1, self.n), dtype=torch.float64, device=device)
    self.cols = torch.zeros((self.m, self.m + 2), dtype=torch.float64, device=device)
    self.host_cols = torch.zeros((self.m, self.m + 2), dtype=torch.float64).pin_memory()
    # The fused Gram-Schmidt kernel can store the new Hessenberg column straight into page-locked memory that is mapped
    # into the device's address space (context.MappedHostArray): one graph node (the copy) less per iteration.  Set up by
    # the owner when its context has the entry point; host_cols then IS that memory (a numpy array).
    self.mapped_cols = None
    self.stream = torch.cuda.Stream(device)
    self.graphs, self.seen, self.signature = {}, set(), None
    self.solves = self.captures = self.replays = self.replays_this_solve = 0
    self.buffers = None               # callable: the context's buffers_signature() (set by the owner), checked before a replay
    self.buffers_at_capture = None
    self.stale_drops = 0
    self.A = self.Minv = self.ortho = self.on_replay = None

  def bind(self, signature, A, Minv, ortho, on_replay):
    """Once per solve, right before solve_stream(), which lets go of it again: the signature of everything the graphs
    point at, and what the device side of an iteration is built from -- operator, preconditioner, the fused Gram-Schmidt
    (or None: torch operations) and the owner's product counter, called on a replay (an eager or capturing iteration
    counts inside A)."""
    if signature != self.signature:
      self.release()
      self.signature = signature
    self.A, self.Minv, self.ortho, self.on_replay = A, Minv, ortho, on_replay

  def use_mapped_columns(self):
    if self.mapped_cols is None:
      from .context import MappedHostArray
      self.mapped_cols = MappedHostArray((self.m, self.m + 2))
      self.host_cols = self.mapped_cols.array

  def release(self):
    """Destroy the graphs now (a safe point: nothing is capturing) rather than whenever the collector finds them.  A graph
    of the previous solve may still be executing -- the lagged bookkeeping leaves its last, discarded iteration in flight,
    and a stale-buffer drop happens in the middle of a solve: wait for the device first, destroying an executing
    hipGraphExec is not something to rely on (an intermittent hang of a slip-scheme test on the box was traced to here)."""
    if self.graphs and self.device.type == "cuda":
      torch.cuda.synchronize(self.device)
    self.graphs.clear()
    self.seen.clear()
    self.solves = 0

  @contextlib.contextmanager
  def solve_stream(self, ctx):
    """The whole solve runs on the workspace's stream (a capture cannot happen on the default stream, and the context must
    already enqueue on the capturing stream when a capture begins).  Yields the caller's stream, which waits for the
    solve afterwards; a result computed inside wants record_stream(that stream).  What bind() was handed goes when the
    solve ends, so that between solves the workspace holds no reference to its owner (an owner dropped without close() is
    freed by its reference count, graphs included, not whenever the cyclic collector runs)."""
    cur = torch.cuda.current_stream(self.device)
    self.stream.wait_stream(cur)
    try:
      with torch.cuda.stream(self.stream):
        ctx._follow_torch_stream()
        self.solves += 1
        self.replays_this_solve = 0
        yield cur
    finally:
      self.A = self.Minv = self.ortho = self.on_replay = None
    cur.wait_stream(self.stream)

  def _device_side(self, j):
    """Everything the device does in iteration j, on this workspace's buffers."""
    V, cols = self.V, self.cols
    w = self.A(self.Minv(V[j]))
    if self.ortho is not None and self.mapped_cols is not None:
      # the kernel stores the column into host memory itself: row j of the mapped buffer
      self.ortho(V, j + 1, w, cols[j], V[j + 1], self.mapped_cols.dev_ptr + 8 * j * (self.m + 2))
      return
    if self.ortho is not None:
      self.ortho(V, j + 1, w, cols[j], V[j + 1])
    else:
      torch.div(_gram_schmidt(V, cols, j, w), cols[j, j + 1], out=V[j + 1])
    self.host_cols[j, :j + 2].copy_(cols[j, :j + 2], non_blocking=True)

  def step(self, j):
    g = self.graphs.get(j)
    if g is not None and self.buffers is not None and self.buffers() != self.buffers_at_capture:
      # The graph holds the addresses of the context's internal buffers by value, and one of them has moved since the
      # capture (another, larger suspension used the shared context; a product grew a scratch buffer): every graph is
      # stale.  Same treatment as a changed signature in bind(): drop them, run eagerly again, capture afresh after
      # `capture_after` further solves.
      self.release()
      self.solves = 1            # this solve is the first of the new series
      self.stale_drops += 1
      g = None
    if g is None:
      if j not in self.seen or self.solves <= self.capture_after:
        self._device_side(j)                     # eager: also warms every library call of this iteration's shapes
        self.seen.add(j)
        return
      g = torch.cuda.CUDAGraph()
      torch.cuda.synchronize(self.device)
      # No cyclic garbage collection while the stream is capturing: collecting a dead CUDAGraph (another suspension's,
      # say) calls hipGraphDestroy, which HIP refuses during a capture -- and the refusal surfaces in a destructor.
      gc_was_on = gc.isenabled()
      gc.disable()
      try:
        g.capture_begin(capture_error_mode="thread_local")
        try:
          self._device_side(j)                   # enqueues nothing: recorded into the graph (the owner counts it)
        finally:
          g.capture_end()
      finally:
        if gc_was_on:
          gc.enable()
      if self.buffers is not None:
        now = self.buffers()
        if self.graphs and now != self.buffers_at_capture:    # the eager warm-ups have sized everything: never expected
          self.graphs.clear()
          self.stale_drops += 1
        self.buffers_at_capture = now
      self.graphs[j] = g
      self.captures += 1
    elif self.on_replay is not None:
      self.on_replay()
    g.replay()
    self.replays += 1
    self.replays_this_solve += 1


# page-locked staging rows for the Hessenberg columns of running solves (allocated once, handed out per solve)
_pinned_pool = []


def _pinned_columns(rows, cols):
  for k, t in enumerate(_pinned_pool):
    if t.shape[0] >= rows and t.shape[1] >= cols:
      return _pinned_pool.pop(k)
  return torch.empty((max(rows, 62), max(cols, 63)), dtype=torch.float64).pin_memory()


def _gram_schmidt(V, cols, j, w):
  """Two passes of classical Gram-Schmidt of w against V[0..j]; the new Hessenberg column and |w| go to cols[j]."""
  Vj = V[:j + 1]
  h = Vj @ w
  w = torch.addmv(w, Vj.t(), h, alpha=-1.0)
  h2 = Vj @ w
  w = torch.addmv(w, Vj.t(), h2, alpha=-1.0)
  torch.add(h, h2, out=cols[j, :j + 1])
  torch.linalg.vector_norm(w, out=cols[j, j + 1])
  return w


def _gmres_steps(Minv, b, tol, restart, maxiter, x0, sync, lag=None, ws=None, ortho=None):
  """GMRES(restart) on A.Minv written as a coroutine: it YIELDS every vector it needs the operator applied to and
  receives A(vector) back, so `drive` can serve a single solve (gmres_right_preconditioned) or advance two solves
  in lockstep and hand both requests to a two-vector operator (gmres_pair_right_preconditioned).  Returns (x, info).

  On a GPU the host side of an iteration (Givens rotations on the new Hessenberg column, the convergence test) runs ONE
  ITERATION LATE (`lag`, default on for CUDA tensors): the column is normalised on the device, copied to page-locked
  memory asynchronously, and read only after the NEXT iteration's preconditioner + operator + Gram-Schmidt have been
  enqueued -- the device never waits for the host between sweeps.  The iterates, the stopping rule and the iteration
  count are those of the plain loop; what the lag can cost is one discarded sweep when the solve converges earlier than
  its own history predicts, so the loop turns synchronous as soon as the last observed reduction rate says the next
  column may meet the tolerance (normally the last two or three iterations).

  ws: a static workspace (_ArnoldiNative, _ArnoldiGraphs) that runs the device side of iteration j itself, operator
  included: ws.step(j) leaves V[j + 1] and cols[j] on the device and the column in ws.host_cols.  Only the initial and
  the restart residuals are then requested from the driver."""
  dev = b.device
  n = b.numel()
  if lag is None:
    lag = dev.type == "cuda"
  if ws is not None:
    assert sync is None and dev.type == "cuda" and ws.n == n and ws.m == restart
    lag = True
  if not lag or sync is not None:      # the fused Gram-Schmidt normalises on the device right away
    ortho = None

  def host_norm(v):
    t = torch.linalg.vector_norm(v).reshape(1)
    if sync is not None:
      sync(t)
    return float(t)

  bnorm = host_norm(b)
  y = torch.zeros(n, dtype=torch.float64, device=dev)
  if x0 is not None:
    b = b - (yield x0)
    beta = host_norm(b)
  else:
    beta = bnorm
  r = b.clone()
  its = 0
  res = beta / bnorm if bnorm > 0 else 0.0
  history = []
  wasted = 0
  pooled = _pinned_columns(restart + 1, restart + 2) if lag and ws is None else None
  host_cols = ws.host_cols if ws is not None else pooled
  events = [torch.cuda.Event(), torch.cuda.Event()] if lag else None
  # the stream the iterations are enqueued on: looked up once (a solve does not change streams; the lookup is 4 us of the
  # ~45 us of host time an iteration of a small deck costs)
  ev_stream = torch.cuda.current_stream(dev) if lag else None
  try:
    while its < maxiter and res > tol:
      m = min(restart, maxiter - its)
      if ws is not None:
        V, cols = ws.V, ws.cols
      else:
        V = torch.empty((m + 1, n), dtype=torch.float64, device=dev)
        cols = torch.empty((m, m + 2), dtype=torch.float64, device=dev)    # row j = column j of H, then |w_j|
      V[0] = r / beta
      H = np.zeros((m + 1, m))
      cs, sn = [0.0] * m, [0.0] * m          # plain Python floats: the rotations below are a scalar recurrence, and numpy
      g = [0.0] * (m + 1)                    # scalars cost ~10x a float operation (it is host time between two sweeps)
      g[0] = beta
      k_used = 0
      prev_res = None

      def finish(j):
        """Host side of iteration j: read its column, rotate, test.  True = stop after this column."""
        nonlocal its, k_used, res, prev_res
        if lag:
          events[j & 1].synchronize()
          col = host_cols[j, :j + 2].tolist()
        else:
          col = cols[j, :j + 2].tolist()                              # the one host transfer of the iteration
        w_norm = col[-1]
        last_norm[0] = w_norm
        for i in range(j):                                           # previous rotations
          t = cs[i] * col[i] + sn[i] * col[i + 1]
          col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
          col[i] = t
        d = math.hypot(col[j], col[j + 1])
        cs[j], sn[j] = (col[j] / d, col[j + 1] / d) if d > 0 else (1.0, 0.0)
        col[j] = d
        col[j + 1] = 0.0
        H[:j + 2, j] = col
        g[j + 1] = -sn[j] * g[j]
        g[j] = cs[j] * g[j]
        its += 1
        k_used = j + 1
        prev_res, res = res, abs(g[j + 1]) / bnorm
        history.append(res)
        return res <= tol or w_norm == 0 or not math.isfinite(w_norm)

      def may_defer():
        """Whether the pending column can wait until the next iteration has been enqueued: not when the last
        observed reduction rate says it may already meet the tolerance."""
        rate = min(1.0, res / prev_res) if prev_res else 1.0
        return res * rate > 20.0 * tol

      pending, stop, last_norm = None, False, [0.0]
      for j in range(m):
        if pending is not None and not may_defer():
          stop, pending = finish(pending), None
          if stop:
            break
        if ws is not None:
          ws.step(j)
        else:
          w = yield Minv(V[j])
          if ortho is not None:                                      # both passes, column, |w| and V[j + 1] in four launches
            ortho(V, j + 1, w if w.is_contiguous() else w.contiguous(), cols[j], V[j + 1])
          else:
            w = _gram_schmidt(V, cols, j, w)
          if sync is not None:                                       # multi-rank: all ranks act on rank 0's numbers
            sync(cols[j, :j + 2])
          if lag:
            if ortho is None:
              torch.div(w, cols[j, j + 1], out=V[j + 1])             # normalised on the device: no host value needed
            host_cols[j, :j + 2].copy_(cols[j, :j + 2], non_blocking=True)
        if lag:
          # fence on the stream the copy was enqueued on: the current stream of the VECTORS' device, which need not
          # be the process's current device (a suspension built on cuda:1 while cuda:0 is current)
          events[j & 1].record(ev_stream)
          if pending is not None:
            stop, pending = finish(pending), None
            if stop:
              wasted += 1                                            # iteration j was enqueued for nothing
              break
          pending = j
        else:
          stop = finish(j)
          if last_norm[0] > 0:
            torch.mul(w, 1.0 / last_norm[0], out=V[j + 1])
          if stop:
            break
      if pending is not None and not stop:
        finish(pending)
      coef = np.linalg.solve(np.triu(H[:k_used, :k_used]), np.array(g[:k_used])) if k_used > 0 else np.zeros(0)
      y = y + V[:k_used].t() @ torch.as_tensor(coef, device=dev)
      if res > tol and its < maxiter:                                # restart: true residual
        r = b - (yield Minv(y))
        beta = host_norm(r)
        res = beta / bnorm
  finally:
    if pooled is not None:
      _pinned_pool.append(pooled)
  x = Minv(y)
  if x0 is not None:
    x = x + x0
  return x, dict(iterations=its, residual=res, converged=bool(res <= tol), history=history, discarded_sweeps=wasted)


def gmres_right_preconditioned(A, Minv, b, tol=1e-8, restart=60, maxiter=1000, x0=None, sync=None, lag=None, ws=None,
                               ortho=None):
  """Solve A x = b with x = x0 + Minv y, GMRES(restart) on A.Minv (general_application_utils.py:608-627).
  Stops when |b - A x| <= tol |b| (scipy `tol`, atol = 0) or after `maxiter` INNER iterations in total -- not restart
  cycles: scipy (and the reference's call, maxiter=1000 with restart=60) counts cycles, i.e. up to 60 000 inner
  iterations; the solves here converge in tens of iterations, so the cap only differs in how soon a diverging solve
  gives up.
  Arnoldi with two passes of classical Gram-Schmidt (one device GEMV each); Givens rotations on the host, on a GPU one
  iteration behind the device (`lag`, see _gmres_steps; None = on for CUDA tensors).
  x0: optional initial guess (the roller torque solve warm-starts from the previous step,
  quaternion_integrator_rollers.py:961); the Krylov space is then built on the residual b - A x0.
  ws: a bound workspace that runs the iterations itself (see _gmres_steps); A then serves the residuals only."""
  steps = _gmres_steps(Minv, b, tol, restart, maxiter, x0, sync, lag, ws=ws, ortho=ortho)
  return drive([steps], lambda requests: (A(requests[0]),))[0]


def gmres_pair_right_preconditioned(A, A2, Minv, b_a, b_b, tol=1e-8, restart=60, maxiter=1000, sync=None, ortho=None):
  """Two independent solves A x_a = b_a, A x_b = b_b advanced in lockstep: while both are running, each iteration
  hands its two operator requests to A2(u, v) -> (A u, A v) -- one pass over the blob pairs with two vectors
  (rmb_matvec2_device) instead of two.  Every solve sees exactly the iterates it would see alone.
  Returns ((x_a, info_a), (x_b, info_b))."""
  tasks = [_gmres_steps(Minv, b, tol, restart, maxiter, None, sync, ortho=ortho) for b in (b_a, b_b)]
  return tuple(drive(tasks, pair_server(A, A2)))
