"""numpy restatement of the 6 x 6 mean-square displacement sums, in the reference's rotation-matrix form
(general_application_utils.py: calc_total_msd_from_matrix_and_center), plus the trajectories and the error bound the MSD tests
share.  With dtype=np.longdouble it is the extended-precision oracle and also returns the absolute sums of the bound."""
import numpy as np

U = 2.0 ** -53
# Rounding counts of the bound  |S - S_ld|_ij <= u [ (n + C0) A_ij + C1 (X_i B_j + X_j B_i) ]  (test_gpu_msd.py derives them)
C0 = 4
C1 = 54


def rotation_matrices(q, dtype=np.float64):
  """The reference's Quaternion.rotation_matrix for q (..., 4), scalar part first, not normalised: (..., 3, 3)."""
  q = np.asarray(q, dtype=dtype)
  s, p0, p1, p2 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
  half = dtype(1) / dtype(2)
  diag = s * s - half
  R = np.empty(q.shape[:-1] + (3, 3), dtype=dtype)
  R[..., 0, 0] = p0 * p0 + diag; R[..., 0, 1] = p0 * p1 - s * p2; R[..., 0, 2] = p0 * p2 + s * p1
  R[..., 1, 0] = p1 * p0 + s * p2; R[..., 1, 1] = p1 * p1 + diag; R[..., 1, 2] = p1 * p2 - s * p0
  R[..., 2, 0] = p2 * p0 - s * p1; R[..., 2, 1] = p2 * p1 + s * p0; R[..., 2, 2] = p2 * p2 + diag
  return dtype(2) * R


def tracked(frames, offsets=None, dtype=np.float64):
  """(c, R): tracked points (F, N, 3) = x + R(q) p and rotation matrices (F, N, 3, 3) of frames (F, N, 7)."""
  f = np.asarray(frames, dtype=dtype)
  R = rotation_matrices(f[..., 3:7], dtype)
  c = f[..., :3].copy()
  if offsets is not None:
    p = np.broadcast_to(np.asarray(offsets, dtype=dtype).reshape(-1, 3), (f.shape[1], 3))
    c = c + np.einsum("fbij,bj->fbi", R, p)
  return c, R


def displacements(c, R, lag, n_origins):
  """Delta (n_origins, N, 6) of origins 0 .. n_origins - 1 at `lag`: [c(o + l) - c(o); 1/2 sum_i (R(o) e_i) x (R(o + l) e_i)]."""
  dx = c[lag:lag + n_origins] - c[:n_origins]
  R0, R1 = R[:n_origins], R[lag:lag + n_origins]
  u = np.zeros_like(dx)
  for i in range(3):
    u = u + np.cross(R0[..., :, i], R1[..., :, i]) / c.dtype.type(2)
  return np.concatenate([dx, u], axis=-1)


def n_origins_of(n_frames, n_lags, lag, origins):
  return max(n_frames - n_lags + 1, 0) if origins == "window" else max(n_frames - lag, 0)


def sums(frames, n_lags, offsets=None, origins="window", dtype=np.float64, absolute=False):
  """S (n_lags, 6, 6) and counts (n_lags,); absolute=True adds A_ij[l] = sum |Delta_i Delta_j| and B_i[l] = sum |Delta_i|."""
  f = np.asarray(frames)
  F, N = f.shape[0], f.shape[1]
  c, R = tracked(f, offsets, dtype)
  S = np.zeros((n_lags, 6, 6), dtype=dtype)
  A = np.zeros((n_lags, 6, 6), dtype=dtype)
  B = np.zeros((n_lags, 6), dtype=dtype)
  n = np.zeros(n_lags, dtype=np.int64)
  for lag in range(n_lags):
    k = n_origins_of(F, n_lags, lag, origins)
    n[lag] = k * N
    if k == 0 or N == 0:
      continue
    D = displacements(c, R, lag, k).reshape(-1, 6)
    S[lag] = np.einsum("ti,tj->ij", D, D)
    if absolute:
      A[lag] = np.einsum("ti,tj->ij", np.abs(D), np.abs(D))
      B[lag] = np.abs(D).sum(axis=0)
  return (S, n, A, B) if absolute else (S, n)


def bound(frames, offsets, n, A, B):
  """u [ (n[l] + C0) A_ij[l] + C1 (X_i B_j[l] + X_j B_i[l]) ], X = max(|x| + |p|) for the translational components, 1 for
  the rotational ones."""
  f = np.asarray(frames, dtype=np.float64)
  pmax = 0.0 if offsets is None else np.abs(np.asarray(offsets, dtype=np.float64)).max()
  xmax = (np.abs(f[..., :3]).max() if f.size else 0.0) + pmax
  X = np.array([xmax] * 3 + [1.0] * 3)
  A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
  n = np.asarray(n, dtype=np.float64)
  return U * ((n[:, None, None] + C0) * A + C1 * (X[None, :, None] * B[:, None, :] + X[None, None, :] * B[:, :, None]))


def quat_mul(a, b):
  """Hamilton product of quaternions (..., 4), scalar part first."""
  s = a[..., 0] * b[..., 0] - np.sum(a[..., 1:] * b[..., 1:], axis=-1)
  v = a[..., :1] * b[..., 1:] + b[..., :1] * a[..., 1:] + np.cross(a[..., 1:], b[..., 1:])
  return np.concatenate([s[..., None], v], axis=-1)


def axis_angle_quat(axis, angle):
  axis = np.asarray(axis, dtype=np.float64)
  angle = np.asarray(angle, dtype=np.float64)
  return np.concatenate([np.cos(angle / 2)[..., None], np.sin(angle / 2)[..., None] * axis], axis=-1)


def random_walk(n_frames, n_bodies, seed, centre=10.0, step=0.05, rot_step=0.05):
  """Seeded Brownian-like trajectory (F, N, 7): bodies near `centre`, translational steps of about `step`, rotations by
  about `rot_step` rad about random axes, unit quaternions (renormalised at every step, as the integrators do)."""
  rng = np.random.RandomState(seed)
  x = centre + rng.uniform(-1, 1, (n_bodies, 3))
  q = rng.randn(n_bodies, 4)
  q /= np.linalg.norm(q, axis=1, keepdims=True)
  out = np.empty((n_frames, n_bodies, 7))
  for f in range(n_frames):
    out[f, :, :3], out[f, :, 3:] = x, q
    x = x + step * rng.randn(n_bodies, 3)
    w = rot_step * rng.randn(n_bodies, 3)
    ang = np.linalg.norm(w, axis=1)
    dq = axis_angle_quat(w / ang[:, None], ang)
    q = quat_mul(dq, q)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
  return out


def screw_motion(n_frames, n_bodies, seed, tau=2.0 ** -6):
  """Constant velocity v_b and constant angular velocity w_b about a fixed lab-frame axis n_b: frames (F, N, 7) and the exact
  displacement Delta(l) = [v_b l tau; sin(w_b l tau) n_b] as a function lag -> (N, 6).  Start points, velocities and tau are
  dyadic, so every location is exact in double; the quaternions carry their own rounding (a few u, absolute)."""
  rng = np.random.RandomState(seed)
  x0 = 10.0 + np.round(1024 * rng.uniform(-1, 1, (n_bodies, 3))) / 1024
  v = np.round(16 * rng.uniform(-5, 5, (n_bodies, 3))) / 16
  axis = rng.randn(n_bodies, 3)
  axis /= np.linalg.norm(axis, axis=1, keepdims=True)
  w = rng.uniform(4.0, 12.0, n_bodies)
  q0 = rng.randn(n_bodies, 4)
  q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
  t = tau * np.arange(n_frames)
  frames = np.empty((n_frames, n_bodies, 7))
  frames[:, :, :3] = x0[None] + t[:, None, None] * v[None]
  q = quat_mul(axis_angle_quat(axis[None], t[:, None] * w[None]), q0[None])
  frames[:, :, 3:] = q / np.linalg.norm(q, axis=-1, keepdims=True)

  def exact(lag):
    return np.concatenate([v * (lag * tau), np.sin(w * (lag * tau))[:, None] * axis], axis=1)
  return frames, exact


def config_text(frames):
  """`.config` text of frames (F, N, 7): a count line, then the seven numbers of every body, repr-exact."""
  lines = []
  for frame in frames:
    lines.append("%d" % len(frame))
    lines.extend(" ".join(repr(float(v)) for v in row) for row in frame)
  return "\n".join(lines) + "\n"


def parse_msd(text):
  """(t, n, upper triangles (L, 21)) of the module's output format."""
  rows = np.array([[float(v) for v in line.split()] for line in text.splitlines() if line.strip()])
  return rows[:, 0], rows[:, 1].astype(np.int64), rows[:, 2:]
