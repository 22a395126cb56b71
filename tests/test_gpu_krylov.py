"""The O(N) helpers of the rigid-body solve (csrc/rmb_krylov.hip) against plain numpy / torch fp64: the batched
two-by-two block product (preconditioner, K and K^T products) and the fused two-pass Gram-Schmidt of an Arnoldi step."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nb,r1,c1,r2,c2", [(1, 1, 1, 1, 1), (5, 36, 36, 6, 6), (300, 36, 36, 6, 6), (7, 150, 150, 6, 6), (3, 700, 640, 9, 5),
                                            (4, 5, 0, 3, 2), (2048, 36, 36, 6, 6), (32, 126, 126, 6, 6), (5, 96, 96, 6, 6), (5, 97, 97, 6, 6), (3, 129, 257, 5, 130)])
def test_block_apply_matches_batched_products(nb, r1, c1, r2, c2):
  import torch
  from rigidmultiblobswall_amd import MobilityContext
  g = torch.Generator(device="cpu").manual_seed(nb + r1)
  rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).cuda()
  ctx = MobilityContext(0)
  try:
    A11, A12, A21, A22 = rnd(nb, r1, c1), rnd(nb, r1, c2), rnd(nb, r2, c1), rnd(nb, r2, c2)
    x1, x2 = rnd(nb, c1), rnd(nb, c2)
    y1, y2 = rnd(nb, r1), rnd(nb, r2)
    y1_0, y2_0 = y1.clone(), y2.clone()
    mv = lambda A, x: torch.bmm(A, x.unsqueeze(-1)).squeeze(-1)
    # overwrite (beta = 0: the old contents, here with a NaN planted, must not be read)
    y1[0, 0] = float("nan")
    ctx.block_apply_device(A11, A12, A21, A22, x1, x2, y1, y2)
    assert rel_err(y1.cpu().numpy(), (mv(A11, x1) + mv(A12, x2)).cpu().numpy()) < 1e-13
    assert rel_err(y2.cpu().numpy(), (mv(A21, x1) + mv(A22, x2)).cpu().numpy()) < 1e-13
    # accumulate with alpha, beta; absent blocks; a transposed block (the operator's use: top -= K U, bottom = -K^T lambda)
    if c1 == r1:
      K = rnd(nb, r1, c2)
      KT_shape_ok = (r2 == c2)
      y1.copy_(y1_0); y2.copy_(y2_0)
      if KT_shape_ok:
        ctx.block_apply_device(None, K, K, None, x1, x2, y1, y2, alpha=-1.0, beta1=1.0, transpose=(False, False, True, False))
        assert rel_err(y1.cpu().numpy(), (y1_0 - mv(K, x2)).cpu().numpy()) < 1e-13
        assert rel_err(y2.cpu().numpy(), (-mv(K.transpose(1, 2), x1)).cpu().numpy()) < 1e-13
    y1.copy_(y1_0); y2.copy_(y2_0)
    ctx.block_apply_device(A11, None, None, A22, x1, x2, y1, y2, alpha=0.5, beta1=2.0, beta2=-1.0)
    assert rel_err(y1.cpu().numpy(), (2.0 * y1_0 + 0.5 * mv(A11, x1)).cpu().numpy()) < 1e-13
    assert rel_err(y2.cpu().numpy(), (-y2_0 + 0.5 * mv(A22, x2)).cpu().numpy()) < 1e-13
    # strided blocks: a slice of a larger tensor
    big = rnd(nb, r1 + 3, c1 + 2)
    sub = big[:, 1:1 + r1, 2:2 + c1]
    ctx.block_apply_device(sub, None, None, None, x1, x2, y1, y2)
    assert rel_err(y1.cpu().numpy(), mv(sub, x1).cpu().numpy()) < 1e-13 if c1 > 0 else float(y1.abs().max()) == 0.0
    assert float(y2.abs().max()) == 0.0
  finally:
    ctx.close()


@pytest.mark.parametrize("n,rows", [(1, 1), (5, 3), (1024, 1), (1025, 7), (4608, 9), (4608, 60), (86016, 19), (300001, 61), (70000, 256),
                                    (2688, 17), (6144, 61), (6144, 256), (6145, 61)])
def test_fused_gram_schmidt_matches_two_classical_passes(n, rows):
  import torch
  from rigidmultiblobswall_amd import MobilityContext
  g = torch.Generator(device="cpu").manual_seed(n + rows)
  m = rows + 2
  rows_eff = min(rows, n)           # an orthonormal set of more than n vectors does not exist
  Q, _ = torch.linalg.qr(torch.randn(n, rows_eff, generator=g, dtype=torch.float64))
  V = torch.zeros((m, n), dtype=torch.float64)
  V[:rows_eff] = Q.t()
  V = V.cuda()
  w0 = torch.randn(n, generator=g, dtype=torch.float64).cuda()
  ctx = MobilityContext(0)
  try:
    w, col = w0.clone(), torch.zeros(m + 1, dtype=torch.float64, device="cuda")
    ctx.krylov_orthogonalize_device(V, rows, w, col, V[rows])
    Vj = V[:rows].clone()
    h = Vj @ w0
    w1 = w0 - Vj.t() @ h
    h2 = Vj @ w1
    w2 = w1 - Vj.t() @ h2
    nrm = float(torch.linalg.vector_norm(w2))
    assert rel_err(col[:rows].cpu().numpy(), (h + h2).cpu().numpy()) < 1e-12
    if rows_eff < n:
      assert abs(float(col[rows]) - nrm) <= 1e-12 * max(nrm, 1.0)
      assert rel_err(w.cpu().numpy(), w2.cpu().numpy()) < 1e-9
      assert rel_err(V[rows].cpu().numpy(), (w2 / nrm).cpu().numpy()) < 1e-9
      # what the solver needs of it: orthogonal to the basis to rounding, unit length
      assert float((Vj @ V[rows]).abs().max()) < 1e-12 and abs(float(torch.linalg.vector_norm(V[rows])) - 1.0) < 1e-13
    # fixed-order reductions: bit-reproducible
    w_b, col_b = w0.clone(), torch.zeros_like(col)
    vb = torch.empty(n, dtype=torch.float64, device="cuda")
    ctx.krylov_orthogonalize_device(V, rows, w_b, col_b, vb)
    assert torch.equal(w_b, w) and torch.equal(col_b[:rows + 1], col[:rows + 1])
    # the column once more in page-locked, device-mapped host memory: readable after one stream wait, no copy command
    from rigidmultiblobswall_amd.context import MappedHostArray
    mapped = MappedHostArray((3, m + 1))
    try:
      w_c, col_c = w0.clone(), torch.zeros_like(col)
      ctx.krylov_orthogonalize_device(V, rows, w_c, col_c, vb, mapped.dev_ptr + 8 * (m + 1))      # row 1 of the buffer
      torch.cuda.synchronize()
      assert np.array_equal(mapped.array[1, :rows + 1], col[:rows + 1].cpu().numpy())
      assert not mapped.array[0].any() and not mapped.array[2].any() and torch.equal(w_c, w)
    finally:
      mapped.close()
  finally:
    ctx.close()


@pytest.mark.parametrize("nb,n_b,wall,L", [(40, 12, True, None), (7, 15, False, None), (3, 42, True, None), (64, 12, True, (60.0, 60.0, 0.0)),
                                           (5, 12, True, None), (300, 12, True, None)])
def test_rigid_operator_in_one_call_equals_product_and_block_products(nb, n_b, wall, L):
  """rmb_rigid_operator_device = [M_tt lambda - K U; -K^T lambda] (multi_bodies.py:424-471): the pair sweep + ONE finishing
  launch with the symmetric kernels, the three-launch fallback below 128 blobs and with periodic images -- against the
  product and numpy K products, twice in a row (the accumulators are back to zero), and against the oracle's M."""
  import torch
  from rigidmultiblobswall_amd import MobilityContext
  from oracle import oracle
  rng = np.random.RandomState(nb + n_b)
  N = nb * n_b
  a, eta = 0.3, 1.3
  r = rng.rand(N, 3) * (N / 0.05) ** (1.0 / 3.0) * a
  r[:, 2] += 0.5 * a
  K = rng.randn(nb, 3 * n_b, 6)
  x = rng.randn(3 * N + 6 * nb)
  dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")
  ctx = MobilityContext(0)
  try:
    ctx.set_positions(dev(r.reshape(-1)), a, None if L is None else np.array(L), wall)
    lam, U = x[:3 * N], x[3 * N:].reshape(nb, 6)
    Mlam = ctx.matvec_device("tt", dev(lam), eta).cpu().numpy()
    want = np.concatenate([Mlam - np.einsum("bij,bj->bi", K, U).reshape(-1),
                           -np.einsum("bij,bi->bj", K, lam.reshape(nb, 3 * n_b)).reshape(-1)])
    for rep in range(2):
      out = torch.full((3 * N + 6 * nb,), float("nan"), dtype=torch.float64, device="cuda")
      ctx.rigid_operator_device(dev(K), dev(x), eta, out)
      assert rel_err(out.cpu().numpy(), want) < 1e-13, (rep, rel_err(out.cpu().numpy(), want))
    assert rel_err(ctx.matvec_device("tt", dev(lam), eta).cpu().numpy(), Mlam) < 1e-13      # the plain product still finds clean accumulators
    kw = {} if L is None else dict(periodic_length=np.array(L))
    fn = oracle.single_wall_mobility_trans_times_force_oracle if wall else oracle.no_wall_mobility_trans_times_force_oracle
    assert rel_err(out.cpu().numpy()[:3 * N] + np.einsum("bij,bj->bi", K, U).reshape(-1), fn(r, lam.reshape(-1, 3), eta, a, **kw)) < 1e-11
  finally:
    ctx.close()


def test_helper_argument_checks():
  import torch
  from rigidmultiblobswall_amd import MobilityContext, _lib
  ctx = MobilityContext(0)
  try:
    V = torch.zeros((300, 16), dtype=torch.float64, device="cuda")
    w = torch.zeros(16, dtype=torch.float64, device="cuda")
    col = torch.zeros(301, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.RmbError):
      ctx.krylov_orthogonalize_device(V, 257, w, col, V[299])          # more rows than one call takes
    x1 = torch.zeros((2, 9000), dtype=torch.float64, device="cuda")
    x2 = torch.zeros((2, 1), dtype=torch.float64, device="cuda")
    y = torch.zeros((2, 1), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.RmbError):
      ctx.block_apply_device(None, None, None, None, x1, x2, y, y.clone())   # operand of one entry does not fit LDS
  finally:
    ctx.close()


@pytest.mark.parametrize("nb,n_b", [(1, 1), (3, 2), (5, 12), (300, 12), (7, 16), (2048, 12), (4, 7)])
def test_rigid_configuration_kernel_matches_the_body_formulas(nb, n_b):
  """Blob coordinates, body-frame offsets and K of body/body.py:64-115 in one launch, against the numpy formulas
  (rigid.blob_positions / quaternion_rotation_matrix, the rot matrix written out)."""
  import torch
  from rigidmultiblobswall_amd import MobilityContext
  from rigidmultiblobswall_amd.rigid import blob_positions
  rng = np.random.RandomState(nb + n_b)
  ref = rng.randn(nb, n_b, 3)
  loc = rng.randn(nb, 3) * 3
  quat = rng.randn(nb, 4)
  quat /= np.linalg.norm(quat, axis=1, keepdims=True)
  dev = lambda x: torch.as_tensor(x, device="cuda")
  r = torch.empty((nb * n_b, 3), dtype=torch.float64, device="cuda")
  rel = torch.empty((nb, n_b, 3), dtype=torch.float64, device="cuda")
  K = torch.full((nb, 3 * n_b, 6), float("nan"), dtype=torch.float64, device="cuda")       # every entry must be written
  ctx = MobilityContext(0)
  try:
    ctx.rigid_configuration_device(dev(ref), dev(loc), dev(quat), r, rel, K)
    r_ref = np.concatenate([blob_positions(ref[b], loc[b], quat[b]) for b in range(nb)])
    assert np.abs(r.cpu().numpy() - r_ref).max() < 1e-13
    rel_ref = r_ref.reshape(nb, n_b, 3) - loc[:, None, :]
    assert np.abs(rel.cpu().numpy() - rel_ref).max() < 1e-13
    K_ref = np.zeros((nb, n_b, 3, 6))
    K_ref[:, :, 0, 0] = K_ref[:, :, 1, 1] = K_ref[:, :, 2, 2] = 1.0
    K_ref[:, :, 0, 4] = rel_ref[:, :, 2];  K_ref[:, :, 0, 5] = -rel_ref[:, :, 1]
    K_ref[:, :, 1, 3] = -rel_ref[:, :, 2]; K_ref[:, :, 1, 5] = rel_ref[:, :, 0]
    K_ref[:, :, 2, 3] = rel_ref[:, :, 1];  K_ref[:, :, 2, 4] = -rel_ref[:, :, 0]
    assert np.abs(K.cpu().numpy() - K_ref.reshape(nb, 3 * n_b, 6)).max() < 1e-13
    # outputs that are not wanted may be left out
    r2 = torch.empty_like(r)
    ctx.rigid_configuration_device(dev(ref), dev(loc), dev(quat), r2)
    assert torch.equal(r2, r)
  finally:
    ctx.close()


@pytest.mark.parametrize("nb,n_b", [(1, 3), (5, 12), (300, 12), (9, 16), (2048, 12), (6, 4),
                                    # round 5: 17 .. 42 blobs per body, ONE n x n matrix in LDS, everything in place
                                    (3, 17), (7, 30), (2, 42), (300, 42)])
def test_rigid_preconditioner_kernel_matches_dense_linear_algebra(nb, n_b):
  """Per-body Cholesky factor, its inverse, M^-1, N = (K^T M^-1 K)^-1 and the four blocks of [[M, -K], [-K^T, 0]]^-1
  (multi_bodies.py:516-560) against numpy on every body -- the blocks checked by what they must satisfy."""
  import torch
  from rigidmultiblobswall_amd import MobilityContext
  rng = np.random.RandomState(nb * 7 + n_b)
  n = 3 * n_b
  G = rng.randn(nb, n, n)
  Mb = G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n)          # SPD, condition number O(10)
  rel = rng.randn(nb, n_b, 3)
  K = np.zeros((nb, n_b, 3, 6))
  K[:, :, 0, 0] = K[:, :, 1, 1] = K[:, :, 2, 2] = 1.0
  K[:, :, 0, 4] = rel[:, :, 2];  K[:, :, 0, 5] = -rel[:, :, 1]
  K[:, :, 1, 3] = -rel[:, :, 2]; K[:, :, 1, 5] = rel[:, :, 0]
  K[:, :, 2, 3] = rel[:, :, 1];  K[:, :, 2, 4] = -rel[:, :, 0]
  K = K.reshape(nb, n, 6)
  dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")
  mk = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
  out = dict(Lchol=mk(nb, n, n), Linv=mk(nb, n, n), Minv=mk(nb, n, n), Nbody=mk(nb, 6, 6), A11=mk(nb, n, n), A12=mk(nb, n, 6),
             A21=mk(nb, 6, n), A22=mk(nb, 6, 6))
  info = torch.ones(1, dtype=torch.int32, device="cuda")
  ctx = MobilityContext(0)
  try:
    # a slightly unsymmetric input: the kernel symmetrises on load, like the torch path
    skew = 1e-13 * rng.randn(nb, n, n)
    ctx.rigid_preconditioner_device(dev(Mb + skew - skew.transpose(0, 2, 1)), dev(K), *out.values(), info)
    assert int(info) == 0
    o = {k: v.cpu().numpy() for k, v in out.items()}
    L = np.linalg.cholesky(Mb)
    assert np.abs(o["Lchol"] - L).max() < 1e-12 and np.abs(np.triu(o["Lchol"], 1)).max() == 0.0
    eye = np.eye(n)
    assert np.abs(o["Linv"] @ L - eye).max() < 1e-11
    assert np.abs(o["Minv"] @ Mb - eye).max() < 1e-10 and np.abs(o["Minv"] - o["Minv"].transpose(0, 2, 1)).max() == 0.0
    Rres = K.transpose(0, 2, 1) @ np.linalg.solve(Mb, K)
    assert np.abs(o["Nbody"] @ Rres - np.eye(6)).max() < 1e-9 and np.abs(o["Nbody"] - o["Nbody"].transpose(0, 2, 1)).max() == 0.0
    # the blocks ARE the inverse of the saddle-point matrix of one body
    S = np.zeros((nb, n + 6, n + 6))
    S[:, :n, :n] = Mb; S[:, :n, n:] = -K; S[:, n:, :n] = -K.transpose(0, 2, 1)
    P = np.zeros_like(S)
    P[:, :n, :n] = o["A11"]; P[:, :n, n:] = o["A12"]; P[:, n:, :n] = o["A21"]; P[:, n:, n:] = o["A22"]
    assert np.abs(P @ S - np.eye(n + 6)).max() < 1e-8
    assert np.abs(o["A21"] - o["A12"].transpose(0, 2, 1)).max() == 0.0
    # a body whose resistance has no inverse (all blobs at the tracking point: K^T M^-1 K is rank 3): flagged
    K_bad = K.copy(); K_bad[0, :, 3:] = 0.0
    ctx.rigid_preconditioner_device(dev(Mb), dev(K_bad), *out.values(), info)
    assert int(info) == 1
    # and a matrix that is not positive definite
    Mb_bad = Mb.copy(); Mb_bad[-1] = -Mb_bad[-1]
    ctx.rigid_preconditioner_device(dev(Mb_bad), dev(K), *out.values(), info)
    assert int(info) == 1
    ctx.rigid_preconditioner_device(dev(Mb), dev(K), *out.values(), info)
    assert int(info) == 0                                        # the flag is reset by every call
  finally:
    ctx.close()


def test_native_preconditioner_equals_the_torch_build_and_single_blobs_take_the_pseudo_inverse():
  """RigidSuspension.build_preconditioner through the kernel against native_helpers = False (batched torch.linalg): same
  factors and blocks to rounding; a suspension of single-blob bodies (rank-3 resistance) is flagged by the kernel once
  and keeps the reference's pseudo-inverse route."""
  import torch
  from rigidmultiblobswall_amd import structures as st
  from rigidmultiblobswall_amd.rigid import RigidSuspension
  R, eta = 1.0155, 0.957e-3
  shell = st.icosahedron_shell(0.792079207921 * R)
  a = st.min_blob_separation(shell) / 2
  nb = 50
  loc, quat, _ = st.roller_monolayer(nb, radius=R, seed=3)
  nat = RigidSuspension([shell] * nb, loc, quat, a, eta, device="cuda:0")
  ref = RigidSuspension([shell] * nb, loc, quat, a, eta, device="cuda:0")
  ref.native_helpers = False
  try:
    ref.set_configuration(loc, quat)
    assert rel_err(nat.r_vectors, ref.r_vectors) < 1e-14
    assert rel_err(nat.groups[0].K.cpu().numpy(), ref.groups[0].K.cpu().numpy()) < 1e-14
    nat.build_preconditioner(); ref.build_preconditioner()
    assert nat.groups[0].Linv is not None and ref.groups[0].Linv is None
    for name, tol in (("Lchol", 1e-12), ("Minv", 1e-10), ("Nbody", 1e-10), ("A11", 1e-10), ("A12", 1e-10), ("A21", 1e-10), ("A22", 1e-10)):
      assert rel_err(getattr(nat.groups[0], name).cpu().numpy(), getattr(ref.groups[0], name).cpu().numpy()) < tol, name
    ref._stochastic_factors()
    assert rel_err(nat.groups[0].Linv.cpu().numpy(), ref.groups[0].Linv.cpu().numpy()) < 1e-11
  finally:
    nat.close(); ref.close()
  one = np.zeros((1, 3))
  loc1 = np.random.RandomState(0).rand(30, 3) * 8 + np.array([0, 0, 1.5])
  quat1 = np.tile([1.0, 0, 0, 0], (30, 1))
  s1 = RigidSuspension([one] * 30, loc1, quat1, 0.5, 1.0, device="cuda:0")
  s2 = RigidSuspension([one] * 30, loc1, quat1, 0.5, 1.0, device="cuda:0")
  s2.native_helpers = False
  try:
    s1.build_preconditioner(); s2.build_preconditioner()
    assert len(s1._native_pc_rejected) == 1
    assert rel_err(s1.groups[0].Nbody.cpu().numpy(), s2.groups[0].Nbody.cpu().numpy()) < 1e-12
    FT = np.zeros((30, 6)); FT[:, 2] = -1.0
    U1, _, i1 = s1.solve_mobility_problem(force_torque=FT, tol=1e-10)
    U2, _, i2 = s2.solve_mobility_problem(force_torque=FT, tol=1e-10)
    assert i1["converged"] and rel_err(U1[:, :3], U2[:, :3]) < 1e-8
  finally:
    s1.close(); s2.close()


def test_native_preconditioner_for_the_references_42_blob_shells():
  """Bodies of 42 blobs (multi_bodies/Structures/shell_N_42_Rg_0_8913_Rh_1.vertex through the g9 fixture): the per-body
  factors come from the in-place LDS kernel (Linv is only set by the native path), equal the batched torch.linalg build, and
  the preconditioned solve takes the same iterations either way."""
  import os
  import torch
  from conftest import GOLDEN, load_golden
  from rigidmultiblobswall_amd.rigid import RigidSuspension
  g = load_golden(os.path.join(GOLDEN, "g9_rigid_det_euler_42blob_shells.npz"))
  shell, loc, quat = g["vertex_shell42"], g["locations_shell42"], g["quaternions_shell42"]
  assert len(shell) == 42
  d = np.linalg.norm(shell[:, None] - shell[None], axis=2)
  a, eta = float(np.min(d[d > 0]) / 2), 1.1
  # 6 bodies as the fixture, and 60 of them on a lattice (more workgroups than one per CU is not needed for the check)
  loc60 = np.array([[2.6 * (k % 8), 2.6 * (k // 8), 1.4] for k in range(60)])
  quat60 = np.tile(quat, (10, 1))
  for L_, Q_ in ((loc, quat), (loc60, quat60)):
    nb = len(L_)
    nat = RigidSuspension([shell] * nb, L_, Q_, a, eta, device="cuda:0")
    ref = RigidSuspension([shell] * nb, L_, Q_, a, eta, device="cuda:0")
    ref.native_helpers = False
    try:
      nat.build_preconditioner(); ref.build_preconditioner()
      assert nat.groups[0].Linv is not None and ref.groups[0].Linv is None          # the kernel ran, not torch.linalg
      assert not getattr(nat, "_native_pc_rejected", ())
      for name, tol in (("Lchol", 1e-12), ("Minv", 1e-9), ("Nbody", 1e-9), ("A11", 1e-9), ("A12", 1e-9), ("A21", 1e-9), ("A22", 1e-9)):
        assert rel_err(getattr(nat.groups[0], name).cpu().numpy(), getattr(ref.groups[0], name).cpu().numpy()) < tol, name
      FT = np.zeros((nb, 6)); FT[:, 2] = -1.0; FT[:, 4] = 0.3
      U1, _, i1 = nat.solve_mobility_problem(force_torque=FT, tol=1e-9)
      U2, _, i2 = ref.solve_mobility_problem(force_torque=FT, tol=1e-9)
      assert i1["converged"] and abs(i1["iterations"] - i2["iterations"]) <= 1 and rel_err(U1, U2) < 1e-7
    finally:
      nat.close(); ref.close()


def test_rigid_advance_kernel_matches_the_quaternion_update():
  """x + v dt and quaternion(omega dt) * q (quaternion_integrator_multi_bodies.py:86-91) in one launch against the torch
  formulas of rigid.py, with a scalar step, a per-body step, and a body that does not rotate (|omega| = 0)."""
  import torch
  from rigidmultiblobswall_amd import MobilityContext
  from rigidmultiblobswall_amd.rigid import quaternion_from_rotation_torch, quaternion_multiply_torch
  g = torch.Generator().manual_seed(4)
  nb = 777
  loc = torch.randn(nb, 3, generator=g, dtype=torch.float64).cuda()
  quat = torch.randn(nb, 4, generator=g, dtype=torch.float64)
  quat = (quat / quat.norm(dim=1, keepdim=True)).cuda()
  U = torch.randn(nb, 6, generator=g, dtype=torch.float64).cuda()
  U[5, 3:] = 0.0
  ctx = MobilityContext(0)
  try:
    for dt in (0.013, torch.rand(nb, 1, generator=g, dtype=torch.float64).cuda()):
      l2, q2 = ctx.rigid_advance_device(loc, quat, U, dt)
      l_ref = loc + U[:, :3] * dt
      q_ref = quaternion_multiply_torch(quaternion_from_rotation_torch(U[:, 3:] * dt), quat)
      assert float((l2 - l_ref).abs().max()) < 1e-14 and float((q2 - q_ref).abs().max()) < 1e-14
      assert torch.equal(q2[5], quat[5])
      assert float((q2.norm(dim=1) - 1).abs().max()) < 1e-14
  finally:
    ctx.close()


def test_lanczos_with_the_fused_step_equals_the_plain_recurrence():
  """stochastic_forcing_lanczos with ortho = the fused orthogonalisation against the plain three-term recurrence + full
  re-orthogonalisation: same iteration counts, the same M^{1/2} z to rounding, equal to the dense symmetric square root;
  and an exact breakdown (z an eigenvector: |w| = 0 after one step) is survived."""
  import torch
  from rigidmultiblobswall_amd import MobilityContext
  from rigidmultiblobswall_amd.stochastic import stochastic_forcing_lanczos, stochastic_forcing_eig_symm
  rng = np.random.RandomState(3)
  n = 900
  Q, _ = np.linalg.qr(rng.randn(n, n))
  lam = 10.0 ** rng.uniform(-1.5, 1.0, n)
  M = torch.as_tensor((Q * lam) @ Q.T, device="cuda")
  ctx = MobilityContext(0)
  try:
    for tol in (1e-3, 1e-8):
      z = torch.as_tensor(rng.randn(n), device="cuda")
      a, ia = stochastic_forcing_lanczos(factor=0.7, tolerance=tol, mobility_mult=lambda v: M @ v, z=z)
      b, ib = stochastic_forcing_lanczos(factor=0.7, tolerance=tol, mobility_mult=lambda v: M @ v, z=z,
                                         ortho=ctx.krylov_orthogonalize_device)
      assert ia == ib, (tol, ia, ib)
      assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-10
      if tol < 1e-6:
        ref = stochastic_forcing_eig_symm(M, factor=0.7, z=z)
        assert rel_err(b.cpu().numpy(), ref.cpu().numpy()) < 1e-6
    z = torch.as_tensor(Q[:, 5].copy(), device="cuda")        # eigenvector: the Krylov space is one-dimensional
    b, ib = stochastic_forcing_lanczos(factor=1.0, tolerance=1e-8, mobility_mult=lambda v: M @ v, z=z, ortho=ctx.krylov_orthogonalize_device)
    assert np.all(np.isfinite(b.cpu().numpy())) and rel_err(b.cpu().numpy(), np.sqrt(lam[5]) * Q[:, 5]) < 1e-7
  finally:
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# Step-level parity (tests/_krylov_numpy.py): every launch form of the fused Gram-Schmidt step, the linear combination and
# the norm, one step at a time through entries that enqueue and return -- against the long-double restatement, on bases that
# cannot hide a wrong pass.  No loop runs here.
# ---------------------------------------------------------------------------------------------------------------------
import _krylov_numpy as kn
import _rigid_kernels_numpy as rk

NAN = float("nan")
_ORTHO_CASES = set(kn.ortho_cases())


@pytest.fixture(scope="module")
def kctx():
  from rigidmultiblobswall_amd import MobilityContext
  ctx = MobilityContext(0)
  yield ctx
  ctx.close()


def _dev(x):
  import torch
  return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _run_ortho(ctx, V, rows, w0, low_sync, pad=0, separate=False, pc=None, mapped=False):
  """One rmb_krylov_orthogonalize3_device call on fresh buffers.  pad: ldv = n + pad, the padding holds NaN; separate: v_next
  is a buffer of its own, otherwise row `rows` of V (NaN before the call); pc = (blocks, r1, r2, transpose).
  -> dict of numpy arrays col (rows + 1), w, v, z, mapped"""
  import torch
  from rigidmultiblobswall_amd.context import MappedHostArray
  m, n = V.shape
  Vd = torch.full((m, n + pad), NAN, dtype=torch.float64, device="cuda")
  Vd[:, :n] = _dev(V)
  Vv = Vd[:, :n]
  Vv[rows] = NAN
  w = _dev(w0).clone()
  col = torch.full((rows + 2,), NAN, dtype=torch.float64, device="cuda")
  v = torch.full((n,), NAN, dtype=torch.float64, device="cuda") if separate else Vv[rows]
  z = torch.full((n,), NAN, dtype=torch.float64, device="cuda") if pc else None
  host = MappedHostArray((3, rows + 2)) if mapped else None
  try:
    kw = dict(blocks=pc[0], r1=pc[1], r2=pc[2], transpose=pc[3], z=z) if pc else {}
    ctx.krylov_orthogonalize3_device(Vv, rows, w, col, v, host.dev_ptr + 8 * (rows + 2) if mapped else 0, low_sync=low_sync, **kw)
    torch.cuda.synchronize()
    out = dict(col=col[:rows + 1].cpu().numpy(), w=w.cpu().numpy(), v=v.cpu().numpy().copy(), z=z.cpu().numpy() if pc else None)
    assert np.isnan(col[rows + 1].item())                                   # nothing past the norm
    assert np.array_equal(Vd[:rows, :n].cpu().numpy(), V[:rows])            # the basis is read only
    if mapped:
      out["mapped"] = host.array[1, :rows + 1].copy()
      assert not host.array[0].any() and not host.array[2].any() and host.array[1, rows + 1] == 0.0
  finally:
    if host is not None:
      host.close()
  return out


def _same_bits(a, b):
  return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("col", "w", "v")) and (a["z"] is None or np.array_equal(a["z"], b["z"], equal_nan=True))


def _check(form, f, where, failures):
  for k, x in sorted(f.items()):
    kn.record(form, k, x)
    print("%-12s %-10s %.4f of %.3f  %s" % (form, k, x, kn.bound(k), where))
    if not x <= kn.bound(k):
      failures.append((form, k, x, kn.bound(k), where))


def _ortho_forms(ctx, V, rows, w0, kind, where, failures, pc=None, ref=None):
  """both endings on one case: every statement on the first variant, the other buffer layouts and a second call bit for bit"""
  ref = kn.reference(V[:rows], w0) if ref is None else ref
  outs = {}
  for low_sync in (False, True):
    form = ("low_sync" if low_sync else "four") + ("_pc" if pc else "")
    o = _run_ortho(ctx, V, rows, w0, low_sync, pc=pc, mapped=True)
    f, breakdown = kn.fractions(ref, o["col"], o["w"], o["v"], low_sync, kind == "a")
    _check(form, f, where, failures)
    if breakdown:
      # only the Pythagoras norm on a basis that is not orthonormal can come out <= 0 with w2 != 0 (rows = n - 1 on basis
      # (b)); its bound says so and has been checked; v_next is then inf / nan throughout, as documented
      assert low_sync and kind != "a" and not np.isfinite(o["v"]).any(), where
    assert np.array_equal(o["mapped"], o["col"]), where                        # the mapped column is the device column
    assert _same_bits(o, _run_ortho(ctx, V, rows, w0, low_sync, pc=pc)), where                             # a second call
    assert _same_bits(o, _run_ortho(ctx, V, rows, w0, low_sync, pad=3, separate=True, pc=pc)), where       # ldv = n + 3, own v_next
    outs[low_sync] = o
  # the two endings differ in the norm only: same first update, same second projection
  assert np.array_equal(outs[False]["col"][:rows], outs[True]["col"][:rows]) and np.array_equal(outs[False]["w"], outs[True]["w"]), where
  return outs


@pytest.mark.parametrize("n,rows_list", kn.ORTHO_SHAPES)
def test_gram_schmidt_step_on_orthonormal_and_designed_bases(kctx, n, rows_list):
  """rmb_krylov_orthogonalize3_device, both endings, on bases (a) QR-orthonormal, (b) rows (q_r + 0.3 q_{r+1}) normalised and
  (d) the same with 0.01: the column and w against the long-double restatement within the running bound, the statements that
  hold for any basis, orthogonality on (a); ldv = n and n + 3, v_next as row `rows` of V and as its own buffer, the mapped
  column, a second call -- bit for bit."""
  failures = []
  for rows in rows_list:
    for kind in ("a", "b", "d"):
      if (n, rows, kind) not in _ORTHO_CASES:
        continue
      V, w0 = kn.ortho_case(n, rows, kind)
      _ortho_forms(kctx, V, rows, w0, kind, (n, rows, kind), failures)
  assert not failures, failures


@pytest.mark.parametrize("nb,r1,r2", kn.PC_SHAPES)
def test_gram_schmidt_step_with_the_block_product_in_its_last_launch(kctx, nb, r1, r2):
  """The endings with workgroup = body (ortho_normalise_pc_kernel, ortho_last_pc_kernel) on caller-chosen V and w: the same
  statements, and z = blocks * v_next within the row-wise bound of the block product, on the kernel's own v_next.  Row-scaled
  random blocks; thread = row and wave = row walks (r1 = 96 | 126), absent blocks (r2 = 0), a transposed block (300 bodies:
  L^-T as the Lanczos step passes it)."""
  n = nb * (r1 + r2)
  d = rk.block_case(nb, r1, r1, r2, r2, seed=nb + r1)
  transposed = nb == 300
  blocks = (_dev(d["A11"]), _dev(d["A12"]) if r2 else None, _dev(d["A21"]) if r2 else None, _dev(d["A22"]) if r2 else None)
  pc = (blocks, r1, r2, (transposed, False, False, False))
  A11 = d["A11"].transpose(0, 2, 1) if transposed else d["A11"]
  failures = []
  for rows in kn.PC_ROWS[(nb, r1, r2)]:
    for kind in ("a", "b", "d"):
      if kind == "d" and rows == 1:
        continue
      V, w0 = kn.ortho_case(n, rows, kind)
      ref = kn.reference(V[:rows], w0)
      plain = _ortho_forms(kctx, V, rows, w0, kind, (nb, r1, r2, rows, kind, "no blocks"), [], ref=ref)
      outs = _ortho_forms(kctx, V, rows, w0, kind, (nb, r1, r2, rows, kind), failures, pc=pc, ref=ref)
      for low_sync, o in outs.items():
        form = "low_sync_pc" if low_sync else "four_pc"
        # workgroup = body computes what workgroup = chunk computes: same w, same column, same v_next
        assert all(np.array_equal(o[k], plain[low_sync][k], equal_nan=True) for k in ("col", "w", "v")), (nb, r1, r2, rows, kind, low_sync)
        v1, v2 = o["v"][:nb * r1].reshape(nb, r1), o["v"][nb * r1:].reshape(nb, r2)
        z1, z2 = o["z"][:nb * r1].reshape(nb, r1), o["z"][nb * r1:].reshape(nb, r2)
        fz = rk.block_fraction(z1, A11, d["A12"] if r2 else None, v1, v2, np.zeros((nb, r1)), 1.0, 0.0)
        if r2:
          fz = max(fz, rk.block_fraction(z2, d["A21"], d["A22"], v1, v2, np.zeros((nb, r2)), 1.0, 0.0))
        kn.record(form, "z", fz)
        print("%-12s %-10s %.4f of %.3f  %s" % (form, "z", fz, rk.bound(("block",)), (nb, r1, r2, rows, kind)))
        if not fz <= rk.bound(("block",)):
          failures.append((form, "z", fz, (nb, r1, r2, rows, kind)))
  assert not failures, failures


@pytest.mark.parametrize("delta", kn.LADDER_DELTAS)
def test_gram_schmidt_step_near_breakdown(kctx, delta):
  """w0 = V^T c + delta u on basis (a), delta from 1 down to 0: the norm of either ending within its bound -- for the
  low-synchronisation ending the bound the Pythagoras step |w2|^2 = |w1|^2 - |h2|^2 can guarantee --, v_next normalised and
  orthogonal within theirs.  Where the stored norm is 0 (the documented breakdown: only possible at delta = 0, where w2 is
  rounding noise) every entry of v_next is inf / nan and the two statements about it have no content."""
  V, w0 = kn.ladder_case(delta)
  rows = kn.LADDER_ROWS
  ref = kn.reference(V[:rows], w0)
  failures = []
  for low_sync in (False, True):
    o = _run_ortho(kctx, V, rows, w0, low_sync)
    f, breakdown = kn.fractions(ref, o["col"], o["w"], o["v"], low_sync, True)
    _check("low_sync" if low_sync else "four", f, ("ladder", delta), failures)
    if breakdown:
      assert delta == 0.0 and not np.isfinite(o["v"]).any()
    else:
      assert {"normalise", "orth"} <= set(f)
  assert not failures, failures


@pytest.mark.parametrize("n,rows", kn.EXACT_SHAPES)
def test_gram_schmidt_step_is_exact_on_unit_vector_bases(kctx, n, rows):
  """Basis (c): rows are coordinate unit vectors on either side of the chunk edges, w0 integer-valued -- every result is exact
  and compared bitwise in both endings: the column equals the integers, 3 and 4 off the basis give |w| = 5.0 and
  v_next = w / 5, one-hot vectors on the rows at the four- and eight-row group edges pin each partial slot; a w0 in the span
  and an all-zero w0 give col[rows] = 0.0 and inf / nan in every entry of v_next (the documented breakdown)."""
  for last_free in (False, True):
    V, pos, free = kn.exact_basis(n, rows, last_free)
    for name, w0, col, w_out, in_span in kn.exact_vectors(n, rows, pos, free):
      for low_sync in (False, True):
        o = _run_ortho(kctx, V, rows, w0, low_sync, pad=3 if low_sync else 0, separate=low_sync)
        assert np.array_equal(o["col"], col), (name, last_free, low_sync, o["col"], col)
        assert np.array_equal(o["w"], w_out), (name, last_free, low_sync)
        if in_span:
          assert o["col"][rows] == 0.0 and not np.isfinite(o["v"]).any(), (name, last_free, low_sync)
        else:
          assert np.array_equal(o["v"], w_out / 5.0), (name, last_free, low_sync)


@pytest.mark.parametrize("n,rows", kn.EXACT_SHAPES)
def test_gram_schmidt_step_one_hot_on_either_side_of_every_chunk_edge(kctx, n, rows):
  """Basis (c) once more, w0 = 7 e_p for EVERY position p on either side of a chunk edge (and the first and the last element;
  513 positions at n = 1048577), both endings, bitwise.  Where a basis row sits on p: col = 7 e_r, w = 0, the breakdown.  Off
  the basis: col = 0, w = w0, |w| = 7.0, v_next = e_p.  In each call exactly one per-chunk partial is non-zero -- of the
  dots of pass 1 in the first case, of |w|^2 in the second --, so each chunk's slot is pinned, the one-element last chunk and
  the slots past the 64-lane stride of the partial sums included.  The basis stays on the device."""
  import torch
  V, pos, free = kn.exact_basis(n, rows)
  Vd = _dev(V)
  zero = torch.zeros(n, dtype=torch.float64, device="cuda")
  for p, r in kn.edge_one_hots(n, pos):
    w0 = zero.clone()
    w0[p] = 7.0
    want = np.zeros(rows + 1)
    if r is None:
      want[rows] = 7.0
    else:
      want[r] = 7.0
    for low_sync in (False, True):
      w = w0.clone()
      col = torch.full((rows + 2,), NAN, dtype=torch.float64, device="cuda")
      Vd[rows] = NAN
      kctx.krylov_orthogonalize3_device(Vd, rows, w, col, Vd[rows], low_sync=low_sync)
      assert np.array_equal(col[:rows + 1].cpu().numpy(), want), (p, r, low_sync, col[:rows + 1].cpu().numpy())
      if r is None:
        assert torch.equal(w, w0) and torch.equal(Vd[rows], w0 / 7.0), (p, r, low_sync)
      else:
        assert torch.equal(w, zero) and not bool(torch.isfinite(Vd[rows]).any()), (p, r, low_sync)
  assert torch.equal(Vd[:rows], _dev(V[:rows]))


@pytest.mark.parametrize("k", kn.LINCOMB_K)
def test_linear_combination_with_cancelling_coefficients(kctx, k):
  """rmb_krylov_lincomb_device (vec_lincomb_kernel): y += V[:k]^T coef with V^T coef = -y0 up to a thousandth, ldv = n + 5 with
  NaN in the padding and in the rows past k, coefficients in plain device memory; a second call bit for bit."""
  import torch
  failures = []
  for n in kn.LINCOMB_N:
    V, coef, y0 = kn.lincomb_case(k, n)
    Vd = torch.full((k + 1, n + 5), NAN, dtype=torch.float64, device="cuda")
    Vd[:k, :n] = _dev(V)
    got = []
    for rep in range(2):
      y = _dev(y0).clone()
      kctx.krylov_lincomb_device(y, Vd[:, :n], _dev(coef), k)
      got.append(y.cpu().numpy())
    assert np.array_equal(got[0], got[1]), (k, n)
    _check("vec_lincomb", {"lincomb": kn.lincomb_fraction(got[0], y0, V, coef)}, (k, n), failures)
  assert not failures, failures


def test_norm_over_three_hundred_decades(kctx):
  """rmb_krylov_norm_device (vec_norm_kernel): entries from 1e-150 to 1e150, whose squares and their sum stay inside the range
  of a double, and standard normals, where every entry counts (a dropped one is tenfold outside the bound:
  tests/test_krylov_host.py); lengths on either side of the 1024 threads; the result in plain device memory."""
  import torch
  failures = []
  for n, flat in [(n, flat) for n in kn.VNORM_N for flat in (False, True)]:
    v = kn.vnorm_case(n, flat)
    out = torch.full((3,), NAN, dtype=torch.float64, device="cuda")
    kctx.krylov_norm_device(_dev(v), out[1:2])
    got = out.cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[2]) and np.isfinite(got[1]) and got[1] > 0.0, (n, got)
    _check("vec_norm", {"vnorm": kn.vnorm_fraction(got[1], v)}, (n, flat), failures)
    out2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    kctx.krylov_norm_device(_dev(v), out2)
    assert out2.item() == got[1]
  assert not failures, failures


# ---- one step of the loops, on a resident configuration -----------------------------------------------------------------
# The symmetric pair sweep adds its pair terms with atomics: a product is reproducible to ~1e-15 only, not bit for bit.  The
# statements above need the vector the step orthogonalises exactly, so every sweep here is given an input that is zero except
# at ONE blob: each target then receives one non-zero pair term, the order of the additions no longer matters, and the product
# -- taken once more through the separately tested entries -- is the step's own w0 bit for bit (two calls of a step agree bit
# for bit for the same reason).  The vector that comes out of the operator is dense all the same.
ETA_STEP, A_STEP = 1.3, 0.3


def _body_cloud(n_b, nb, seed):
  """well-separated bodies above the wall: centres on a square lattice of spacing 6, blobs within 1.2 of their centre at
  height 3 -- (N, 3)"""
  rng = np.random.RandomState(seed)
  side = int(np.ceil(np.sqrt(nb)))
  k = np.arange(nb)
  centres = np.stack([6.0 * (k % side), 6.0 * (k // side), np.full(nb, 3.0)], axis=1)
  off = rng.randn(n_b, 3)
  off *= 1.2 / max(1.0, np.abs(off).max() * np.sqrt(3.0))
  if n_b == 1:
    off[:] = 0.0
  return (centres[:, None, :] + off[None, :, :] + 0.05 * rng.randn(nb, n_b, 3)).reshape(-1, 3)


def _padded(V, pad):
  """(m, n) numpy -> view of a (m, n + pad) device buffer whose padding holds NaN"""
  import torch
  m, n = V.shape
  Vd = torch.full((m, n + pad), NAN, dtype=torch.float64, device="cuda")
  Vd[:, :n] = _dev(V)
  return Vd[:, :n]


def _step_statements(form, V, rows, w0, col, w, v, kind, where, failures):
  ref = kn.reference(V[:rows], w0)
  f, breakdown = kn.fractions(ref, col, w, v, True, kind == "a")
  assert not breakdown, where
  _check(form, f, where, failures)


def _z_fraction(form, z, blocks, v, nb, r1, r2, where, failures):
  A11, A12, A21, A22 = blocks
  v1, v2 = v[:nb * r1].reshape(nb, r1), v[nb * r1:].reshape(nb, r2)
  fz = rk.block_fraction(z[:nb * r1].reshape(nb, r1), A11, A12, v1, v2, np.zeros((nb, r1)), 1.0, 0.0)
  if r2:
    fz = max(fz, rk.block_fraction(z[nb * r1:].reshape(nb, r2), A21, A22, v1, v2, np.zeros((nb, r2)), 1.0, 0.0))
  kn.record(form, "z", fz)
  print("%-12s %-10s %.4f of %.3f  %s" % (form, "z", fz, rk.bound(("block",)), where))
  if not fz <= rk.bound(("block",)):
    failures.append((form, "z", fz, where))


_STEP_PARAMS = [(n_b, nb, True) for n_b, nb in kn.STEP_SHAPES] + [(1, 132, False), (12, 10, False), (12, 33, False), (33, 12, False)]


@pytest.mark.parametrize("n_b,nb,wall", _STEP_PARAMS)
def test_one_gmres_and_one_rigid_lanczos_step_in_the_loops_forms(kctx, n_b, nb, wall):
  """rmb_rigid_arnoldi_step2_device and rmb_rigid_lanczos_step_device in the three flag combinations the native loops use
  -- (not ready, not fused), (not ready, fused): the first step of a cycle, (ready, fused): every later one -- on bases (b)
  and (a): the vector the step orthogonalises is the output of block_apply_device / rigid_operator_device (matvec_device and
  block_apply_device for the Lanczos step) on the same input; every statement of the Gram-Schmidt step, where the per-body
  first-pass partials of the finishing launches sit; the fused z / pv within the block-product bound; what is not fused
  bit-equal to the separate entries; two calls bit for bit; the pair-sweep family where the context reports it."""
  import torch
  idx = kn.STEP_SHAPES.index((n_b, nb))
  N, nn = n_b * nb, 3 * n_b
  n3, n = 3 * N, 3 * N + 6 * nb
  rng = np.random.RandomState(1000 * n_b + nb)
  kctx.set_positions(_dev(_body_cloud(n_b, nb, idx).reshape(-1)), A_STEP, None, wall)
  b0, l0 = (idx * 7) % nb, (idx * 5) % n_b                        # the one blob that carries the sweep's input
  blob = 3 * (b0 * n_b + l0) + np.arange(3)
  dense = dict(A11=rng.randn(nb, nn, nn) / np.sqrt(nn), A12=rng.randn(nb, nn, 6), A21=rng.randn(nb, 6, nn) / np.sqrt(nn), A22=rng.randn(nb, 6, 6))
  sparse = dict(dense, A11=np.zeros((nb, nn, nn)), A12=np.zeros((nb, nn, 6)))
  sparse["A11"][b0, 3 * l0:3 * l0 + 3] = dense["A11"][b0, 3 * l0:3 * l0 + 3]
  sparse["A12"][b0, 3 * l0:3 * l0 + 3] = dense["A12"][b0, 3 * l0:3 * l0 + 3]
  K = rng.randn(nb, nn, 6)
  Linv = rng.randn(nb, nn, nn) / np.sqrt(nn)
  Linv_sparse = np.zeros_like(Linv)
  Linv_sparse[b0, :, 3 * l0:3 * l0 + 3] = Linv[b0, :, 3 * l0:3 * l0 + 3]
  Kd = _dev(K)
  failures = []
  js = (kn.STEP_J[idx % 5], kn.STEP_J[(idx + 2) % 5])
  for j, kinds in ((js[0], ("b", "a")), (js[1], ("b", "d"))):
    rows = j + 1
    for kind in kinds:
      for z_ready, fuse in ((False, False), (False, True), (True, True)):
        where = (n_b, nb, wall, j, kind, z_ready, fuse)
        # ---- GMRES ----
        V, _ = kn.ortho_case(n, rows, kind)
        V = np.vstack([V, np.zeros((1, n))])
        blocks = dense if z_ready else sparse
        Bd = [_dev(blocks[k]) for k in ("A11", "A12", "A21", "A22")]
        z_in = torch.zeros(n, dtype=torch.float64, device="cuda")
        if z_ready:
          zi = np.zeros(n)
          zi[blob] = rng.randn(3)
          zi[n3:] = rng.randn(6 * nb)
          z_in = _dev(zi)
        else:
          vj = _dev(V[j])
          kctx.block_apply_device(*Bd, vj[:n3].view(nb, nn), vj[n3:].view(nb, 6), z_in[:n3].view(nb, nn), z_in[n3:].view(nb, 6))
          lam = z_in[:n3].cpu().numpy()
          assert np.count_nonzero(lam) == 3 and np.all(lam[blob] != 0.0)
        w0 = kctx.rigid_operator_device(Kd, z_in, ETA_STEP, torch.full((n,), NAN, dtype=torch.float64, device="cuda")).cpu().numpy()
        got = []
        for rep in range(2):
          Vd = _padded(V, 3 * rep)
          z = z_in.clone() if z_ready else torch.full((n,), NAN, dtype=torch.float64, device="cuda")
          w = torch.full((n,), NAN, dtype=torch.float64, device="cuda")
          col = torch.full((rows + 2,), NAN, dtype=torch.float64, device="cuda")
          kctx.rigid_arnoldi_step2_device(*Bd, Kd, Vd, j, ETA_STEP, z, w, col, z_ready=z_ready, fuse_pc=fuse)
          path = kctx.get_option("last_path")
          assert (path == 0) == (N < 128), (where, path)
          # the operator's finishing launch takes the first-pass dots, one partial per body: inside the fused form, with the
          # symmetric sweep, up to 256 bodies
          assert kctx.get_option("last_krylov_partials") == (nb if fuse and N >= 128 and nb <= 256 else 0), where
          got.append(dict(col=col.cpu().numpy(), w=w.cpu().numpy(), v=Vd[rows].cpu().numpy(), z=z.cpu().numpy()))
        assert all(np.array_equal(got[0][k], got[1][k], equal_nan=True) for k in got[0]), where
        o = got[0]
        assert np.isnan(o["col"][rows + 1])
        _step_statements("gmres_step", V, rows, w0, o["col"][:rows + 1], o["w"], o["v"], kind, where, failures)
        if fuse:
          _z_fraction("gmres_step", o["z"], [blocks[k] for k in ("A11", "A12", "A21", "A22")], o["v"], nb, nn, 6, where, failures)
        else:
          assert np.array_equal(o["z"], z_in.cpu().numpy()), where
        # ---- Lanczos ----
        V, _ = kn.ortho_case(n3, rows, kind)
        V = np.vstack([V, np.zeros((1, n3))])
        L = Linv if z_ready else Linv_sparse
        Ld = _dev(L)
        pv_in = torch.zeros(n3, dtype=torch.float64, device="cuda")
        if z_ready:
          pi = np.zeros(n3)
          pi[blob] = rng.randn(3)
          pv_in = _dev(pi)
        else:
          kctx.block_apply_device(Ld, None, None, None, _dev(V[j]).view(nb, nn), torch.zeros((nb, 0), dtype=torch.float64, device="cuda"),
                                  pv_in.view(nb, nn), torch.zeros((nb, 0), dtype=torch.float64, device="cuda"), transpose=(True, False, False, False))
          assert np.count_nonzero(pv_in.cpu().numpy()) == 3
        mw = kctx.matvec_device("tt", pv_in, ETA_STEP)
        d0 = torch.full((n3,), NAN, dtype=torch.float64, device="cuda")
        kctx.block_apply_device(Ld, None, None, None, mw.view(nb, nn), torch.zeros((nb, 0), dtype=torch.float64, device="cuda"),
                                d0.view(nb, nn), torch.zeros((nb, 0), dtype=torch.float64, device="cuda"))
        w0 = d0.cpu().numpy()
        got = []
        for rep in range(2):
          Vd = _padded(V, 3 * rep)
          pv = pv_in.clone() if z_ready else torch.full((n3,), NAN, dtype=torch.float64, device="cuda")
          mwb, d = (torch.full((n3,), NAN, dtype=torch.float64, device="cuda") for _ in range(2))
          col = torch.full((rows + 2,), NAN, dtype=torch.float64, device="cuda")
          kctx.rigid_lanczos_step_device(Ld, Vd, j, ETA_STEP, pv, mwb, d, col, pv_ready=z_ready, fuse_next=fuse)
          path = kctx.get_option("last_path")
          assert (path == 0) == (N < 128), (where, path)
          # the Lanczos finishing launch takes them whenever it runs (symmetric sweep), up to 256 bodies
          assert kctx.get_option("last_krylov_partials") == (nb if N >= 128 and nb <= 256 else 0), where
          got.append(dict(col=col.cpu().numpy(), w=d.cpu().numpy(), v=Vd[rows].cpu().numpy(), z=pv.cpu().numpy()))
        assert all(np.array_equal(got[0][k], got[1][k], equal_nan=True) for k in got[0]), where
        o = got[0]
        _step_statements("lanczos_step", V, rows, w0, o["col"][:rows + 1], o["w"], o["v"], kind, where, failures)
        if fuse:
          _z_fraction("lanczos_step", o["z"], (L.transpose(0, 2, 1), None, None, None), o["v"], nb, nn, 0, where, failures)
        else:
          assert np.array_equal(o["z"], pv_in.cpu().numpy()), where
  assert not failures, failures


def _basis_with_one_blob_row(kind, rows, n, i, support, rng):
  """kn.basis (a: orthonormal, b / d: coupling 0.3 / 0.01) with row i replaced by a unit vector supported on `support` (one blob) and the other rows built in its
  orthogonal complement: (rows + 1, n)"""
  e = np.zeros(n)
  e[support] = rng.randn(len(support))
  e /= np.linalg.norm(e)
  Q = rng.randn(n, rows + 1)
  Q -= np.outer(e, e @ Q)
  Q, _ = np.linalg.qr(Q)
  Q -= np.outer(e, e @ Q)
  B = Q[:, :rows] + {"a": 0.0, "b": 0.3, "d": 0.01}[kind] * Q[:, 1:]
  V = np.zeros((rows + 1, n))
  V[:rows] = (B / np.linalg.norm(B, axis=0)).T
  V[i] = e
  return V


@pytest.mark.parametrize("N", kn.PLAIN_N)
def test_one_plain_lanczos_step(kctx, N):
  """rmb_lanczos_step_device: the M_tt product whose finishing launch takes the first-pass dots per tile of 64 blobs (up to
  256 tiles: N = 16384; 16448 is 257 tiles and takes the separate dots launch), at blob counts on either side of a tile edge;
  the in-plane and the grand-mobility products, which have no fused dots.  V[i] is a unit vector on one blob (see above), the
  other rows are bases (b) and (a) in its complement; the product is taken once more through matvec_device /
  matvec_op_device."""
  import torch
  rng = np.random.RandomState(N)
  r = rng.rand(N, 3) * np.array([1.0, 1.0, 0.0]) * (N / 0.15) ** 0.5 * A_STEP * 2 + np.array([0.0, 0.0, 2 * A_STEP]) + rng.rand(N, 3) * np.array([0.0, 0.0, 3.0])
  kctx.set_positions(_dev(r.reshape(-1)), A_STEP, None, True)
  products = ("tt", "in_plane", "grand") if N in (129, 193) else ("tt",)
  failures = []
  for i in ((0, 4, 16) if N < 10000 else (0, 4)):
    rows = i + 1
    for product in products:
      dim = 6 * N if product == "grand" else 3 * N
      for kind in (("b", "a", "d") if i == 4 else ("b",)):
        where = (N, i, product, kind)
        k0 = (7 * i + 3) % N
        support = np.concatenate([3 * k0 + np.arange(3), 3 * N + 3 * k0 + np.arange(3)]) if product == "grand" else 3 * k0 + np.arange(3)
        V = _basis_with_one_blob_row(kind, rows, dim, i, support, rng)
        vi = _dev(V[i])
        if product == "grand":
          w0 = torch.cat(kctx.matvec_op_device("grand", (vi[:3 * N].contiguous(), vi[3 * N:].contiguous()), ETA_STEP)).cpu().numpy()
        else:
          w0 = kctx.matvec_device("tt", vi, ETA_STEP, in_plane=product == "in_plane").cpu().numpy()
        got = []
        for rep in range(2):
          Vd = _padded(V, 3 * rep)
          x1 = torch.full((dim,), NAN, dtype=torch.float64, device="cuda")
          col = torch.full((rows + 2,), NAN, dtype=torch.float64, device="cuda")
          kctx.lanczos_step_device("grand" if product == "grand" else "tt", Vd, i, ETA_STEP, x1, col, in_plane=product == "in_plane")
          # one partial per tile of 64 blobs from the plain product's finishing launch, up to 256 tiles; none for the others
          tiles = (N + 63) // 64
          assert kctx.get_option("last_krylov_partials") == (tiles if product == "tt" and tiles <= 256 else 0), where
          assert kctx.get_option("last_path") != 0, where
          got.append(dict(col=col.cpu().numpy(), w=x1.cpu().numpy(), v=Vd[rows].cpu().numpy()))
        assert all(np.array_equal(got[0][k], got[1][k], equal_nan=True) for k in got[0]), where
        o = got[0]
        assert np.isnan(o["col"][rows + 1])
        _step_statements("plain_step", V, rows, w0, o["col"][:rows + 1], o["w"], o["v"], kind, where, failures)
  assert not failures, failures


def test_step_entries_refuse_bad_arguments(kctx):
  """The refusals of every step-level entry."""
  import torch
  from rigidmultiblobswall_amd import MobilityContext, _lib
  t = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
  V, w, col = t(300, 48), t(48), t(301)
  def refused(fn, *a, **k):
    with pytest.raises(_lib.RmbError):
      fn(*a, **k)
  o3 = kctx.krylov_orthogonalize3_device
  refused(o3, V, 257, w, col, V[299])                                                     # more rows than one call takes
  refused(o3, V, 0, w, col, V[299])
  refused(o3, t(300, 47), 3, w, col, V[299])                                             # ldv < n
  blocks = (t(6, 7, 7), t(6, 7, 1), t(6, 1, 7), t(6, 1, 1))
  refused(o3, V, 3, w, col, V[299], blocks=blocks, z=t(48), r1=7, r2=2)                   # 48 is no multiple of 9
  refused(o3, V, 3, w, col, V[299], blocks=blocks, z=t(48), r1=0, r2=0)
  refused(o3, t(4, 8000), 3, t(8000), col, t(8000), blocks=(None,) * 4, z=t(8000), r1=4000, r2=0)      # a body's slices do not fit LDS
  o3(V, 3, w, col, V[299], blocks=blocks, z=t(48), r1=7, r2=1)                            # the same call with the blocks covering the vector
  lc = kctx.krylov_lincomb_device
  refused(lc, w, V, t(300), 257)
  refused(lc, w, V, t(300), 0)
  refused(lc, w, t(300, 47), t(300), 3)
  refused(lc, t(0), V, t(300), 3)
  refused(kctx.krylov_norm_device, t(0), t(1))
  # the steps on a resident configuration: none yet, then one of 20 blobs
  ctx = MobilityContext(0)
  try:
    A11, A12, A21, A22, K = t(4, 15, 15), t(4, 15, 6), t(4, 6, 15), t(4, 6, 6), t(4, 15, 6)
    Vs, z, ws, cs = t(4, 84), t(200), t(200), t(6)                                        # (z, w: room for any body count tried below)
    arn = lambda **k: ctx.rigid_arnoldi_step2_device(A11, A12, A21, A22, K, k.pop("V", Vs), k.pop("j", 0), k.pop("eta", 1.0), z, ws, cs, **k)
    lan = lambda **k: ctx.rigid_lanczos_step_device(A11, k.pop("V", Vs[:, :60]), k.pop("i", 0), k.pop("eta", 1.0), t(200), t(200), t(200), cs, **k)
    pln = lambda product, **k: ctx.lanczos_step_device(product, k.pop("V", Vs[:, :60]), k.pop("i", 0), k.pop("eta", 1.0), t(200), cs, **k)
    for fn in (arn, lan, lambda: pln("tt")):
      refused(fn)                                                                         # no configuration
    r = np.random.RandomState(0).rand(20, 3) * 10 + np.array([0, 0, 1.0])
    ctx.set_positions(_dev(r.reshape(-1)), 0.3, None, True)
    arn(fuse_pc=True); lan(fuse_next=True); pln("tt")                                     # 4 bodies of 5 blobs: accepted
    for fn in (arn, lan):
      refused(fn, j=-1) if fn is arn else refused(fn, i=-1)
      refused(fn, eta=0.0)
    refused(arn, V=t(4, 83))                                                              # ldv < 3 N + 6 n_bodies
    refused(lan, V=t(4, 59))
    A11, K = t(5, 15, 15), t(5, 15, 6)                                                    # 5 bodies of 5 blobs are not the 20 resident ones
    refused(arn); refused(lan)
    refused(pln, 2)                                                                       # no such product
    refused(pln, "grand", in_plane=True, V=t(4, 120))
    refused(pln, "grand")                                                                 # ldv = 60 < 6 N
    refused(pln, "tt", V=t(4, 59))
    refused(pln, "tt", i=256, V=t(258, 60))
    refused(pln, "tt", i=-1)
    refused(pln, "tt", eta=0.0)
    ctx.synchronize()
  finally:
    ctx.close()


def test_zz_worst_fractions_of_the_step_kernels():
  """Prints the worst fraction of its bound per kernel form and statement that the tests above saw (run with -s); the figures
  of profiles/r33_krylov_steps.txt and DESIGN section 4 are this table."""
  print()
  for (form, key), x in sorted(kn.RESULTS.items()):
    limit = rk.bound(("block",)) if key == "z" else kn.bound(key)
    print("worst  %-14s %-10s %.4f of %.3f" % (form, key, x, limit))
    assert x <= limit, (form, key, x, limit)
