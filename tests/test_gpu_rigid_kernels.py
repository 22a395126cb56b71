"""The per-body kernels of the rigid-body solve (csrc/rmb_rigid.hip: rigid_pc_kernel, rigid_pc_large_kernel,
rigid_config_kernel, rigid_advance_kernel) held element by element to the rounding bounds of tests/_rigid_kernels_numpy.py
(derivation, families and the yardstick C there; tests/test_rigid_kernels_host.py checks the yardstick on the CPU): real blob
mobilities at every body size from 1 to 42 blobs, above a wall and unbounded; every residual evaluated in long double from
the kernel's own fp64 outputs."""
import numpy as np
import pytest

import _rigid_kernels_numpy as rk

pytestmark = pytest.mark.gpu

PC_OUT = ("Lchol", "Linv", "Minv", "Nbody", "A11", "A12", "A21", "A22")


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _dev(x):
  import torch
  return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _precondition(ctx, M, K, info_start=1):
  """one launch with every output pre-filled with NaN -> ({name: numpy}, info)"""
  import torch
  nb, n = M.shape[0], M.shape[1]
  mk = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
  out = dict(Lchol=mk(nb, n, n), Linv=mk(nb, n, n), Minv=mk(nb, n, n), Nbody=mk(nb, 6, 6), A11=mk(nb, n, n), A12=mk(nb, n, 6),
             A21=mk(nb, 6, n), A22=mk(nb, 6, 6))
  info = torch.full((1,), info_start, dtype=torch.int32, device="cuda")
  ctx.rigid_preconditioner_device(_dev(M), _dev(K), *[out[k] for k in PC_OUT], info)
  return {k: v.cpu().numpy() for k, v in out.items()}, int(info)


def _check_launch(o, info, M, K, fam, n_b, where, refs):
  """every body of one launch against its bounds; M: the matrices as the kernel read them"""
  kern = rk.kernel_of(n_b)
  expect = rk.expected_info(fam, n_b)
  assert info == expect, (where, info)
  full = expect == 0
  failures = []
  for b in range(len(M)):
    one = {k: o[k][b] for k in PC_OUT}
    if full:
      assert rk.exact_structure(one) == [], (where, b, rk.exact_structure(one))
    else:
      assert not np.any(np.triu(one["Lchol"], 1)) and not np.any(np.triu(one["Linv"], 1)) and np.array_equal(one["Minv"], one["Minv"].T), (where, b)
    fr = {(q, kern): v for q, v in rk.factor_fractions(one, M[b], K[b], full=full).items()}
    fr.update({(q, fam, kern): v for q, v in rk.e2e_fractions(one, refs[b], rk.E2E if full else ("Minv", "Lchol")).items()})
    for key, v in fr.items():
      print("%s body %d %s: %.4g (bound %.4g)" % (where, b, key, v, rk.bound(key)))
      rk.record(key, v / rk.bound(key))
      if not v <= rk.bound(key):
        failures.append((where, b, key, v, rk.bound(key)))
  assert not failures, failures


@pytest.mark.parametrize("n_b", rk.N_B_ALL)
def test_preconditioner_meets_the_rounding_bounds_at_every_body_size(ctx, n_b):
  """Two families at this n_b (and the exactly collinear rods at ROD_N_B), three bodies per launch, wall and unbounded:
  |L L^T - sym M| <= gamma_{n+1}|L||L^T|, the left (n <= 48) or right (n > 48) residual of L^-1, Minv against the kernel's own
  L^-1, the panels through A12 and A11, N through R N - I, the exact structure, and every output against the long-double
  restatement.  One or two blobs and rods: info = 1 with Lchol, Linv, Minv still inside their bounds."""
  fams = list(rk.families_of(n_b)) + (["rod"] if n_b in rk.ROD_N_B else [])
  for fam in fams:
    for bnd in rk.BOUNDARIES:
      M, K = rk.launch(fam, n_b, bnd)
      o, info = _precondition(ctx, M, K)
      _check_launch(o, info, M, K, fam, n_b, (fam, n_b, bnd), [rk.ext_reference(fam, n_b, bnd, v) for v in range(3)])


@pytest.mark.parametrize("fam,n_b,bnd", rk.SKEW_CASES)
def test_preconditioner_symmetrises_a_visibly_unsymmetric_input(ctx, fam, n_b, bnd):
  """M + S - S^T with |S| = 1e-3 |M|: the same bounds against sym of the matrix as given (a kernel that reads one triangle
  is off by 1e-3)"""
  M, K = rk.launch(fam, n_b, bnd)
  Ms = np.stack([rk.skewed(M[v], v) for v in range(3)])
  assert np.abs(Ms - Ms.transpose(0, 2, 1)).max() > 1e-4 * np.abs(Ms).max()
  o, info = _precondition(ctx, Ms, K)
  _check_launch(o, info, Ms, K, fam, n_b, ("skew", fam, n_b, bnd), [rk.ext_reference(fam, n_b, bnd, v, skew_seed=v) for v in range(3)])


@pytest.mark.parametrize("n_b", rk.INDEPENDENCE_N_B)
def test_preconditioner_bodies_do_not_see_each_other(ctx, n_b):
  """[A, B, bad, C, D] in one launch: info = 1, and A, B, C, D come out bit for bit as from their own single-body launches;
  the flag is reset by the next good call."""
  M, K = rk.independence_launch(n_b)
  o, info = _precondition(ctx, M, K, info_start=0)
  assert info == 1
  for b in range(5):
    o1, info1 = _precondition(ctx, M[b:b + 1], K[b:b + 1], info_start=1)
    assert info1 == (1 if b == 2 else 0), (b, info1)
    if b != 2:
      for k in PC_OUT:
        assert np.array_equal(o[k][b], o1[k][0]), (n_b, b, k)
      assert np.all(np.isfinite(o1["A11"]))


@pytest.mark.parametrize("n_b,nb", rk.CONFIG_SHAPES)
def test_configuration_meets_the_rounding_bound_per_component(ctx, n_b, nb):
  """r, rel within 7 u and 6 u of the sum of |terms| per component (reference components from 1e-6 to 1e3 within a body);
  the quaternions (1, 0, 0, 0) and (0, 1, 0, 0) give rel = ref and diag(1, -1, -1) ref bit for bit; K holds the kernel's own
  rel exactly; NaN-filled outputs are fully written; r does not depend on which outputs are asked for."""
  import torch
  ref, loc, quat = rk.config_case(n_b, nb)
  assert rk.quat_norm_defect(quat) <= rk.UNIT_QUAT_TOL
  assert np.abs(ref).min(axis=(1, 2)).max() <= 1e-6 and np.abs(ref).max(axis=(1, 2)).min() >= 1e3
  nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
  r, rel, K = nan(nb * n_b, 3), nan(nb, n_b, 3), nan(nb, 3 * n_b, 6)
  ctx.rigid_configuration_device(_dev(ref), _dev(loc), _dev(quat), r, rel, K)
  r2 = nan(nb * n_b, 3)
  ctx.rigid_configuration_device(_dev(ref), _dev(loc), _dev(quat), r2)
  assert torch.equal(r2, r)
  r, rel, K = r.cpu().numpy(), rel.cpu().numpy(), K.cpu().numpy()
  assert np.all(np.isfinite(r)) and np.all(np.isfinite(rel)) and np.all(np.isfinite(K))
  assert np.array_equal(rel[0], ref[0])
  if nb > 1:
    assert np.array_equal(rel[1], ref[1] * np.array([1.0, -1.0, -1.0]))
  assert np.array_equal(K, np.stack([rk.build_K(x) for x in rel]))
  for key, v in rk.config_fractions(r, rel, ref, loc, quat).items():
    print("configuration", (n_b, nb), key, "%.4g (bound %.4g)" % (v, rk.bound((key,))))
    rk.record((key,), v / rk.bound((key,)))
    assert v <= rk.bound((key,)), (key, v)


@pytest.mark.parametrize("per_body_dt", (False, True))
@pytest.mark.parametrize("nb", rk.ADVANCE_BODIES)
def test_advance_meets_the_rounding_bound_on_the_ladder_of_angles(ctx, nb, per_body_dt):
  """|omega dt| from 0 over 1e-200 (the squares underflow), 1e-160, 1e-20 ... to 1e3, each with the quaternion (1, 0, 0, 0)
  -- the output is the rotation quaternion itself, every component held to its own size -- and with a random one;
  omega dt = 0 returns the input quaternion bit for bit."""
  import torch
  loc, quat, Uv, dt, ang = rk.advance_case(nb, per_body_dt)
  dt_dev = _dev(dt) if per_body_dt else dt
  l2, q2 = ctx.rigid_advance_device(_dev(loc), _dev(quat), _dev(Uv), dt_dev)
  l2, q2 = l2.cpu().numpy(), q2.cpu().numpy()
  still = ang == 0.0
  assert np.array_equal(q2[still], quat[still])
  for key, v in rk.advance_fractions(l2, q2, loc, quat, Uv, dt).items():
    print("advance", (nb, per_body_dt), key, "%.4g (bound %.4g)" % (v, rk.bound((key,))))
    rk.record((key,), v / rk.bound((key,)))
    assert v <= rk.bound((key,)), (key, v)
