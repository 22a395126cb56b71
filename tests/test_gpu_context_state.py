"""The state a context keeps between calls (csrc/rmb_context.hip, rmb_internal.h): the option table as the boundary shows
it, the mapped host buffers of the synchronous product when they grow and are reused, and the one workspace the native
GMRES and Lanczos loops share while the problem size and the restart length change."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

# key -> (default, how a set value is stored)
OPTIONS = {
    "chunks": (0, "given"), "timing": (0, "given"), "symmetric": (1, "given"), "fused_symmetric": (1, "given"),
    "symx_single": (0, "given"), "deterministic": (0, "given"), "det_workspace_mb": (8192, "floor1"), "sym_wps": (0, "given"),
    "sym_pin": (1, "given"), "free_surface": (0, "bool"), "free_surface_rotation": (0, "bool"), "precision": (64, (32, 64)),
    "force_precision": (0, (0, 32, 64)), "force_cull": (1, "bool"), "force_sort": (1, "bool"), "potential_resort": (16, "floor1"),
    "sym_fine_steps": (0, "floor0"), "sym_coop": (1, (0, 1, 2)), "sym_chunk_steps": (1024, "floor0"),
    "sym_two_targets": (1, "clamp02"), "host_zero_copy_in": (1, "bool"), "gmres_fuse_pc": (1, "bool"), "gmres_fuse_dots": (1, "bool"),
    "krylov_low_sync": (1, "bool"), "lanczos_fuse_finish": (1, "bool"), "host_zero_copy": (786432, "floor0"), "sym_order": (1, "bool"),
    "sym_xcd": (1, "bool"), "sym_oversub": (8, "floor1"), "sym_min_steps": (64, "floor1"), "wave_clock": (0, "diagnostics"),
    "skip_pairs": (0, "diagnostics"),
}
REFUSALS = {"precision": "precision must be 32 or 64", "force_precision": r"force_precision must be 0 \(follow \"precision\"\), 32 or 64",
            "sym_coop": r"sym_coop must be 0 \(never\), 1 \(launches below one resident round\) or 2 \(always\)"}
STORED = {"given": lambda v: v, "floor1": lambda v: max(v, 1), "floor0": lambda v: max(v, 0), "clamp02": lambda v: min(max(v, 0), 2),
          "bool": lambda v: int(v != 0)}
VALUES = (-7, 0, 1, 2, 3, 32, 64, 10 ** 12)       # negative, the edges of every rule, large


def _plain():
  from rigidmultiblobswall_amd import MobilityContext
  return MobilityContext(0)


def _engine():
  from rigidmultiblobswall_amd.multi import MultiContext
  return MultiContext([0, 0])


@pytest.mark.parametrize("make", [_plain, _engine], ids=["context", "multi"])
def test_every_option_has_its_default_and_stores_a_set_value_by_its_rule(make):
  """All 32 keys on a fresh context that launches nothing: the default, then what a negative, an out-of-range and a large
  value read back as; the three validated keys and the two diagnostics of the release library refuse with their texts and
  keep what they had; an unknown key is an error on both sides.  The multi-device engine forwards the same keys."""
  from rigidmultiblobswall_amd._lib import RmbError
  assert len(OPTIONS) == 32
  ctx = make()
  try:
    assert ctx.get_option("diagnostics_build") == 0
    for key, (default, rule) in OPTIONS.items():
      assert ctx.get_option(key) == default, key
    for key, (default, rule) in OPTIONS.items():
      held = default
      for v in VALUES:
        if rule == "diagnostics":
          with pytest.raises(RmbError, match="option \"%s\" exists only in the diagnostics build" % key):
            ctx.set_option(key, v)
        elif isinstance(rule, tuple) and v not in rule:
          with pytest.raises(RmbError, match=REFUSALS[key]):
            ctx.set_option(key, v)
        else:
          ctx.set_option(key, v)
          held = v if isinstance(rule, tuple) else STORED[rule](v)
        assert ctx.get_option(key) == held, (key, v)
      if rule != "diagnostics":
        ctx.set_option(key, default)
      assert ctx.get_option(key) == default, key
    for call in (lambda: ctx.set_option("no_such_option", 1), lambda: ctx.get_option("no_such_option")):
      with pytest.raises(RmbError, match="unknown option: no_such_option"):
        call()
  finally:
    ctx.close()


@pytest.fixture(scope="module")
def clouds():
  from test_gpu_parity import d2_cloud
  out = {}
  for n in (128, 1000):
    r, f, eta, a = d2_cloud(n, seed=20 + n)
    out[n] = (r, f.reshape(-1), np.random.RandomState(n).randn(3 * n), eta, a)
  return out


def test_mapped_hand_off_of_the_host_product_grows_and_is_reused(clouds):
  """rmb_matvec through its mapped input and result buffers at 128 blobs (the smallest size that takes them), at 1000 (both
  are reallocated) and at 128 again (the larger ones are reused), one and two input vectors: bit-identical to the device
  entry on the same context and vectors in the bit-reproducible symmetric mode."""
  import torch
  ctx = _plain()
  try:
    ctx.set_option("deterministic", 2)
    for n in (128, 1000, 128):
      r, f, t, eta, a = clouds[n]
      ctx.set_positions(r, a, np.zeros(3), wall=True)
      fd, td = torch.as_tensor(f, device="cuda"), torch.as_tensor(t, device="cuda")
      for kind, v2, v2d in (("tt", None, None), ("tt_tr", t, td)):
        u = ctx.matvec(kind, f, eta, vec2=v2)
        assert ctx.get_option("last_path") == 2
        ud = ctx.matvec_device(kind, fd, eta, vec2=v2d).cpu().numpy()
        assert np.all(np.isfinite(u)) and np.array_equal(u, ud), (n, kind, rel_err(u, ud))
  finally:
    ctx.close()


def test_mapped_host_array_is_zeroed_and_usable_by_the_gram_schmidt_step():
  """rmb_host_mapped_alloc: zero-filled whatever was freed before it, and its device address receives the column of
  rmb_krylov_orthogonalize2_device."""
  import torch
  from rigidmultiblobswall_amd.context import MappedHostArray
  small = MappedHostArray((8,))
  assert not small.array.any()
  small.array[:] = 3.0
  small.close()
  mapped = MappedHostArray((4096,))
  ctx = _plain()
  try:
    assert mapped.array.shape == (4096,) and not mapped.array.any()
    g = torch.Generator(device="cpu").manual_seed(3)
    Q, _ = torch.linalg.qr(torch.randn(64, 2, generator=g, dtype=torch.float64))
    V = torch.zeros((3, 64), dtype=torch.float64)
    V[:2] = Q.t()
    V = V.cuda()
    w = torch.randn(64, generator=g, dtype=torch.float64).cuda()
    col = torch.zeros(3, dtype=torch.float64, device="cuda")
    ctx.krylov_orthogonalize_device(V, 2, w, col, V[2], col_mapped=mapped.dev_ptr + 8 * 100)
    torch.cuda.synchronize()
    assert float(col[2]) > 0.0 and np.array_equal(mapped.array[100:103], col.cpu().numpy())
    assert not mapped.array[:100].any() and not mapped.array[103:].any()
  finally:
    ctx.close()
    mapped.close()


def test_one_workspace_serves_both_native_loops_while_the_sizes_change():
  """One context under two suspensions (4 and 9 twelve-blob shells): native GMRES with restart 60, the native Lanczos forcing,
  the larger suspension with restart 5 (the device vectors grow, the coefficient rows shrink, several restart cycles), its
  forcing, the first solve again -- each step against the generic Python loops on contexts of their own, with the bounds of
  test_native_gmres_loop_equals_the_python_loop."""
  import torch
  from test_gpu_rigid import _shell_suspension
  ctx = _plain()
  nat, ref, conf = {}, {}, {}
  rng = np.random.RandomState(13)
  try:
    for nb in (4, 9):
      nat[nb], loc, quat = _shell_suspension(nb, seed=nb, ctx=ctx)
      ref[nb], _, _ = _shell_suspension(nb, seed=nb)
      ref[nb].native_gmres = ref[nb].native_lanczos = False
      conf[nb] = (loc, quat)

    def solve(nb, restart):
      s, g = nat[nb], ref[nb]
      s.set_configuration(*conf[nb])          # the shared context holds the last configuration bound
      rhs = torch.as_tensor(rng.randn(s.size), device="cuda:0")
      xn, inn = s.solve(rhs, tol=1e-9, restart=restart)
      xp, ip = g.solve(rhs, tol=1e-9, restart=restart)
      assert inn.get("native_gmres") and "native_gmres" not in ip, (nb, restart)
      assert inn["converged"] and ip["converged"] and inn["iterations"] == ip["iterations"], (nb, restart, inn["iterations"], ip["iterations"])
      assert np.allclose(inn["history"], ip["history"], rtol=1e-6, atol=1e-13), (nb, restart)
      assert rel_err(xn.cpu().numpy(), xp.cpu().numpy()) < 1e-8, (nb, restart, rel_err(xn.cpu().numpy(), xp.cpu().numpy()))
      return inn["iterations"]

    def forcing(nb):
      s, g = nat[nb], ref[nb]
      s.set_configuration(*conf[nb])
      z = torch.as_tensor(rng.randn(3 * s.n_blobs), device="cuda:0")
      m0, calls = s.matvec_count, s.lanczos_native_loop_calls
      a, ia = s.stochastic_forcing(z, 0.37, tol=1e-8)
      b, ib = g.stochastic_forcing(z, 0.37, tol=1e-8)
      # the library's loop ran and was not handed back to the generic one: its + 1 products, + the discarded one
      assert s.lanczos_native_loop_calls == calls + 1 and s.matvec_count - m0 in (ia + 1, ia + 2), (nb, ia, s.matvec_count - m0)
      assert g.lanczos_native_loop_calls == 0 and ia == ib and ia >= 2, (nb, ia, ib)
      assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-8, (nb, rel_err(a.cpu().numpy(), b.cpu().numpy()))

    first = solve(4, 60)
    forcing(4)
    assert solve(9, 5) > 2 * 5        # several restart cycles
    forcing(9)
    assert solve(4, 60) > 0 and first > 0
  finally:
    for s in list(nat.values()) + list(ref.values()):
      s.close()
    ctx.close()
