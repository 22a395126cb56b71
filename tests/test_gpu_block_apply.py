"""The batched two-by-two block product (block_rows.h, block_apply_kernel, rmb_block_apply_device) row by row: every row
within gamma_{c1+c2+2} (|alpha| (|A11||x1| + |A12||x2|) + |beta y0|) of the long-double product -- tightened to MARGIN C, see
tests/_rigid_kernels_numpy.py -- with the rows of one block scaled by powers of ten from 1e-8 to 1e8, so that a wrong entry in
a small row is as visible as one in a large row."""
import numpy as np
import pytest

import _rigid_kernels_numpy as rk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _dev(x):
  import torch
  return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _check(ctx, where, x1, x2, y1_0, y2_0, al, be, blocks, dev_blocks=None, transpose=(False,) * 4):
  """blocks: the four (batch, rows, cols) numpy arrays as the product sees them, or None; dev_blocks: what is handed to
  the kernel instead (strided views, untransposed storage).  beta = 0: the outputs start as NaN and must not be read."""
  import torch
  dev_blocks = [None if b is None else _dev(b) for b in blocks] if dev_blocks is None else dev_blocks
  y1 = _dev(y1_0) if be != 0.0 else torch.full(y1_0.shape, float("nan"), dtype=torch.float64, device="cuda")
  y2 = _dev(y2_0) if be != 0.0 else torch.full(y2_0.shape, float("nan"), dtype=torch.float64, device="cuda")
  ctx.block_apply_device(*dev_blocks, _dev(x1), _dev(x2), y1, y2, alpha=al, beta1=be, beta2=be, transpose=transpose)
  for name, y, (A, B), y0 in (("top", y1, blocks[:2], y1_0), ("bottom", y2, blocks[2:], y2_0)):
    v = rk.block_fraction(y.cpu().numpy(), A, B, x1, x2, y0, al, be)
    print("block", where, name, "%.4g (bound %.4g)" % (v, rk.bound(("block",))))
    rk.record(("block",), v / rk.bound(("block",)))
    assert v <= rk.bound(("block",)), (where, name, v)


@pytest.mark.parametrize("c1", rk.BLOCK_COLS)
def test_every_row_count_at_this_column_count(ctx, c1):
  """rows 1 .. 129 (the four-rows-per-wave tail, the thread-count steps of two_by_two_threads) x this c1, lower blocks 6 x 6;
  alpha, beta in {0, 1, -1, 0.5} and the batch in {1, 3} cycle over the cases"""
  for nb, r1, cc, r2, c2, al, be, seed in rk.block_cases():
    if cc == c1 and r2 == 6 and seed < 9500:
      d = rk.block_case(nb, r1, cc, r2, c2, seed)
      _check(ctx, (nb, r1, cc, al, be), d["x1"], d["x2"], d["y1"], d["y2"], al, be, [d["A11"], d["A12"], d["A21"], d["A22"]])


@pytest.mark.parametrize("n_b", rk.PC_SHAPES_NB)
def test_the_preconditioners_shapes(ctx, n_b):
  for nb, r1, c1, r2, c2, al, be, seed in rk.block_cases():
    if seed >= 9500 and r1 == 3 * n_b:
      d = rk.block_case(nb, r1, c1, r2, c2, seed)
      _check(ctx, ("pc", nb, n_b, al, be), d["x1"], d["x2"], d["y1"], d["y2"], al, be, [d["A11"], d["A12"], d["A21"], d["A22"]])


@pytest.mark.parametrize("label", [str(c[0]) for c in rk.block_extra_cases()])
def test_transposed_strided_and_absent_blocks(ctx, label):
  """A21 = B^T with B stored (c1, r2): long strided rows, walked wave = row up to 8 rows and thread = row above; the operator's
  own use (top = y - K U, bottom = -K^T lambda from one K); every block a slice of a larger tensor; one block absent in each
  position; c1 = 0"""
  (_, how, d, al, be, blocks), = [c for c in rk.block_extra_cases() if str(c[0]) == label]
  dev_blocks, transpose = None, (False,) * 4
  if how == "transposed":
    dev_blocks = [_dev(blocks[0]), _dev(blocks[1]), _dev(np.ascontiguousarray(blocks[2].transpose(0, 2, 1))), _dev(blocks[3])]
    transpose = (False, False, True, False)
  elif how == "operator":
    K = _dev(blocks[1])
    dev_blocks, transpose = [None, K, K, None], (False, False, True, False)
  elif how == "strided":
    rng = np.random.RandomState(9801)
    keep, dev_blocks = [], []
    for A in blocks:
      g = rng.randn(A.shape[0], A.shape[1] + 3, A.shape[2] + 2)
      g[:, 1:1 + A.shape[1], 2:2 + A.shape[2]] = A
      keep.append(_dev(g))
      dev_blocks.append(keep[-1][:, 1:1 + A.shape[1], 2:2 + A.shape[2]])
  _check(ctx, label, d["x1"], d["x2"], d["y1"], d["y2"], al, be, blocks, dev_blocks=dev_blocks, transpose=transpose)
