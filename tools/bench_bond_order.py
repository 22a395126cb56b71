#!/usr/bin/env python
"""The bond-orientational order sweeps (rmb_bond_order_frames_device, rmb_pair_field_frames_device) and the lag sums of C_m on one
GPU, next to the same quantities evaluated with torch on the same device and, for the pair correlation, next to the batch pair
histogram on the same frames.

Cases (seeded uniform points in a square box of density ~1.17, z = 0, plane "xy"; orders 4 and 6, r_cut = 1.5):
  pass1_trajectory   neighbour sums, 1000 frames x 1875 points, box 40 x 40          (the reference example's frame size)
  pass2_trajectory   pair correlation of quantise(psi_6) of the same frames, 1000 bins to 20
  pass1_large        neighbour sums, 1 frame x 262 144 points, box 473 x 473
  pass2_large        pair correlation, the same frame, 1000 bins to 20
  cn                 lag sums of 4096 series x 10 000 frames x 100 lags (random psi in the unit disc), origins="window", in the
                     blocks of bondorder.ORIGIN_BLOCK origins BondOrder uses
  bound              no timing: the worst fraction of the derived bound of DESIGN.md 3.9.4 met by the neighbour sums on the shapes
                     of tests/test_gpu_bond_order.py (long-double restatement of tests/_bond_order_numpy.py)

Per case: device time of the WHOLE call from torch events around it, primed (2 calls), median and minimum of --events calls; pairs
= frames n (n - 1) for pass 1 (ordered: every target meets every source), frames n (n - 1) / 2 for pass 2, terms = series x
origins x lags for cn.  Yardsticks, never the code under test itself:
  torch      the same quantity on the same device by broadcasting (pass 1: image, atan2, cos / sin of m theta, masked sums; pass 2:
             image, norm, bin, int64 products, bincount / index_add_) on --torch-frames frames or --torch-rows rows of the large
             frame (its rate is per pair); cn: per lag one product of two slices and a sum.  Primed once, median of --torch-events.
  pair_hist  rmb_pair_histogram_frames_device on the same frames and bins: pass 2 does its work plus one integer multiply-add and a
             second LDS atomic.
Each pass-1 row carries the largest difference from torch's sums on the compared part, each pass-2 row the number of counts by
which the kernel's histogram differs from torch's (pairs within a rounding error of a bin edge may differ).

  python tools/bench_bond_order.py [--out FILE.json] [--events 5] [--torch-events 3] [--cases ...]
--out merges: rows of other cases already in the file are kept.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"trajectory": (1000, 1875, 40.0), "large": (1, 262144, 473.0)}
CASES = ("pass1_trajectory", "pass2_trajectory", "pass1_large", "pass2_large", "cn", "bound")
ORDERS, R_CUT, R_MAX, N_BINS = (4, 6), 1.5, 20.0, 1000
CN = (10000, 4096, 100)
TORCH_PAIRS = 1 << 24      # separations per broadcast


def points(n_frames, n, side, seed):
  g = torch.Generator(device="cuda")
  g.manual_seed(seed)
  x = torch.rand((n_frames, n, 3), dtype=torch.float64, device="cuda", generator=g) * side
  x[:, :, 2] = 0.0
  return x


def timed(call, prime, events):
  for _ in range(prime):
    call()
  ms = []
  for _ in range(events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
  return float(np.median(ms)), float(np.min(ms))


def _image(d, side):
  return d - torch.trunc(d / side + 0.5 * torch.sign(d)) * side


def torch_pass1(frames, side, rows_of_frame=None):
  """[N, Re, Im per order] for every frame (all rows, or the first `rows_of_frame` rows of each)"""
  F, n = frames.shape[0], frames.shape[1]
  m_rows = n if rows_of_frame is None else min(n, rows_of_frame)
  out = torch.zeros((F, m_rows, 1 + 2 * len(ORDERS)), dtype=torch.float64, device="cuda")
  step = max(1, TORCH_PAIRS // n)
  for f in range(F):
    for i0 in range(0, m_rows, step):
      i1 = min(i0 + step, m_rows)
      dx = _image(frames[f, i0:i1, None, 0] - frames[f, None, :, 0], side)
      dy = _image(frames[f, i0:i1, None, 1] - frames[f, None, :, 1], side)
      rho2 = dx * dx + dy * dy
      nb = (rho2 < R_CUT * R_CUT) & (rho2 > 0)
      theta = torch.atan2(dy, dx)
      out[f, i0:i1, 0] = nb.sum(dim=1)
      for k, m in enumerate(ORDERS):
        out[f, i0:i1, 1 + 2 * k] = torch.where(nb, torch.cos(m * theta), 0.0).sum(dim=1)
        out[f, i0:i1, 2 + 2 * k] = torch.where(nb, torch.sin(m * theta), 0.0).sum(dim=1)
  return out


def torch_pass2(frames, field, side, rows_of_frame=None):
  """(counts, sums) over the unordered pairs (i < j) of every frame whose i is among the first `rows_of_frame` rows"""
  F, n = frames.shape[0], frames.shape[1]
  m_rows = n if rows_of_frame is None else min(n, rows_of_frame)
  counts = torch.zeros(N_BINS, dtype=torch.int64, device="cuda")
  sums = torch.zeros(N_BINS, dtype=torch.int64, device="cuda")
  step = max(1, TORCH_PAIRS // n)
  cols = torch.arange(n, device="cuda")
  q = field.to(torch.int64)
  for f in range(F):
    for i0 in range(0, m_rows, step):
      i1 = min(i0 + step, m_rows)
      dx = _image(frames[f, i0:i1, None, 0] - frames[f, None, :, 0], side)
      dy = _image(frames[f, i0:i1, None, 1] - frames[f, None, :, 1], side)
      r = torch.sqrt(dx * dx + dy * dy)
      keep = (cols[None, :] > torch.arange(i0, i1, device="cuda")[:, None]) & (r < R_MAX)
      b = torch.clamp((r * (N_BINS / R_MAX)).long(), max=N_BINS - 1)[keep]
      term = ((q[f, i0:i1, None, 0] * q[f, None, :, 0] + q[f, i0:i1, None, 1] * q[f, None, :, 1] + (1 << 29)) >> 30)[keep]
      counts += torch.bincount(b, minlength=N_BINS)
      sums.index_add_(0, b, term)
  return counts, sums


def psi6_field(ctx, frames, L):
  out = ctx.bond_order_frames_device(frames, L, R_CUT, (6,), plane="xy")
  N = out[:, :, :1]
  psi = torch.where(N > 0, out[:, :, 1:] / N, torch.zeros_like(out[:, :, 1:]))
  return torch.round(psi * float(2 ** 30)).to(torch.int32).contiguous()


def run_pass(name, args, ctx):
  which, shape = name.split("_")
  F, n, side = SHAPES[shape]
  L = (side, side, 0.0)
  frames = points(F, n, side, seed=28)
  row = dict(kind=name, frames=F, points=n, box=side, r_cut=R_CUT, events=args.events, torch_events=args.torch_events)
  sub_f = min(F, args.torch_frames)
  sub_rows = None if shape == "trajectory" else args.torch_rows
  if which == "pass1":
    pairs = F * n * (n - 1)
    out = torch.empty((F, n, 1 + 2 * len(ORDERS)), dtype=torch.float64, device="cuda")
    med, low = timed(lambda: ctx.bond_order_frames_device(frames, L, R_CUT, ORDERS, plane="xy", out=out), 2, args.events)
    t_med, _ = timed(lambda: torch_pass1(frames[:sub_f], side, sub_rows), 1, args.torch_events)
    ref = torch_pass1(frames[:sub_f], side, sub_rows)
    t_pairs = sub_f * ref.shape[1] * (n - 1)
    got = out[:sub_f, :ref.shape[1]]
    row.update(orders=list(ORDERS), work="ordered pairs", neighbours_mean=float(out[..., 0].mean()),
               n_differs_from_torch=int((got[..., 0] != ref[..., 0]).sum()), max_sum_difference_from_torch=float((got[..., 1:] - ref[..., 1:]).abs().max()))
  else:
    pairs = F * n * (n - 1) // 2
    field = psi6_field(ctx, frames, L)
    counts = torch.zeros(N_BINS, dtype=torch.int64, device="cuda")
    sums = torch.zeros(N_BINS, dtype=torch.int64, device="cuda")
    med, low = timed(lambda: ctx.pair_field_correlation_frames_device(frames, field, L, R_MAX, N_BINS, plane="xy", counts=counts, sums=sums), 2, args.events)
    t_med, _ = timed(lambda: torch_pass2(frames[:sub_f], field[:sub_f], side, sub_rows), 1, args.torch_events)
    rows = n if sub_rows is None else min(n, sub_rows)
    t_pairs = sub_f * (rows * (n - 1) - rows * (rows - 1) // 2)
    row.update(n_bins=N_BINS, r_max=R_MAX, work="unordered pairs")
    if sub_rows is None:
      c1, s1 = ctx.pair_field_correlation_frames_device(frames[:sub_f], field[:sub_f], L, R_MAX, N_BINS, plane="xy")
      c2, s2 = torch_pass2(frames[:sub_f], field[:sub_f], side)
      row.update(counted_pairs_compared=int(c1.sum()), counts_differing_from_torch=int((c1 - c2).abs().sum()),
                 sums_equal_where_counts_equal=bool(torch.equal(s1[c1 == c2], s2[c1 == c2])))
    hist = torch.zeros(N_BINS, dtype=torch.int64, device="cuda")
    p_med, p_low = timed(lambda: ctx.pair_histogram_frames_device(frames, L, R_MAX, N_BINS, out=hist), 2, args.events)
    row.update(pair_hist_ms_median=p_med, pair_hist_ms_min=p_low, pair_hist_g_pairs_per_s=pairs / p_med * 1e-6, pass2_over_pair_hist=med / p_med)
  row.update(pairs=pairs, device_ms_median=med, device_ms_min=low, g_pairs_per_s=pairs / med * 1e-6, torch_pairs=t_pairs, torch_ms_median=t_med,
             torch_g_pairs_per_s=t_pairs / t_med * 1e-6, torch_over_hip=(t_med / t_pairs) / (med / pairs))
  return row


def run_cn(args, ctx):
  from rigidmultiblobswall_amd import bondorder
  F, n, n_lags = CN
  g = torch.Generator(device="cuda")
  g.manual_seed(28)
  psi = (torch.rand((F, n, 2), dtype=torch.float64, device="cuda", generator=g) - 0.5) * np.sqrt(2.0)
  out = torch.zeros((n_lags, n), dtype=torch.float64, device="cuda")
  B = bondorder.ORIGIN_BLOCK
  n_o = F - n_lags + 1

  def hip():
    full = n_o - n_o % B
    for b in range(0, full, B):
      ctx.scattering_lags_device(psi[b:b + B + n_lags - 1], n_lags, origins="window", out=out)
    if n_o > full:
      ctx.scattering_lags_device(psi[full:], n_lags, origins="window", out=out)

  def by_torch():
    C = torch.zeros(n_lags, dtype=torch.float64, device="cuda")
    for lag in range(n_lags):
      C[lag] = (psi[lag:lag + n_o] * psi[:n_o]).sum()
    return C
  med, low = timed(hip, 1, args.events)
  t_med, _ = timed(by_torch, 1, args.torch_events)
  out.zero_()
  hip()
  C, Ct = out.sum(dim=1), by_torch()
  terms = n * n_o * n_lags
  return dict(kind="cn", frames=F, series=n, lags=n_lags, origins=n_o, origin_block=B, terms=terms, device_ms_median=med, device_ms_min=low,
              g_terms_per_s=terms / med * 1e-6, torch_ms_median=t_med, torch_g_terms_per_s=terms / t_med * 1e-6, torch_over_hip=t_med / med,
              max_relative_difference_from_torch=float(((C - Ct).abs() / Ct.abs().max()).max()), events=args.events, torch_events=args.torch_events)


def run_bound(ctx):
  sys.path.insert(0, os.path.join(ROOT, "tests"))
  import _bond_order_numpy as bo
  box = np.array([7.0, 5.0, 3.0])
  worst, rows = 0.0, []
  for n, F, periods in ((65, 5, (1, 1, 0)), (130, 2, (0, 0, 0)), (513, 1, (1, 1, 1)), (513, 1, (0, 0, 0))):
    L = box * np.asarray(periods, dtype=np.float64)
    make = lambda rng: rng.uniform(0, 1, (F, n, 3)) * box + rng.randint(-2, 3, (F, n, 3)) * L      # noqa: E731
    for plane in ("xy", "xyz"):
      frames = bo.frames_with_margin(make, L, 1.1, plane, seed=n)
      dev = torch.from_numpy(frames).cuda()
      for orders in ((6,), (1, 4, 12, 16)):
        N, S, ratio = bo.neighbour_sums(frames, L, 1.1, orders, plane)
        out = ctx.bond_order_frames_device(dev, L, 1.1, orders, plane=plane).cpu().numpy()
        bound = bo.sum_bound(N, ratio, orders)
        err = np.abs(out[..., 1:].reshape(F, n, len(orders), 2).astype(bo.EXT) - S).max(axis=-1).astype(np.float64)
        frac = float((err[bound > 0] / bound[bound > 0]).max())
        rows.append(dict(points=n, frames=F, periods=list(periods), plane=plane, orders=list(orders), n_exact=bool(np.array_equal(out[..., 0], N)),
                         worst_fraction_of_bound=frac))
        worst = max(worst, frac)
  return dict(kind="bound", worst_fraction_of_bound=worst, cases=rows)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--events", type=int, default=5)
  ap.add_argument("--torch-events", type=int, default=3)
  ap.add_argument("--torch-frames", type=int, default=10, help="frames the torch yardstick evaluates")
  ap.add_argument("--torch-rows", type=int, default=2048, help="rows of the large frame the torch yardstick evaluates")
  ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
  args = ap.parse_args()
  from rigidmultiblobswall_amd import MobilityContext
  ctx = MobilityContext(0)
  rows = []
  try:
    for name in args.cases:
      rows.append(run_bound(ctx) if name == "bound" else (run_cn(args, ctx) if name == "cn" else run_pass(name, args, ctx)))
      print(json.dumps(rows[-1]), flush=True)
      torch.cuda.empty_cache()
  finally:
    ctx.close()
  if args.out:
    kept = []
    if os.path.exists(args.out):
      with open(args.out) as fh:
        kept = [r for r in json.load(fh).get("rows", []) if r.get("kind") not in {x["kind"] for x in rows}]
    with open(args.out, "w") as fh:
      json.dump(dict(device=torch.cuda.get_device_name(0), rows=kept + rows), fh, indent=1)


if __name__ == "__main__":
  main()
