"""clusters.Clusters and its command line on the GPU against the numpy restatement (_clusters_numpy.py): the statistics are exact
integers, so every comparison is equality -- of the integers, and of the floats formed from them in one fixed way.  The bond-margin
precondition of test_gpu_clusters.py is asserted on every input."""
import io
import runpy
import sys

import numpy as np
import pytest
import torch

import _clusters_numpy as cn
import _pair_hist_numpy as phnp
from rigidmultiblobswall_amd import clusters

pytestmark = pytest.mark.gpu

N, F = 300, 12
BOX = np.array([16.0, 12.0, 3.0])
L_XY = BOX * np.array([1.0, 1.0, 0.0])
R_CUT = {"xy": 0.6, "xyz": 0.9}      # 1.8 bonds per point in the plane, 1.6 in 3-D
_SHARED = {}


@pytest.fixture(scope="module")
def ctx():
  from rigidmultiblobswall_amd import MobilityContext
  c = MobilityContext(0)
  yield c
  c.close()


def _frames():
  if "frames" not in _SHARED:
    def make(rng):
      return rng.uniform(0, 1, (F, N, 3)) * BOX + rng.randint(-2, 3, (F, N, 3)) * L_XY
    for seed in range(31, 51):
      frames = make(np.random.RandomState(seed))
      if all(cn.bond_margin(frames, L_XY, R_CUT[p], p) > cn.MARGIN for p in R_CUT):
        break
    assert all(cn.bond_margin(frames, L_XY, R_CUT[p], p) > cn.MARGIN for p in R_CUT)
    _SHARED["frames"] = frames
    _SHARED["select"] = np.random.RandomState(6).uniform(size=(F, N)) < 0.7
  return _SHARED["frames"], _SHARED["select"]


def _results(acc):
  return dict(n_selected=acc.n_selected(), n_clusters=acc.n_clusters(), largest=acc.largest(), sum_squares=acc.sum_squares(),
              n_s=acc.size_distribution(), fraction=acc.largest_fraction(), mean=acc.mean_size(), wmean=acc.weight_mean_size(),
              last=acc.labels_last(), text=acc.format())


def _equal(a, b):
  for k in a:
    if isinstance(a[k], np.ndarray):
      assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    else:
      assert a[k] == b[k], k


@pytest.mark.parametrize("plane", ["xy", "xyz"])
@pytest.mark.parametrize("selected", [False, True])
def test_pieces_and_the_restatement(ctx, plane, selected, tmp_path):
  frames, select = _frames()
  sel = select if selected else None
  runs = []
  for cuts in ((12,), (5, 7), (1,) * 12):
    acc = clusters.Clusters(N, L_XY, R_CUT[plane], plane=plane, ctx=ctx)
    k = 0
    for c in cuts:
      piece = frames[k:k + c] if len(cuts) != 2 else torch.from_numpy(frames[k:k + c].copy()).cuda()      # numpy and device pieces
      acc.add_frames(piece, None if sel is None else sel[k:k + c])
      k += c
    runs.append(_results(acc.finish()))
    assert acc.n_frames == F
    with pytest.raises(ValueError, match="after finish"):
      acc.add_frames(frames[:1])
    if len(cuts) == 1:
      acc.write(str(tmp_path / "clusters.txt"))
      assert (tmp_path / "clusters.txt").read_text() == runs[0]["text"]
    acc.close()
  _equal(runs[0], runs[1])
  _equal(runs[0], runs[2])
  lab, siz = cn.labels_sizes(frames, L_XY, R_CUT[plane], plane, sel)
  st = cn.statistics(lab, siz)
  got = runs[0]
  for k in ("n_selected", "n_clusters", "largest", "sum_squares", "n_s"):
    assert got[k].dtype == np.int64 and np.array_equal(got[k], st[k]), k
  assert got["n_s"].size == N + 1 and np.array_equal(got["last"], lab[-1]) and got["last"].dtype == np.int32
  assert got["mean"] == cn.mean_size(st["n_s"]) and got["wmean"] == cn.weight_mean_size(st["n_s"])
  assert np.array_equal(got["fraction"], st["largest"] / st["n_selected"])
  assert got["text"].splitlines() == cn.format_lines(st)
  assert int(np.sum(np.arange(N + 1) * got["n_s"])) == (int(sel.sum()) if selected else N * F)
  assert np.count_nonzero(got["n_s"][3:]) >= 3 and got["n_s"][1] >= 3      # a broad distribution


def test_refused_frames(ctx):
  acc = clusters.Clusters(N, L_XY, 0.5, ctx=ctx)
  with pytest.raises(ValueError, match="whole frames"):
    acc.add_frames(np.zeros((2, N - 1, 3)))
  with pytest.raises(ValueError, match="CUDA float64"):
    acc.add_frames(torch.zeros((1, N, 3)))
  with pytest.raises(ValueError, match="select must hold"):
    acc.add_frames(np.zeros((2, N, 3)), np.ones((2, N - 1), bool))
  with pytest.raises(ValueError, match="select must hold"):
    acc.add_frames(np.zeros((2, N, 3)), np.ones((2, N), np.int32))
  with pytest.raises(ValueError, match="no frame"):
    acc.labels_last()
  assert acc.n_frames == 0 and np.isnan(acc.mean_size()) and acc.format() == ""
  acc.close()


def _by_hand(ctx, frames, L, order, thresh, r_cut_psi, plane):
  """the selection |psi_m| >= thresh from the neighbour sums, in numpy; the threshold margin is asserted"""
  out = ctx.bond_order_frames_device(torch.from_numpy(frames.copy()).cuda(), L, r_cut_psi, (order,), plane=plane).cpu().numpy()
  Nn = out[..., 0]
  safe = np.where(Nn > 0, Nn, 1.0)
  re, im = out[..., 1] / safe, out[..., 2] / safe
  mod = np.sqrt(re * re + im * im)
  assert np.abs(mod[Nn > 0] - thresh).min() > 1e-9
  return (Nn > 0) & (mod >= thresh)


def test_psi_selection_and_command_line(ctx, tmp_path):
  n = 60
  for seed in range(3, 23):
    rng = np.random.RandomState(seed)
    frames = rng.uniform(0, 1, (9, n, 3)) * np.array([7.0, 5.0, 0.5])
    if cn.bond_margin(frames[1::2], (7.0, 5.0, 0.0), 0.8, "xy") > cn.MARGIN:
      break
  used = frames[1::2]      # what --skip 1 --every 2 keeps
  L = np.array([7.0, 5.0, 0.0])
  assert cn.bond_margin(used, L, 0.8, "xy") > cn.MARGIN
  traj = tmp_path / "run.config"
  traj.write_text(phnp.config_text(frames))
  base = [str(traj), str(n), "7.0", "5.0", "0", "--rcut", "0.8", "--plane", "xy", "--skip", "1", "--every", "2"]
  # without a selection
  buf = io.StringIO()      # the module's main(), which `python -m rigidmultiblobswall_amd.clusters` runs
  assert clusters.main(base, out=buf) == 0
  st = cn.statistics(*cn.labels_sizes(used, L, 0.8, "xy"))
  assert buf.getvalue().splitlines() == cn.format_lines(st) and len(st["n_selected"]) == 4
  # --psi 6,0.4,1.2: the same selection done by hand
  sel = _by_hand(ctx, used, L, 6, 0.4, 1.2, "xy")
  assert 0 < sel.sum() < sel.size
  dev = clusters.psi_select(ctx, torch.from_numpy(used.copy()).cuda(), L, 6, 0.4, 1.2, plane="xy")
  assert dev.dtype == torch.bool and np.array_equal(dev.cpu().numpy(), sel)
  buf = io.StringIO()
  assert clusters.main(base + ["--psi", "6,0.4,1.2"], out=buf) == 0
  st = cn.statistics(*cn.labels_sizes(used, L, 0.8, "xy", sel))
  assert buf.getvalue().splitlines() == cn.format_lines(st) and int(st["n_selected"].sum()) == int(sel.sum())
  acc = clusters.Clusters(n, L, 0.8, plane="xy", ctx=ctx).add_frames(used, sel).finish()
  assert acc.format() == buf.getvalue()
  acc.close()
  _SHARED["cli"] = (base + ["--psi", "6,0.4,1.2"], buf.getvalue(), phnp.config_text(frames))


@pytest.mark.filterwarnings("ignore:.*found in sys.modules:RuntimeWarning")      # runpy's note that the test imported the module first
def test_run_as_main_writes_the_same_text_to_standard_output(ctx, tmp_path, capsys, monkeypatch):
  """what `python -m rigidmultiblobswall_amd.clusters` does, through runpy in this process (a child would spend ten seconds on
  imports and the device): the `__main__` guard, sys.argv, the text on sys.stdout and the exit status.  The refusal of a bad
  argument by a real child process is in test_clusters_host.py."""
  if "cli" not in _SHARED:
    test_psi_selection_and_command_line(ctx, tmp_path)
  argv, text, config = _SHARED["cli"]
  traj = tmp_path / "again.config"
  traj.write_text(config)
  monkeypatch.setattr(sys, "argv", ["clusters", str(traj)] + argv[1:])
  capsys.readouterr()
  with pytest.raises(SystemExit) as exc:
    runpy.run_module("rigidmultiblobswall_amd.clusters", run_name="__main__", alter_sys=True)
  assert exc.value.code == 0
  assert capsys.readouterr().out == text
