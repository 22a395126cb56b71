"""The restatement of the cluster analysis (_clusters_numpy.py) against a brute-force closure, the statistics identities, and
the refusals of clusters.Clusters, of the command line's parser and of the C entries that need no device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _clusters_numpy as cn
from rigidmultiblobswall_amd import clusters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOXES = ((0.0, 0.0, 0.0), (3.0, 2.5, 0.0), (3.0, 2.5, 2.0))


def _cloud(rng, n, L):
  span = np.array([3.0, 2.5, 2.0])
  return rng.uniform(0, 1, (n, 3)) * span + rng.randint(-2, 3, (n, 3)) * np.asarray(L)


@pytest.mark.parametrize("plane", ["xy", "xyz"])
@pytest.mark.parametrize("L", BOXES)
def test_restatement_against_the_brute_force_closure(L, plane):
  rng = np.random.RandomState(7)
  seen = 0
  for n in (1, 2, 5, 9, 12):
    for r_cut in (0.6, 1.1):      # about 0.7 and 4.4 neighbours per point at 12 points in the open 3-D box: below and above percolation
      x = _cloud(rng, n, L)
      sel = rng.uniform(size=n) < 0.7
      for s in (None, sel):
        adj = cn.bonds(x, L, r_cut, plane, s)
        assert np.array_equal(adj, adj.T) and not adj.diagonal().any()
        lab = cn.components(adj, s)
        assert np.array_equal(lab, cn.closure_labels(adj, s))
        live = lab >= 0
        assert np.all(lab[live] <= np.arange(n)[live]) and np.all(lab[lab[live]] == lab[live])      # the minimum, itself a root
        seen += int(cn.sizes_of(lab).max(initial=0) >= 3)
  assert seen >= 3      # the clouds do form clusters


def test_restatement_against_scipy():
  csgraph = pytest.importorskip("scipy.sparse.csgraph")
  rng = np.random.RandomState(11)
  for L in BOXES:
    x = _cloud(rng, 150, L)
    for plane in ("xy", "xyz"):
      adj = cn.bonds(x, L, 0.35, plane)
      k, comp = csgraph.connected_components(adj, directed=False)
      lab = cn.components(adj)
      assert len(np.unique(lab)) == k
      for c in range(k):
        members = np.nonzero(comp == c)[0]
        assert np.all(lab[members] == members.min())


def test_minimal_image_planes_ties_and_stacks():
  L = (4.0, 4.0, 0.0)
  pair = np.array([[0.125, 2.0, 0.0], [3.875 + 3 * 4.0, 2.0 - 5 * 4.0, 0.0]])      # 0.25 apart through the images
  assert cn.labels_sizes(pair, L, 0.5)[0].tolist() == [[0, 0]] and cn.labels_sizes(pair, (0, 0, 0), 0.5)[0].tolist() == [[0, 1]]
  tie = np.array([[0.0, 0.0, 0.0], [0.75, 0.0, 0.0]])      # dyadic: r^2 = 0.5625 exactly
  assert cn.labels_sizes(tie, L, 0.75)[0].tolist() == [[0, 1]]      # d = r_cut: not bonded
  assert cn.labels_sizes(tie, L, np.nextafter(0.75, np.inf))[0].tolist() == [[0, 0]]
  assert cn.bond_margin(tie, L, 0.75) == 0.0
  stack = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 5.0], [1.0, 1.0, 0.0]])
  assert cn.labels_sizes(stack, L, 0.5, "xy")[0].tolist() == [[0, 0, 0]]
  lab, siz = cn.labels_sizes(stack, L, 0.5, "xyz")
  assert lab.tolist() == [[0, 1, 0]] and siz.tolist() == [[2, 1, 0]]
  # L_z is ignored under xy, used under xyz
  zz = np.array([[0.0, 0.0, 0.1], [0.0, 0.0, 1.9]])
  assert cn.labels_sizes(zz, (0, 0, 2.0), 0.5, "xyz")[0].tolist() == [[0, 0]] and cn.labels_sizes(zz, (0, 0, 0), 0.5, "xyz")[0].tolist() == [[0, 1]]


def test_selection_and_statistics_identities():
  rng = np.random.RandomState(3)
  L = (3.0, 2.5, 0.0)
  frames = np.stack([_cloud(rng, 40, L) for _ in range(6)])
  sel = rng.uniform(size=(6, 40)) < 0.6
  sel[2] = False
  sel[3] = True
  for s in (None, sel):
    lab, siz = cn.labels_sizes(frames, L, 0.45, "xy", s)
    st = cn.statistics(lab, siz)
    n_sel = 6 * 40 if s is None else int(s.sum())
    assert int(st["n_selected"].sum()) == n_sel
    assert int(np.sum(np.arange(41) * st["n_s"])) == n_sel                 # sum s n_s = selected points x frames
    assert int(st["n_s"].sum()) == int(st["n_clusters"].sum())            # sum n_s = sum of the clusters per frame
    assert np.all(st["largest"] <= st["n_selected"]) and st["n_s"][0] == 0
    if s is not None:
      assert np.all(lab[~s] == -1) and np.all(lab[s] >= 0) and st["n_clusters"][2] == 0 and st["largest"][2] == 0
      assert np.all(siz[2] == 0)
    assert cn.mean_size(st["n_s"]) == n_sel / st["n_clusters"].sum()
    assert clusters.number_mean(st["n_s"]) == cn.mean_size(st["n_s"]) and clusters.weight_mean(st["n_s"]) == cn.weight_mean_size(st["n_s"])
  # an all-true selection is no selection; a selected point among unselected ones is a singleton
  a, b = cn.labels_sizes(frames, L, 0.45, "xy", np.ones((6, 40), bool)), cn.labels_sizes(frames, L, 0.45, "xy")
  assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
  one = np.zeros((1, 40), bool)
  one[0, 17] = True
  lab, siz = cn.labels_sizes(frames[:1], L, 10.0, "xy", one)
  assert lab[0, 17] == 17 and siz[0, 17] == 1 and siz.sum() == 1 and (lab >= 0).sum() == 1


def test_clusters_refuses_bad_arguments_before_any_device():
  L = (4.0, 3.0, 0.0)
  C = clusters.Clusters
  with pytest.raises(ValueError, match="n_points"):
    C(-1, L, 1.0)
  with pytest.raises(ValueError, match="n_points must not exceed"):
    C(2 ** 31, L, 1.0)
  with pytest.raises(ValueError, match="plane must be"):
    C(5, L, 1.0, plane="xz")
  with pytest.raises(ValueError, match="three lengths"):
    C(5, (4.0, 3.0), 1.0)
  for r_cut in (0.0, -1.0, float("inf"), float("nan"), None):
    with pytest.raises(ValueError, match="r_cut must be positive"):
      C(5, L, r_cut)


def test_command_line_parser_refuses():
  good = ["run.config", "10", "4", "3", "0", "--rcut", "1.0"]
  args, psi = clusters.parse_args(good + ["--psi", "6,0.7,1.5", "--plane", "xy", "--every", "2", "--skip", "1"])
  assert psi == (6, 0.7, 1.5) and args.plane == "xy" and args.every == 2 and args.skip == 1 and args.np == 10 and args.rcut == 1.0
  assert clusters.parse_args(good)[1] is None and clusters.parse_args(good)[0].plane == "xyz"
  for bad in (good[:5], good[:5] + ["--rcut", "0"], good[:5] + ["--rcut", "inf"], good[:5] + ["--rcut", "nan"], good + ["--plane", "xz"],
              good + ["--every", "0"], good + ["--skip", "-1"], good + ["--psi", "6,0.7"], good + ["--psi", "0,0.7,1.5"],
              good + ["--psi", "17,0.7,1.5"], good + ["--psi", "6,x,1.5"], good + ["--psi", "6,0.7,0"], good + ["--psi", "6,0.7,1.5,2"],
              ["run.config", "-3", "4", "3", "0", "--rcut", "1.0"]):
    with pytest.raises(SystemExit) as exc:
      clusters.parse_args(bad)
    assert exc.value.code == 2, bad


def test_python_m_refuses_a_bad_argument_with_status_2_and_no_output():
  """the module run as a program: the parser's refusal goes to stderr, before anything touches a device"""
  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
  run = subprocess.run([sys.executable, "-m", "rigidmultiblobswall_amd.clusters", "run.config", "10", "4", "3", "0", "--rcut", "-1"], env=env,
                       capture_output=True, text=True, timeout=120)
  assert run.returncode == 2 and "--rcut must be positive" in run.stderr and run.stdout == ""


def _declared():
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rmb_mobility.h")).read(), flags=re.S)
  return sorted(set(re.findall(r"\b(rmb_[a-z0-9_]+)\s*\(", src)))


def test_header_library_and_ctypes_table_agree():
  from rigidmultiblobswall_amd import _lib
  names = _declared()
  lib = ctypes.CDLL(_lib.LIB_PATH)
  assert len(names) == len(_lib.SYMBOLS) == sum(hasattr(lib, n) for n in names)
  for name in ("rmb_cluster_labels_frames_device", "rmb_cluster_labels_device"):
    assert name in names and name in _lib.SYMBOLS and hasattr(lib, name)


def test_c_entries_refuse_bad_arguments_without_a_device():
  """Every argument check comes before the context is looked at; the outputs stay as they were."""
  from rigidmultiblobswall_amd import _lib
  lib, ARG = _lib.load(), -1      # RMB_ERR_ARG
  buf, L = np.zeros(3 * 2 * 3), np.array([4.0, 3.0, 0.0])
  labels, sizes = np.full(6, 7, dtype=np.int32), np.full(6, 7, dtype=np.int32)
  p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
  good = dict(frames=p(buf), select=None, n_frames=3, n=2, L=p(L), r_cut=1.5, plane=0, labels=p(labels), sizes=p(sizes))
  bad = [(dict(labels=None), "null labels or sizes"), (dict(sizes=None), "null labels or sizes"), (dict(frames=None), "null frames"),
         (dict(L=None), "null periodic_length"), (dict(n_frames=-1), "negative size"), (dict(n=-1), "negative size"),
         (dict(r_cut=0.0), "r_cut must be positive and finite"), (dict(r_cut=-2.0), "r_cut must be positive and finite"),
         (dict(r_cut=float("inf")), "r_cut must be positive and finite"), (dict(r_cut=float("nan")), "r_cut must be positive and finite"),
         (dict(plane=2), "plane must be 0 (xyz) or 1 (xy)"), (dict(plane=-1), "plane must be 0 (xyz) or 1 (xy)"),
         (dict(n_frames=2 ** 20, n=2 ** 11), "too many points"), (dict(n_frames=1, n=2 ** 31), "too many points"), (dict(), "null context")]
  for change, message in bad:
    a = dict(good, **change)
    rc = lib.rmb_cluster_labels_frames_device(None, a["frames"], a["select"], a["n_frames"], a["n"], a["L"], a["r_cut"], a["plane"],
                                              a["labels"], a["sizes"])
    assert rc == ARG, change
    assert message in lib.rmb_last_error().decode(), (change, lib.rmb_last_error())
  for change, message in bad:
    if set(change) & {"frames", "L", "n_frames", "n"}:
      continue
    a = dict(good, **change)
    rc = lib.rmb_cluster_labels_device(None, a["select"], a["r_cut"], a["plane"], a["labels"], a["sizes"])
    assert rc == ARG, change
    assert message in lib.rmb_last_error().decode(), (change, lib.rmb_last_error())
  assert np.all(labels == 7) and np.all(sizes == 7)
