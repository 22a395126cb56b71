"""Host logic of the Metropolis sampler replayed against the reference driver's recorded chains (g14_mcmc_*), with the numpy
restatement as the energy function: draw order, acceptance, step-size adaptation, output numbering, .MCMC_info text; the
restatement against every logged energy; the refusal of CUDA-string potentials."""
import os

import numpy as np
import pytest

import _potential_numpy as potnp
from _mcmc_common import FIXTURES, IDS, assert_chain_matches, info_numbers, load_case
from rigidmultiblobswall_amd.read_input import ReadInput


def _energy_fn(read, form):
  kw = dict(periodic_length=read.periodic_length, debye_length_wall=read.debye_length_wall, repulsion_strength_wall=read.repulsion_strength_wall,
            debye_length=read.debye_length, repulsion_strength=read.repulsion_strength, weight=1.0 * read.g, blob_radius=read.blob_radius,
            potential=form)
  return lambda r: potnp.total(r, **kw)


def _sampler(path, tmp_path, monkeypatch, **kw):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  g, deck = load_case(path, str(tmp_path))
  monkeypatch.chdir(tmp_path)
  read = ReadInput(deck)
  return g, MCMCSampler(read, potential=str(g["potential"]), energy=_energy_fn(read, str(g["potential"])), keep_saved=True, **kw)


def test_fixtures_are_there():
  assert len(FIXTURES) >= 4


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_host_replay_of_the_reference_chain(path, tmp_path, monkeypatch):
  g, s = _sampler(path, tmp_path, monkeypatch)
  s.run()
  # the restatement reproduces every logged energy (the chains visit z <= 0, z < a and r < 2a) ...
  assert_chain_matches(s, g, 1e-13)
  # ... and the files: names and numbering of the saves, the four .MCMC_info lines
  read = s.read
  text = open("run.MCMC_info").read().splitlines()
  assert [t.split("=")[0] for t in text] == [str(t).split("=")[0] for t in g["mcmc_info"]]
  assert np.allclose(info_numbers(text), info_numbers(g["mcmc_info"]), rtol=1e-14, atol=0)
  assert text[1] == str(g["mcmc_info"][1])
  for f in ("run.inputfile", "run.random_state", "run.time"):
    assert os.path.isfile(f)
  assert open("run.inputfile").read() == str(g["deck"])
  for k, ID in enumerate(read.structures_ID):
    if read.save_clones == "one_file_per_step":
      names = sorted(n for n in os.listdir(".") if n.startswith("run.%s." % ID) and n.endswith(".clones"))
      assert names == ["run.%s.%08d.clones" % (ID, int(st)) for st in g["saved_steps"]]
    else:
      rows = open("run.%s.config" % ID).read().splitlines()
      nb = g["start_loc_%d" % k].shape[0]
      assert len(rows) == (nb + 1) * len(g["saved_steps"]) and all(rows[i] == str(nb) for i in range(0, len(rows), nb + 1))
      last = np.array([r.split() for r in rows[-nb:]], dtype=np.float64)
      assert np.max(np.abs(last[:, :3] - g["saved_loc_%d" % k][-1])) <= 1e-12


def test_the_fixtures_cover_the_special_regions():
  """Blobs at z <= 0, z < a and pairs at r < 2a all occur in the start configurations the logs begin with."""
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  seen = {"behind": 0, "low": 0, "overlap": 0}
  for path in FIXTURES:
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
      g, deck = load_case(path, tmp)
      s = MCMCSampler(ReadInput(deck), energy=lambda r: 0.0, write_files=False, check_user_potential=False)
      r = s.state._blobs(s.loc0, s.quat0)
      a = s.blob_radius
      d = np.linalg.norm(r[:, None] - r[None], axis=-1)[np.triu_indices(len(r), 1)]
      seen["behind"] += int(np.sum(r[:, 2] <= 0)); seen["low"] += int(np.sum((r[:, 2] > 0) & (r[:, 2] < a))); seen["overlap"] += int(np.sum(d < 2 * a))
  assert all(v > 0 for v in seen.values()), seen


def test_prescribed_bodies_do_not_move(tmp_path, monkeypatch):
  path = [p for p in FIXTURES if "prescribed" in p][0]
  g, s = _sampler(path, tmp_path, monkeypatch, write_files=False)
  s.run()
  loc, quat = s.state.configuration()
  assert s.n_free == g["start_loc_0"].shape[0] and s.n_bodies > s.n_free
  assert np.array_equal(loc[s.n_free:], g["start_loc_1"]) and np.array_equal(quat[s.n_free:], g["start_quat_1"])
  assert not np.array_equal(loc[:s.n_free], g["start_loc_0"])


def test_adaptation_changes_the_step_size(tmp_path, monkeypatch):
  path = [p for p in FIXTURES if "adaptation" in p][0]
  g, s = _sampler(path, tmp_path, monkeypatch, write_files=False)
  start = s.max_translation
  s.run()
  assert s.max_translation != start and s.max_translation == pytest.approx(float(g["max_translation"]), rel=1e-14)


def test_batched_draws_are_another_stream_of_the_same_chain_logic(tmp_path, monkeypatch):
  g, s = _sampler(FIXTURES[0], tmp_path, monkeypatch, write_files=False, rng="batched")
  s.run()
  g2, s2 = _sampler(FIXTURES[0], tmp_path, monkeypatch, write_files=False, rng="batched")
  s2.run()
  assert s.energy_log == s2.energy_log and s.accepted == s2.accepted                    # repeatable
  assert s.energy_log[0] == g["energy_log"][0] and s.energy_log[1] != g["energy_log"][1]  # same start, other stream


def test_nan_and_inf_energies_reject(tmp_path, monkeypatch):
  from rigidmultiblobswall_amd.mcmc import MCMCSampler
  g, deck = load_case(FIXTURES[0], str(tmp_path))
  monkeypatch.chdir(tmp_path)
  for bad in (np.nan, np.inf):
    calls = []
    def energy(r, bad=bad, calls=calls):
      calls.append(1)
      return 1.0 if len(calls) == 1 else bad
    s = MCMCSampler(ReadInput(deck), energy=energy, write_files=False).run()
    assert s.accepted_moves == 0 and not any(s.accepted)


def test_user_defined_cuda_potential_is_refused(tmp_path, monkeypatch):
  from rigidmultiblobswall_amd import mcmc
  g, deck = load_case(FIXTURES[0], str(tmp_path))
  monkeypatch.chdir(tmp_path)
  with open("potential_pycuda_user_defined.py", "w") as f:
    f.write("# a CUDA string would be here\n")
  with pytest.raises(mcmc.UserDefinedPotentialError) as err:
    mcmc.MCMCSampler(ReadInput(deck), energy=lambda r: 0.0)
  assert "--potential yukawa" in str(err.value) and "not supported" in str(err.value)
  with pytest.raises(mcmc.UserDefinedPotentialError):
    mcmc.main(["data.main"])
