"""The fixtures of tests/golden/rj_priors/ - the reference's reversible-jump chains under mixed uniform / log-uniform / normal priors
(tests/golden/make_golden_rj_priors.py) - against the pinned oracle on ``TermBranch`` (bit for bit: the specification of
tests/rj_prior_terms.py IS the reference's arithmetic), against ``eryn_amd.prior``'s containers, and - where the reference tree is on the
machine - against a fresh run of the generator."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rj_prior_terms as rp
from tests.test_hip_leaf_kinds import _knife_accepts
from tests.test_prior_terms import needs_reference

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", rp.FIXTURES)
def test_oracle_on_term_branches_reproduces_the_reference(name):
    """Every state of the reference's chain - coordinates of every slot, masks, log-like, log-prior, ladder, swap counts, accept
    counters - bit for bit; births, deaths and -inf priors occur; no accept decision within 1e-12 of the knife edge."""
    fx = rp.load_fixture(name)
    o = rp.fixture_oracle(fx, record=True)
    assert np.array_equal(o.st.P, fx["P0"]) and np.array_equal(o.st.L, fx["L0"])
    n = int(fx["nsteps"])
    assert 6 <= n <= 10 and 2 <= int(fx["T"]) <= 3 and 8 <= int(fx["W"]) <= 12
    cnt, knives = rp.new_counts(len(o.branches)), 0
    for it in range(n):
        o.iteration()
        rec = o.trace.pop()
        knives += _knife_accepts(rec)
        rp.count_record(cnt, rec, o)
        for tag, snap in (("mh", "mh_"), ("rj", "rj_")):
            pre = f"it{it}_{tag}_"
            for b in o.branches:
                assert np.array_equal(rec[snap + f"x_{b.name}"], fx[pre + f"x_{b.name}"]), f"{pre}x_{b.name}"
                assert np.array_equal(rec[snap + f"inds_{b.name}"], fx[pre + f"inds_{b.name}"]), f"{pre}inds_{b.name}"
            assert np.array_equal(rec[snap + "L"], fx[pre + "L"]) and np.array_equal(rec[snap + "P"], fx[pre + "P"]), pre
        assert np.array_equal(rec["mh_accepted"], fx[f"it{it}_mh_accepted"]) and np.array_equal(rec["rj_accepted"], fx[f"it{it}_rj_accepted"])
        assert np.array_equal(o.st.betas, fx[f"it{it}_rj_betas"])
    assert np.array_equal(o.mh_accepted, fx["mh_accepted_total"])
    nm = fx["rj_accepted_total"].shape[0]
    assert np.array_equal(np.stack(o.rj_accepted)[:nm], fx["rj_accepted_total"])
    print(f"{name}: in-model proposals {cnt['proposals']}, -inf prior {cnt['outside']}; decisions changed {cnt['changed']}; accepted births "
          f"{cnt['born'].tolist()}, deaths {cnt['died'].tolist()}; knife-edge decisions {knives}")
    assert knives == 0, "pick another seed in the generator"
    assert cnt["born"].sum() > 0 and cnt["died"].sum() > 0 and cnt["changed"] > 0
    kinds = np.concatenate([fx[f"{k}_prior_kind"] for k in rp.fixture_names(fx)])
    assert set(kinds.tolist()) == {0, 1, 2}, "the fixture mixes uniform_dist, log_uniform and scipy.stats.norm"


@pytest.mark.parametrize("name", rp.FIXTURES)
def test_containers_evaluate_the_fixture_log_prior(name):
    """``eryn_amd.prior`` containers built with the reference's own calls give the fixture's initial log-prior bit for bit."""
    fx = rp.load_fixture(name)
    brs = rp.fixture_branches(fx)
    T, W = int(fx["T"]), int(fx["W"])
    P = np.zeros((T, W))
    for b in brs:
        c = rp.fixture_container(fx[f"{b.name}_prior_kind"], fx[f"{b.name}_box"][:, 0], fx[f"{b.name}_box"][:, 1])
        assert all(np.array_equal(c.prior_terms()[k], b.spec[k]) for k in ("kind", "lo", "hi", "c0", "c1", "c2"))
        v = c.logpdf(fx[f"x0_{b.name}"].reshape(-1, b.ndim)).reshape(T, W, b.nleaves_max)
        v[~fx[f"inds0_{b.name}"]] = 0.0
        P += v.sum(axis=-1)
    assert np.array_equal(P, fx["P0"])


@needs_reference
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_rj_priors.py")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", GOLDEN_OUT=str(tmp_path)))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == sorted(f + ".npz" for f in rp.FIXTURES)
    narrays = 0
    for name in rp.FIXTURES:
        old = rp.load_fixture(name)
        with np.load(tmp_path / (name + ".npz"), allow_pickle=False) as f:
            new = {k: f[k] for k in f.files}
        assert sorted(new) == sorted(old), f"{name}: keys differ"
        for k in old:
            assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k], equal_nan=old[k].dtype.kind == "f"), f"{name}[{k}]"
            narrays += 1
    assert narrays > 300
