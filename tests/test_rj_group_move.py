"""The group stretch move with a stationary friend table on leaf-packing records, without a GPU: the specification
(tests/rj_group_move.py) against the fixtures captured from the reference (tests/golden/make_golden_rj_group.py -> tests/golden/
rj_group/) - table, windows, proposals, masks and states bit for bit, and the order of the draws on both streams; the window walk
against the stable argsort it stands for; the walk as a stand-alone program under -fsanitize=address,undefined; the move class's and
the sampler's refusals; the C surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import rj_group_move as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL_L = 1e-12          # the bar tests/test_hip_rj.py holds reference chains to (the oracle's template sum against the reference's)


def _close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.abs(a - b) <= RTOL_L * np.abs(b)), f"{what}: max rel {np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)):.3e}"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", rg.FIXTURES)
def test_specification_lands_on_the_reference(name):
    """Every iteration of every fixture: whether it rebuilt, keys, table, every slot's window, the draws (picks on active leaves, zz's
    and the accept uniforms: the draw order of rng="numpy" on R and on the global stream), the proposal, the accept mask and the
    states behind the move's sweep and behind the birth / death move, windows included."""
    fx = rg.load_fixture(name)
    o = rg.fixture_oracle(fx)
    names = [b.name for b in o.branches]
    assert np.array_equal(o.st.P, fx["P0"])
    _close(o.st.L, fx["L0"], "initial log-like")
    born = carried = 0
    for it in range(int(fx["nsteps"])):
        before = {k: o.start[k].copy() for k in names}
        o.iteration()
        rec, pre = o.trace.pop(), f"it{it}_"
        assert rec["rebuilt"] == bool(fx[pre + "rebuilt"]) == (it % int(fx["n_iter_update"]) == 0)
        for k in names:
            assert np.array_equal(_bits(rec["keys"][k]), _bits(fx[pre + f"keys_{k}"])), f"{name} it{it}: keys of {k}"
            assert np.array_equal(_bits(rec["tab"][k]), _bits(fx[pre + f"tab_{k}"])), f"{name} it{it}: table of {k}"
            assert np.array_equal(rec["start"][k], fx[pre + f"start_{k}"]), f"{name} it{it}: windows of {k}"
            act = rec[f"pre_inds_{k}"]
            assert np.array_equal(rec["picks"][k][act], fx[pre + f"pick_{k}"][act]), f"{name} it{it}: picks of {k} (the global stream's order)"
            assert np.array_equal(_bits(rec["q"][k]), _bits(fx[pre + f"q_{k}"])), f"{name} it{it}: proposal of {k}, dead slots included"
            assert np.array_equal(rec[f"mh_x_{k}"], fx[pre + f"mh_x_{k}"]) and np.array_equal(rec[f"mh_inds_{k}"], fx[pre + f"mh_inds_{k}"])
            assert np.array_equal(o.st.x[k], fx[pre + f"rj_x_{k}"]) and np.array_equal(o.st.inds[k], fx[pre + f"rj_inds_{k}"])
            assert np.array_equal(o.start[k], fx[pre + f"rj_start_{k}"]), f"{name} it{it}: windows behind the swaps of {k}"
            if not rec["rebuilt"]:
                born += int(rec["born"][k].sum())
                kept = act & ~rec["born"][k]
                carried += int((rec["start"][k][kept] == before[k][kept]).sum())
                assert np.array_equal(rec["start"][k][kept], before[k][kept]), "a window stays with its leaf"
        assert np.array_equal(rec["u_zz"], fx[pre + "u_zz"]) and np.array_equal(rec["u_acc"], fx[pre + "u_acc"]), f"{name} it{it}: R's order"
        assert np.array_equal(rec["mh_accepted"], fx[pre + "keep"]), f"{name} it{it}: accept mask"
        assert np.array_equal(rec["logp"], fx[pre + "logp"]) and np.array_equal(rec["mh_P"], fx[pre + "mh_P"])
        _close(rec["logl"], fx[pre + "logl"], f"{name} it{it}: proposal's log-like")
        _close(rec["mh_L"], fx[pre + "mh_L"], f"{name} it{it}: log-like behind the sweep")
        assert np.array_equal(rec["rj_accepted"], fx[pre + "rj_accepted"])
        np.testing.assert_allclose(o.st.betas, fx[pre + "rj_betas"], rtol=1e-13, atol=0)
    assert o.num_proposals == int(fx["mh_num_proposals"]) == 8 and np.array_equal(o.mh_accepted, fx["mh_accepted_total"])
    assert born > 0 and carried > 0


def test_fixtures_hold_the_cases_they_were_made_for():
    fx = rg.load_fixture("grp1")
    assert not fx["inds0_gauss"][1, 2].any() and not fx["inds0_sine"][1, 2].any(), "grp1: the walker without any leaf"
    assert fx["x0_gauss"][0, 1, 0, 1] == fx["x0_gauss"][0, 0, 0, 1] and np.sum(np.diff(fx["it0_keys_gauss"]) == 0) >= 1, "grp1: two cold leaves with the same key"
    assert str(fx["rj_moves"]) == "together" and int(fx["nfriends"]) == 3
    assert np.array_equal(fx["it0_q_gauss"][1, 2], fx["x0_gauss"][1, 2]), "the walker without a leaf keeps every bit"
    fx = rg.load_fixture("grp2")
    assert not fx["inds0_gauss"][0].any() and len(fx["it0_keys_gauss"]) == 0 and int(fx["nfriends"]) == 8, "grp2: an empty table at the first rebuild"
    for it in range(3):
        pre_x = fx["x0_gauss"] if it == 0 else fx[f"it{it - 1}_rj_x_gauss"]
        assert np.array_equal(_bits(fx[f"it{it}_q_gauss"]), _bits(pre_x)), "no table: no leaf moves until the second rebuild"
    assert len(fx["it3_keys_gauss"]) == 8, "... which finds exactly nfriends entries: every window is the whole table"
    assert str(fx["rj_moves"]) == "separate_branches"
    fx = rg.load_fixture("grp3")
    assert "gauss_prior_kind" in fx and "sine_prior_kind" in fx and str(fx["rj_moves"]) == "separate_branches"
    for name in rg.FIXTURES:
        fx = rg.load_fixture(name)
        assert [bool(fx[f"it{i}_rebuilt"]) for i in range(8)] == [True, False, False] * 2 + [True, False]
        assert any(fx[f"it{i}_mh_swaps"].sum() + fx[f"it{i}_rj_swaps"].sum() > 0 and not fx[f"it{i + 1}_rebuilt"] for i in range(7)), "a swap carried a window"


def test_window_walk_is_the_argsort():
    """Rule 2 on random and adversarial keys: the window's keys are the keys of the stable argsort's first nf entries, the same entries
    where the keys are all different (check_window asserts both); duplicates, ties between the sides, tables shorter than nfriends,
    the empty table, keys below / above every entry, signed zeros."""
    rs = np.random.RandomState(0)
    for trial in range(600):
        n = rs.randint(0, 30)
        keys = np.sort(rs.randint(0, 6 if trial % 2 else 10 ** 6, size=n) / 4.0)
        for nf in (1, 2, 3, 7, 64):
            rg.check_window(keys, nf, rs.randint(-2, 30) / 8.0)
            if n:
                rg.check_window(keys, nf, keys[rs.randint(n)])
    dup = np.array([1.0, 1.0, 3.0, 3.0, 3.0, 4.0])
    assert rg.window(dup, 2, 2.0) == 0 and rg.window(dup, 1, 2.0) == 1 and list(rg.argsort_entries(dup, 1, 2.0)) == [0]
    assert rg.window(dup, 2, 4.0) == 4 and list(rg.argsort_entries(dup, 2, 4.0)) == [2, 5], "the argsort's set need not be contiguous"
    assert rg.window(np.zeros(0), 5, 1.0) == 0 and rg.window(dup, 64, 0.0) == 0
    assert rg.window(dup, 3, -9.0) == 0 and rg.window(dup, 3, 9.0) == 3
    z = np.array([-1.0, 0.0, 0.0, 2.0])
    assert rg.window(z, 2, -0.0) == rg.window(z, 2, 0.0) == 1
    k, tab = rg.friend_table(np.array([[[[1.0, -0.0, 0.0]], [[1.0, 0.0, 1.0]], [[1.0, -1.0, 2.0]]]]), np.ones((1, 3, 1), dtype=bool), 1)
    assert list(k) == [-1.0, 0.0, 0.0] and not np.signbit(k[1:]).any() and list(tab[:, 2]) == [2.0, 0.0, 1.0] and np.signbit(tab[1, 1]), "-0.0 keyed as +0.0, stable, rows keep their bits"


def test_window_walk_under_a_sanitizer_build(tmp_path):
    """tools/rj_group_host_check.cpp: a stand-alone program over csrc/hens_rj_group_host.h - the walk the kernels run, held to the brute
    force - built with -fsanitize=address,undefined and run on the CPU.  Where the compiler cannot link the sanitizers' runtimes the
    test is skipped with the linker's message, as tests/test_rj_gibbs_move.py does."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "rj_group_host_check.cpp"), str(tmp_path / "rj_group_host_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", str(probe), "-o", str(tmp_path / "probe")] + san, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no sanitizer runtimes for " + cxx + ": " + (r.stderr.strip().splitlines() or ["no message"])[-1])
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", src, "-o", exe] + san, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_the_move_class_and_its_refusals():
    from eryn_amd.rj import GroupStretchLeafMove, RJEnsembleSampler
    mv = GroupStretchLeafMove(3, {"gauss": 1, "sine": 1}, n_iter_update=3)
    assert (mv.nfriends, mv.n_iter_update, mv.a, mv.num_proposals, mv.accepted) == (3, 3, 2.0, 0, None) and mv.key == {"gauss": 1, "sine": 1}
    assert GroupStretchLeafMove(64, 0).n_iter_update == 100 and GroupStretchLeafMove(4, 2, n_iter_update=1, live_dangerously=True).n_iter_update == 1
    with pytest.raises(ValueError, match=re.escape("n_iter_update must be greather than or equal to 2.")):       # group.py:45-46
        GroupStretchLeafMove(3, 1, n_iter_update=1)
    with pytest.raises(ValueError, match="n_iter_update"):
        GroupStretchLeafMove(3, 1, n_iter_update=0, live_dangerously=True)
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match=re.escape("nfriends must be an integer in [1, 64]")):
            GroupStretchLeafMove(bad, 1)
    for bad in (-1, 1.5, {}, {"gauss": -1}, None):
        with pytest.raises(ValueError, match="key must be"):
            GroupStretchLeafMove(3, bad)
    with pytest.raises(ValueError, match="finite and > 1"):
        GroupStretchLeafMove(3, 1, a=1.0)
    with pytest.raises(NotImplementedError, match="gibbs_sampling_setup is not built for GroupStretchLeafMove"):
        GroupStretchLeafMove(3, 1, gibbs_sampling_setup="gauss")
    # refused before a device context is made: a Python-callable likelihood
    with pytest.raises(NotImplementedError, match="must be a TemplateLikelihood"):
        RJEnsembleSampler(8, {"gauss": 3, "sine": 3}, lambda x: 0.0, None, moves=mv, tempering_kwargs=dict(ntemps=2), nleaves_max={"gauss": 4, "sine": 2})
    doc = GroupStretchLeafMove.__doc__
    assert "only if the resume" in doc and "falls on a rebuild" in doc, "the table is state that a State does not carry: said in the class docstring"


def test_c_surface():
    from eryn_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "hipensemble.h")).read()
    for name, nargs in (("hens_rj_set_group", 5), ("hens_rj_group_rebuild", 1), ("hens_rj_group_step", 5), ("hens_rj_group_debug", 5),
                        ("hens_rj_group_debug_draws", 5)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs, f"{name}: include/hipensemble.h declares {decl}"
    assert _lib.SIGNATURES["hens_rj_set_group"][1][1:3] == [C.c_int32, C.c_int32] and _lib.SIGNATURES["hens_rj_set_group"][1][4] is C.c_double
    assert _lib.RJ_INMODEL_GROUP == 2 and "HENS_RJ_INMODEL_GROUP = 2" in header
    assert "hens_rj_group.h" in _build.HDRS_HOST and "hens_rj_group_host.h" in _build.HDRS_HOST
    src = open(os.path.join(ROOT, "eryn_amd", "csrc", "hens_rj_group.h")).read()
    assert "only\n//    if the resume falls on a rebuild" in src or "only if the resume falls on a rebuild" in src.replace("\n//   ", "")
    assert "group.py:275-278" in src, "the reference's second setup_friends, written down once"
    assert "hens_rj_set_group" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_group_words_collide_with_no_other_draw():
    """The move's keys: PURPOSE_RJ_GROUP (29) | s << 8 for s = 0 .. 64, and the accept uniform rj_acc_key(RJ_MODE_GROUP = 4, 0).  No
    other purpose number in use is 29, and mode 4 is new among the accept keys."""
    hdrs = "".join(open(os.path.join(ROOT, "eryn_amd", "csrc", h)).read() for h in ("hens_kernels.h", "hens_rj.h", "hens_rj_mt.h", "hens_rj_gibbs.h"))
    purposes = [int(v) for v in re.findall(r"PURPOSE_[A-Z_]+ = (\d+)", hdrs)]
    assert purposes.count(29) == 1 and len(set(purposes)) == len(purposes), sorted(purposes)
    assert "RJ_MODE_GROUP = 4" in hdrs and "PURPOSE_RJ_GROUP = 29" in hdrs
    words = [29 | (s << 8) for s in range(65)] + [21 | (mode << 8) | (b << 16) for mode in (1, 2, 3, 4) for b in range(5)]
    assert len(set(words)) == len(words)
