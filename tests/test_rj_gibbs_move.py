"""Gibbs blocks over branches and leaf slots for the in-model Gaussian move on leaf-packing records, without a GPU: the specification
(tests/rj_gibbs_move.py) against the fixtures captured from the reference (tests/golden/make_golden_rj_gibbs.py -> tests/golden/
rj_gibbs/), block by block; the setup parser on every form and refusal; the C surface; the table parser as a stand-alone program
under -fsanitize=address,undefined; the new move class beside the refusals that stay."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import rj_gibbs_move as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL_L = 1e-12          # the bar tests/test_hip_rj.py holds reference chains to (the oracle's template sum against the reference's)


def _close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.abs(a - b) <= RTOL_L * np.abs(b)), f"{what}: max rel {np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)):.3e}"


@pytest.mark.parametrize("name", rg.FIXTURES)
def test_specification_lands_on_the_reference_block_by_block(name):
    fx = rg.load_fixture(name)
    o = rg.fixture_oracle(name, fx)
    names = [b.name for b in o.branches]
    nblocks, ran_total, rejected, accepted = int(fx["nblocks"]), 0, 0, 0
    assert np.array_equal(o.st.P, fx["P0"])
    _close(o.st.L, fx["L0"], "initial log-like")
    for it in range(int(fx["nsteps"])):
        o.iteration()
        rec = o.trace[-1]
        ran = [k for k in range(nblocks) if bool(fx[f"it{it}_b{k}_ran"])]
        assert [r["block"] for r in rec["gibbs"]] == ran, f"{name} it{it}: the blocks that ran"
        for r in rec["gibbs"]:
            pre, what = f"it{it}_b{r['block']}_", f"{name} it{it} block {r['block']}"
            for k in names:
                assert np.array_equal(r["q"][k], fx[pre + f"q_{k}"]), f"{what}: proposal of {k} (mask put-back, draw order)"
                assert np.array_equal(r[f"upd_x_{k}"], fx[pre + f"x_{k}"]), f"{what}: coordinates of {k}"
                assert np.array_equal(r[f"upd_inds_{k}"], fx[pre + f"inds_{k}"])
            assert np.array_equal(r["u_acc"], fx[pre + "u_acc"]), f"{what}: accept uniforms"
            assert np.array_equal(r["accepted"], fx[pre + "keep"]), f"{what}: accept mask"
            assert np.array_equal(r["upd_P"], fx[pre + "P"]), f"{what}: log-prior"
            _close(r["upd_L"], fx[pre + "L"], what + ": log-like")
            # rule 4 on this block: a walker without a moved leaf is rejected (-inf) or evaluated as it stands (0.0)
            none = r["here"] == 0
            assert np.all(np.isneginf(r["logp"][none & (r["total"] != 0)])) and np.all(r["logp"][none & (r["total"] == 0)] == 0.0)
            assert not r["accepted"][none & (r["total"] != 0)].any(), f"{what}: a walker without a moved leaf was accepted"
            accepted += int(r["accepted"].sum())
            rejected += int((~r["accepted"]).sum())
        ran_total += len(ran)
        for k in names:
            assert np.array_equal(rec[f"mh_x_{k}"], fx[f"it{it}_mh_x_{k}"]) and np.array_equal(rec[f"mh_inds_{k}"], fx[f"it{it}_mh_inds_{k}"])
        assert np.array_equal(rec["mh_accepted"], fx[f"it{it}_mh_accepted"]), "the move's mask is the last block's that ran"
        assert np.array_equal(rec["mh_P"], fx[f"it{it}_mh_P"])
        _close(rec["mh_L"], fx[f"it{it}_mh_L"], f"{name} it{it}: log-like behind the sweep")
        np.testing.assert_allclose(o.st.betas, fx[f"it{it}_mh_betas"] if str(fx["rj_moves"]) == "none" else fx[f"it{it}_rj_betas"], rtol=1e-13, atol=0)
        if str(fx["rj_moves"]) != "none":
            for k in names:
                assert np.array_equal(o.st.x[k], fx[f"it{it}_rj_x_{k}"]) and np.array_equal(o.st.inds[k], fx[f"it{it}_rj_inds_{k}"])
            assert np.array_equal(rec["rj_accepted"], fx[f"it{it}_rj_accepted"])
        o.trace.clear()
    assert o.num_proposals == ran_total == int(fx["mh_num_proposals"])
    assert np.array_equal(o.mh_accepted, fx["mh_accepted_total"])
    assert accepted > 0 and rejected > 0


def test_fixtures_hold_the_cases_they_were_made_for():
    fx = rg.load_fixture("rjg1")
    assert not fx["inds0_gauss"][0, 2].any() and not fx["inds0_sine"][0, 2].any(), "rjg1: the walker without any leaf"
    assert not fx["inds0_gauss"][1, 3, :2].any() and fx["inds0_gauss"][1, 3, 2] and fx["inds0_sine"][1, 3].any(), "rjg1: no leaf in block 0's slots"
    assert not fx["it0_b0_keep"][1, 3], "rejected by fix_logp_gibbs"
    assert fx["it0_b0_keep"][0, 2] and np.array_equal(fx["it0_b0_x_gauss"][0, 2], fx["x0_gauss"][0, 2]), "the empty walker: accepted, unchanged (logp 0.0 both sides)"
    assert str(fx["rj_moves"]) == "together" and int(fx["mh_num_proposals"]) == 18
    fx = rg.load_fixture("rjg2")
    assert not fx["inds0_gauss"][..., 3].any() and int(fx["mh_num_proposals"]) == 18
    assert not any(bool(fx[f"it{i}_b3_ran"]) for i in range(6)) and all(bool(fx[f"it{i}_b{k}_ran"]) for i in range(6) for k in range(3))
    assert not fx["inds0_gauss"][1, 1, 2] and fx["inds0_gauss"][1, 1, :2].all(), "rjg2: the walker that block 2 finds without a leaf to move"
    fx = rg.load_fixture("rjg3")
    assert str(fx["rj_moves"]) == "separate_branches" and "gauss_prior_kind" in fx and int(fx["nblocks"]) == 2


def test_frozen_coordinates_keep_their_bits_in_the_specification():
    fx = rg.load_fixture("rjg1")
    o = rg.fixture_oracle("rjg1", fx)
    o.st.x["gauss"][:, :, 1, 1] = -0.0                    # slot 1's centre: frozen in block 0, in no other block's member slots
    o.st.P = rg.orj.compute_log_prior(o.st.x, o.st.inds, o.branches)
    before = o.st.x["gauss"][:, :, 1, 1].copy()
    for k in range(3):
        o.block(k)
    assert np.array_equal(o.st.x["gauss"][:, :, 1, 1].view(np.uint64), before.view(np.uint64)) and np.signbit(o.st.x["gauss"][:, :, 1, 1]).all()


def test_by_difference_is_the_full_template_to_rounding():
    """tests/rj_gibbs_move.block_by_difference against the oracle's full evaluation of the same proposal."""
    fx = rg.load_fixture("rjg1")
    o = rg.fixture_oracle("rjg1", fx, record=False)
    from tests import leaf_kinds as lk
    t, y, sigma = o.t, o.y, o.sigma
    tm = np.zeros((o.T, o.W, t.shape[0]))
    for b in o.branches:
        for tt, w, n in zip(*np.where(o.st.inds[b.name])):
            tm[tt, w] += lk.leaf_value(b.kind, o.st.x[b.name][tt, w, n], t)
    for k, blk in enumerate(o.blocks):
        going = rg.moved_leaves(blk, o.st.inds)
        rs = np.random.RandomState(k)
        steps = {b.name: 0.01 * rs.randn(*o.st.x[b.name].shape) for b in o.branches}
        q = rg.propose(blk, o.st.x, going, steps)
        _, L = rg.block_by_difference(o.branches, blk, o.st.x, q, going, tm, t, y, sigma)
        full = rg.orj.template_log_like(q, o.st.inds, o.branches, t, y, sigma)
        has = sum(v.sum(axis=-1) for v in o.st.inds.values()) > 0
        assert np.all(np.abs(L - full)[has] <= 1e-12 * np.abs(full)[has])


# ---- the setup parser --------------------------------------------------------------------------------------------------------------
def _branches():
    from eryn_amd.rj import TemplateBranch
    return [TemplateBranch("gauss", "pulse", [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], 4), TemplateBranch("sine", "sine", [(0.5, 1.5), (1.0, 20.0), (0.0, 6.0)], 2)]


def test_setup_parser_every_form():
    from eryn_amd.rj import leaf_gibbs_table, parse_leaf_gibbs_setup
    brs = _branches()
    gm = rg.RJG1_GAUSS_MASK
    for setup, want in (("sine", [[("sine", None)]]), (("gauss", None), [[("gauss", None)]]), ({"sine": None, "gauss": gm}, [[("sine", None), ("gauss", gm)]]),
                        (rg.fixture_setup("rjg1"), [[("gauss", gm)], [("gauss", rg.RJG1_PAIR["gauss"]), ("sine", rg.RJG1_PAIR["sine"])], [("sine", None)]])):
        got = parse_leaf_gibbs_setup(setup)
        assert [[k for k, _ in blk] for blk in got] == [[k for k, _ in blk] for blk in want]
        for gb, wb in zip(got, want):
            for (_, gmask), (_, wmask) in zip(gb, wb):
                assert (gmask is None and wmask is None) or np.array_equal(gmask, wmask)
    blocks = parse_leaf_gibbs_setup(rg.fixture_setup("rjg1"))
    table, members = leaf_gibbs_table(blocks, brs)
    assert table.dtype == bool and table.shape == (3, 18)
    assert np.array_equal(table, rg.table_of(rg.parse_setup(rg.fixture_setup("rjg1"), brs), brs)), "the table is the specification's, byte for byte"
    assert np.array_equal(table[0], np.r_[gm.reshape(-1), np.zeros(6, dtype=bool)]) and table[2, 12:].all() and not table[2, :12].any()
    assert list(members[1]) == ["gauss", "sine"] and np.array_equal(members[1]["gauss"], [False, False, True, True]) and np.array_equal(members[0]["gauss"], [True, True, False, False])
    # the block's own branch order is kept (the draw order under rng="numpy")
    assert list(leaf_gibbs_table(parse_leaf_gibbs_setup({"sine": None, "gauss": None}), brs)[1][0]) == ["sine", "gauss"]


def test_setup_parser_every_refusal():
    from eryn_amd.rj import GibbsGaussianLeafMove, leaf_gibbs_table, parse_leaf_gibbs_setup
    brs = _branches()
    with pytest.raises(ValueError, match=re.escape("gibbs_sampling_setup must be string, dict, tuple, or list.")):
        parse_leaf_gibbs_setup(3)
    for bad in (["gauss", ["sine"]], ["gauss", 4]):
        with pytest.raises(ValueError, match=re.escape("each item needs to be a string, tuple, or dict")):
            parse_leaf_gibbs_setup(bad)
    for bad in (("gauss", [[1, 1, 1]] * 4), ("gauss", np.ones(3, dtype=bool)), {"gauss": "all"}, ("gauss", None, None)):
        with pytest.raises(ValueError, match=re.escape("second item must be None or 2D np.ndarray")):
            parse_leaf_gibbs_setup(bad)
    with pytest.raises(ValueError, match="holds no block"):
        parse_leaf_gibbs_setup([])
    for setup, text in (("burst", "does not have"), (("gauss", np.ones((3, 3), dtype=bool)), re.escape("(4, 3)")),
                        (("gauss", np.zeros((4, 3), dtype=bool)), "no true entry"), (["sine"] * 129, "at most 128")):
        with pytest.raises(ValueError, match=text):
            leaf_gibbs_table(parse_leaf_gibbs_setup(setup), brs)
    with pytest.raises(ValueError, match="GaussianLeafMove"):
        GibbsGaussianLeafMove({"gauss": np.eye(3)}, None)


def test_the_new_class_constructs_where_the_old_refusals_stay():
    from eryn_amd.rj import GaussianLeafMove, GibbsGaussianLeafMove, RJEnsembleSampler, StretchLeafMove, TemplateLikelihood
    cov = {"gauss": np.eye(3) * 1e-3, "sine": np.eye(3) * 1e-3}
    for make in (lambda: GaussianLeafMove(cov, gibbs_sampling_setup="gauss"), lambda: StretchLeafMove(gibbs_sampling_setup="gauss")):
        with pytest.raises(NotImplementedError, match="over leaves and branches"):
            make()
    mv = GibbsGaussianLeafMove(cov, rg.fixture_setup("rjg1"))
    assert isinstance(mv, GaussianLeafMove) and mv.num_proposals == 0 and mv.accepted is None and len(mv.blocks) == 3
    # refused before a device context is made: a Python-callable likelihood
    with pytest.raises(NotImplementedError, match="must be a TemplateLikelihood"):
        RJEnsembleSampler(8, {"gauss": 3, "sine": 3}, lambda x: 0.0, None, moves=mv, tempering_kwargs=dict(ntemps=2), nleaves_max={"gauss": 4, "sine": 2})
    assert TemplateLikelihood is not None


def test_c_surface():
    from eryn_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "hipensemble.h")).read()
    for name, nargs in (("hens_rj_set_gibbs", 3), ("hens_rj_gibbs_select", 2), ("hens_rj_gibbs_debug_draws", 5)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs, f"{name}: include/hipensemble.h declares {decl}"
    assert _lib.SIGNATURES["hens_rj_set_gibbs"][1][1] is C.c_int32 and _lib.SIGNATURES["hens_rj_gibbs_debug_draws"][1][1:3] == [C.c_int64, C.c_int32]
    assert "hens_rj_gibbs.h" in _build.HDRS_HOST and "hens_rj_gibbs_host.h" in _build.HDRS_HOST
    src = open(os.path.join(ROOT, "eryn_amd", "csrc", "hens_rj_gibbs.h")).read()
    assert "<< 25" in src and "<< 19" in src and "k << 25" in header and "k << 19" in header, "the block's place in the draws' keys, stated in both"
    assert "hens_rj_set_gibbs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_block_words_collide_with_no_other_draw():
    """rj_normal_key uses bits 0 - 24 (PURPOSE_MH_NORMAL | (i | 0x10000) << 8, i < 128), rj_acc_key bits 0 - 18 (purpose | mode << 8 |
    branch << 16, branch <= 4): the block index above them; block 0's words are the words without a table."""
    from tests import production_draws as pd
    normal = lambda i, k: pd.PURPOSE_MH_NORMAL | ((i | 0x10000) << 8) | (k << 25)      # noqa: E731
    acc = lambda mode, branch, k: 21 | (mode << 8) | (branch << 16) | (k << 19)         # noqa: E731
    assert max(normal(127, 0), 0) < 1 << 25 and max(acc(3, 4, 0), 0) < 1 << 19
    words = [normal(i, k) for i in range(128) for k in range(128)] + [acc(1, 0, k) for k in range(128)]
    words += [acc(m, b, 0) for m in (2, 3) for b in range(5)]
    assert len(set(words)) == len(words) and max(words) < 2 ** 32


# ---- the stand-alone program of the table parser -------------------------------------------------------------------------------------
def test_table_parser_under_a_sanitizer_build(tmp_path):
    """tools/rj_gibbs_host_check.cpp: a stand-alone program over csrc/hens_rj_gibbs_host.h - every refusal of the table parser and the
    accepted tables byte for byte - built with -fsanitize=address,undefined and run on the CPU.  Where the compiler cannot link the
    sanitizers' runtimes the test is skipped with the linker's message, as tests/test_gibbs_move.py does."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "rj_gibbs_host_check.cpp"), str(tmp_path / "rj_gibbs_host_check")
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
