"""Gibbs parameter blocks on the CPU: the specification (tests/gibbs_move.py) against the reference's recorded chains
(tests/golden/gibbs/), the ``gibbs_sampling_setup`` parser of eryn_amd.moves against the reference's accepted and refused forms, the
C surface, the mask parser and block image of csrc/hens_gibbs_host.h under a sanitizer build, and the sizing of every GPU case of
tests/test_hip_gibbs.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import gibbs_move as gm
from tests import production_draws as pd
from tests import tolerance_log as tol

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the specification lands on the reference's chains ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gm.FIXTURES)
def test_specification_lands_on_the_reference(name):
    fx = gm.load_fixture(name)
    box = bool(np.all(fx["prior_kind"] == 0))
    books = None
    for it, (xm, Lm, Pm, ret), (x, L, P, betas, sw), books in gm.replay_fixture(fx):
        pre, what = f"it{it}_", f"{name}, iteration {it}"
        assert np.array_equal(ret, fx[pre + "accepted"]), f"{what}: the mask propose() returns"
        assert np.array_equal(xm.view(np.uint64), fx[pre + "x_move"].view(np.uint64)), f"{what}: positions after the move"
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(fx[pre + "x"]).view(np.uint64)), f"{what}: positions after the sweep"
        if box:
            assert np.array_equal(Pm, fx[pre + "P_move"]) and np.array_equal(P, fx[pre + "P"]), f"{what}: log-prior"
        else:
            np.testing.assert_allclose(P, fx[pre + "P"], rtol=1e-13, atol=0, err_msg=f"{what}: log-prior")
        tol.check_logl(Lm, fx[pre + "L_move"], tol.RTOL_L, what)
        tol.check_logl(L, fx[pre + "L"], tol.RTOL_L, what)
        assert np.array_equal(sw, fx[pre + "swaps_accepted"]), f"{what}: swap counts"
        np.testing.assert_allclose(betas, fx[pre + "betas"], rtol=1e-13, atol=0, err_msg=f"{what}: betas")
    for tag in ("stretch", "gauss"):
        if "accepted_" + tag in fx:
            assert np.array_equal(books["accepted_" + tag], fx["accepted_" + tag]), f"{name}: move.accepted of the {tag} move"
            assert books["num_proposals_" + tag] == int(fx["num_proposals_" + tag]), f"{name}: num_proposals of the {tag} move"


def test_fixtures_show_the_references_rules():
    """What the issue read off the real reference: num_proposals advances per block, a coordinate in no block keeps its multiset
    of values over the ensemble, and the red-blue move's running OR counts a walker of block 0 again in block 1."""
    g1 = gm.load_fixture("g1_stretch_blocks")
    assert int(g1["num_proposals_stretch"]) == 12 and g1["accepted_stretch"].max() == 12
    per_block = sum(int((g1[f"it{i}_b{b}_keep{s}"]).sum()) for i in range(6) for b in range(2) for s in range(2))
    assert g1["accepted_stretch"].sum() > per_block, "the running OR counts more than the accepted block proposals"
    assert np.array_equal(np.sort(g1["x0"][..., 3].reshape(-1)), np.sort(g1["it5_x"][..., 3].reshape(-1)))
    g2 = gm.load_fixture("g2_gauss_blocks")
    per_block = sum(int(g2[f"it{i}_b{b}_keep"].sum()) for i in range(6) for b in range(2))
    assert int(g2["num_proposals_gauss"]) == 12 and g2["accepted_gauss"].sum() == per_block
    assert all(np.array_equal(g2[f"it{i}_accepted"], g2[f"it{i}_b1_keep"]) for i in range(6)), "the MH move returns the last block's mask"
    g3 = gm.load_fixture("g3_mix_overlap")
    assert np.array_equal(np.sort(g3["x0"][..., 5].reshape(-1)), np.sort(g3["it5_x"][..., 5].reshape(-1)))
    assert int(g3["num_proposals_stretch"]) + int(g3["num_proposals_gauss"]) == 12
    assert {int(g3[f"it{i}_kind"]) for i in range(6)} == {0, 1}


# ---- the setup parser ---------------------------------------------------------------------------------------------------------------------------
def _m(*bits):
    return np.array([bits], dtype=bool)


ACCEPTED = {
    "a branch name": ("model_0", [[1, 1, 1, 1]]),
    "a tuple with a mask": (("model_0", _m(1, 1, 0, 0)), [[1, 1, 0, 0]]),
    "a tuple with None": (("model_0", None), [[1, 1, 1, 1]]),
    "a dict": ({"model_0": _m(0, 0, 1, 0)}, [[0, 0, 1, 0]]),
    "a dict with None": ({"model_0": None}, [[1, 1, 1, 1]]),
    "a list of the three": (["model_0", ("model_0", _m(1, 1, 0, 0)), {"model_0": _m(0, 1, 1, 0)}], [[1, 1, 1, 1], [1, 1, 0, 0], [0, 1, 1, 0]]),
}
REFUSED = {
    "a number": (3, "gibbs_sampling_setup must be string, dict, tuple, or list."),
    "an array": (np.ones((1, 4), dtype=bool), "gibbs_sampling_setup must be string, dict, tuple, or list."),
    "a list with a number": (["model_0", 3], "each item needs to be a string, tuple, or dict"),
    "a 1-D mask": (("model_0", np.ones(4, dtype=bool)), "second item must be None or 2D np.ndarray"),
    "a list for a mask": (("model_0", [[True] * 4]), "second item must be None or 2D np.ndarray"),
    "a 1-D mask in a dict": ({"model_0": np.ones(4, dtype=bool)}, "second item must be None or 2D np.ndarray"),
}


@pytest.mark.parametrize("cls", ["StretchMove", "GaussianMove"])
def test_setup_parser_takes_the_references_forms(cls):
    from eryn_amd import moves

    def make(setup, **kw):
        return moves.StretchMove(gibbs_sampling_setup=setup, **kw) if cls == "StretchMove" else moves.GaussianMove({"model_0": 0.1}, gibbs_sampling_setup=setup, **kw)

    assert make(None).gibbs_sampling_setup is None and make(None).gibbs_masks("model_0", 4) is None
    for what, (setup, want) in ACCEPTED.items():
        got = make(setup).gibbs_masks("model_0", 4)
        assert got.dtype == bool and np.array_equal(got, np.asarray(want, dtype=bool).reshape(-1, 4)), what
    for what, (setup, text) in REFUSED.items():
        with pytest.raises(ValueError, match=re.escape(text)):
            make(setup)
    # a mask must be (nleaves_max, ndim) = (1, ndim); a block names this move's one branch
    with pytest.raises(ValueError, match=re.escape("(1, 4)")):
        make(("model_0", np.ones((2, 4), dtype=bool))).gibbs_masks("model_0", 4)
    with pytest.raises(ValueError, match=re.escape("(1, 4)")):
        make(("model_0", np.ones((1, 5), dtype=bool))).gibbs_masks("model_0", 4)
    with pytest.raises(ValueError, match="single branch"):
        make("other").gibbs_masks("model_0", 4)
    with pytest.raises(ValueError, match="single branch"):
        make({"model_0": None, "other": None}).gibbs_masks("model_0", 4)
    with pytest.raises(ValueError, match="empty list"):           # (the reference takes it and proposes nothing: refused here, in both rng modes)
        make([])
    with pytest.raises(ValueError, match="not allowed with an RJ proposal"):
        make(("model_0", _m(1, 1, 0, 0)), is_rj=True)


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/eryn"), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("what", sorted(ACCEPTED) + sorted(set(REFUSED) - {"a 1-D mask", "a list for a mask"}))
def test_setup_parser_against_the_reference_itself(what):
    """The same forms through the reference's own ``Move`` (a fresh interpreter: its import path is not this suite's).  Not the two
    bad tuples: the reference stops in ``breakpoint()`` in front of that ValueError (move.py:151)."""
    code = r"""
import sys, types
for m in ("corner", "seaborn"):
    sys.modules[m] = types.ModuleType(m)
sys.path.insert(0, "/root/reference/src")
sys.path.insert(0, sys.argv[1])
import numpy as np
from eryn.moves import StretchMove
from tests.test_gibbs_move import ACCEPTED, REFUSED
what = sys.argv[2]
setup = (ACCEPTED.get(what) or REFUSED.get(what))[0]
try:
    mv = StretchMove(gibbs_sampling_setup=setup)
except ValueError as e:
    print("REFUSED", " ".join(str(e).split()))
else:
    masks = [np.ones(4, dtype=int) if i[0] is None else np.asarray(i[0][0], dtype=int) for i in mv.inds_run_all]
    print("ACCEPTED", [m.tolist() for m in masks])
"""
    r = subprocess.run([sys.executable, "-c", code, ROOT, what], capture_output=True, text=True, timeout=120, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(("ACCEPTED", "REFUSED"))][-1]
    if what in ACCEPTED:
        assert line == "ACCEPTED " + str(np.asarray(ACCEPTED[what][1], dtype=int).reshape(-1, 4).tolist()), line
    else:
        assert line.startswith("REFUSED") and " ".join(REFUSED[what][1].split()) in line, line


def test_constructors_and_samplers_refuse_what_is_not_built():
    from eryn_amd import moves
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood, HostLikelihood
    from eryn_amd.prior import ProbDistContainer, uniform_dist
    from eryn_amd.rj import GaussianLeafMove, StretchLeafMove
    pri = {0: uniform_dist(-1.0, 1.0), 1: uniform_dist(-1.0, 1.0)}
    with pytest.raises(NotImplementedError, match="DistributionGenerate"):
        moves.DistributionGenerate({"model_0": ProbDistContainer(pri)}, gibbs_sampling_setup="model_0")
    for make in (lambda: StretchLeafMove(gibbs_sampling_setup="pulse"), lambda: GaussianLeafMove({"pulse": np.eye(3)}, gibbs_sampling_setup="pulse")):
        with pytest.raises(NotImplementedError, match="over leaves and branches"):
            make()
    mv = moves.StretchMove(gibbs_sampling_setup=("model_0", _m(1, 0)))
    assert np.array_equal(mv.gibbs_masks("model_0", 2), [[True, False]])
    # a Python likelihood: refused before a device context is made, whichever way it arrives
    for like in (lambda x: -0.5 * (x * x).sum(axis=1), HostLikelihood(lambda x: -0.5 * (x * x).sum(axis=1), 2)):
        with pytest.raises(NotImplementedError, match="needs a device likelihood"):
            EnsembleSampler(8, 2, like, pri, moves=moves.StretchMove(gibbs_sampling_setup=("model_0", _m(1, 0))))
    # the shapes are checked at construction too
    with pytest.raises(ValueError, match=re.escape("(1, 2)")):
        EnsembleSampler(8, 2, GaussianLikelihood(np.zeros(2), np.eye(2)), pri, moves=moves.GaussianMove({"model_0": 0.1}, gibbs_sampling_setup=("model_0", _m(1, 0, 1))))
    # the leaf-packing sampler
    from eryn_amd.rj import RJEnsembleSampler
    with pytest.raises(NotImplementedError, match="over leaves and branches"):
        RJEnsembleSampler(8, {"pulse": 3}, None, None, moves=mv)


def test_c_surface():
    from eryn_amd import _lib
    header = open(os.path.join(ROOT, "include", "hipensemble.h")).read()
    for name, nargs in (("hens_set_gibbs", 4), ("hens_gibbs_select", 3), ("hens_debug_draws_block", 12)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs, f"{name}: include/hipensemble.h declares {decl}"
    assert _lib.SIGNATURES["hens_set_gibbs"][1][1:3] == [C.c_int32, C.c_int32]
    assert _lib.SIGNATURES["hens_debug_draws_block"][1][1:3] == [C.c_int64, C.c_int32]
    assert _lib.SIGNATURES["hens_debug_draws_block"][1][3:] == _lib.SIGNATURES["hens_debug_draws"][1][2:], "the same arrays, one more argument"
    assert re.search(r"enum \{ HENS_GIBBS_STRETCH = 0, HENS_GIBBS_MH = 1 \};", header)
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hens_set_gibbs" in stub and "hens_gibbs_select" in stub and "hens_debug_draws_block" in stub


def test_block_draw_words():
    """Block 0's words are the words of a context without a table; a block's word collides with no other draw's."""
    assert gm.stretch_word(0) == pd.PURPOSE_STRETCH and gm.mh_acc_word(0) == pd.PURPOSE_MH_ACC and gm.mh_normal_word(0, 0) == pd.PURPOSE_MH_NORMAL
    words = [gm.stretch_word(b) for b in range(128)] + [gm.mh_acc_word(b) for b in range(128)]
    words += [gm.mh_normal_word(p, b) for p in range(64) for b in range(128)]
    words += [14 | (d << 8) for d in range(128)] + [pd.PURPOSE_SPLIT, pd.PURPOSE_PTPERM, pd.PURPOSE_PTU, pd.PURPOSE_MOVE, pd.PURPOSE_STRETCH_ACC,
                                                    pd.PURPOSE_SPLIT ^ 0x100, pd.PURPOSE_PTPERM ^ 0x100]
    assert len(set(words)) == len(words) and max(words) < 2 ** 32
    T, W = 3, 70
    p0, p1 = gm.block_plan(5, 2, T, W, 0, 0), gm.block_plan(5, 2, T, W, 0, 1)
    assert all(np.array_equal(p0[k], pd.plan(5, 2, T, W, 0)[k]) for k in p0)
    assert np.array_equal(p0["own"], p1["own"]) and not np.array_equal(p0["u_zz"], p1["u_zz"]) and not np.array_equal(p0["cw"], p1["cw"])
    z0, u0 = gm.mh_block_draws(5, 2, T, W, 8, 0)
    assert np.array_equal(z0, pd.mh_steps(5, 2, T, W, 8, "iso", 1.0)["z"]) and np.array_equal(u0[1], pd.mh_uniform(5, 2, 1, W))
    z1, u1 = gm.mh_block_draws(5, 2, T, W, 8, 1)
    assert not np.array_equal(z0, z1) and not np.array_equal(u0, u1)


def test_frozen_coordinates_keep_their_bits():
    """The specification itself: a frozen -0.0 stays -0.0 through both moves, a one-coordinate block's factor is exactly 0."""
    from tests import prior_terms as pt
    T, W, D = 2, 12, 5
    spec = pt.make_spec([("uniform", -3.0, 3.0)] * D)
    loglike = lambda q: -0.5 * (q * q).sum(axis=1)      # noqa: E731
    rs = np.random.RandomState(1)
    x = rs.uniform(-1.0, 1.0, size=(T, W, D))
    x[..., 4] = -0.0
    P = pt.log_prior(spec, x.reshape(-1, D)).reshape(T, W)
    L = loglike(x.reshape(-1, D)).reshape(T, W)
    labels = np.tile(np.arange(W) % 2, (T, 1))
    x0 = x.copy()
    one, pair = np.array([0, 0, 1, 0, 0], dtype=bool), np.array([1, 1, 0, 0, 0], dtype=bool)
    out = gm.stretch_block_split(x, L, P, None, labels, 0, rs.randint(6, size=(T, 6)), rs.rand(T, 6), np.full((T, 6), 1e-300), 2.0, one, spec, loglike)
    assert np.all(out["factors"] == 0.0) and out["q"].shape == (T, 6, 1) and out["keep"].all()
    out = gm.mh_block(x, L, P, None, 0.01 * rs.randn(T, W, D), np.full((T, W), 1e-300), pair, spec, loglike)
    assert out["keep"].all() and np.array_equal(P, pt.log_prior(spec, x.reshape(-1, D)).reshape(T, W))
    assert np.array_equal(L, loglike(x.reshape(-1, D)).reshape(T, W)), "the likelihood saw the whole rows"
    assert np.array_equal(x[..., 4].view(np.uint64), x0[..., 4].view(np.uint64)) and np.signbit(x[..., 4]).all()
    assert np.array_equal(x[..., 3], x0[..., 3]) and (x[..., 2] != x0[..., 2]).any() and (x[..., 0] != x0[..., 0]).all()
    assert np.array_equal(x[:, 1::2, 2], x0[:, 1::2, 2]), "the other half did not move in the half-step"


# ---- the stand-alone program of the mask parser --------------------------------------------------------------------------------------------
def test_mask_parser_and_block_image_under_a_sanitizer_build(tmp_path):
    """tools/gibbs_host_check.cpp: a stand-alone program over csrc/hens_gibbs_host.h - every refusal of the mask parser, the accepted
    tables, the box as terms and a block's image byte for byte - built with -fsanitize=address,undefined and run on the CPU.  Where
    the compiler cannot link the sanitizers' runtimes the test is skipped with the linker's message: a plain build would say nothing
    about the parser's memory safety."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "gibbs_host_check.cpp"), str(tmp_path / "gibbs_host_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", str(probe), "-o", str(tmp_path / "probe")] + san, capture_output=True, text=True)
    if r.returncode != 0:                            # (an empty program: the runtimes themselves are missing)
        pytest.skip("no sanitizer runtimes for " + cxx + ": " + (r.stderr.strip().splitlines() or ["no message"])[-1])
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", src, "-o", exe] + san, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- the sizing of the GPU cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_gpu_cases_are_sized_on_the_specification(name):
    """What tests/test_hip_gibbs.py asserts as coverage, counted on the specification alone with the case's production draws: in
    every block and rung of both moves an accepted and a rejected proposal, a proposal outside the support, both moves in the
    mix, no knife edge; a coordinate in no block keeps its multiset."""
    c = gm.CASES[name]
    books, prob, x0, x = gm.free_run(c)
    gm.assert_coverage(books, name)
    assert books.num_proposals > 0 and books.num_proposals_mh > 0, f"{name}: one move of the mix never ran"
    assert books.num_proposals % len(c["stretch"]) == 0 and books.num_proposals_mh % len(c["mh"]) == 0
    assert books.num_proposals // len(c["stretch"]) + books.num_proposals_mh // len(c["mh"]) == c["iters"]
    if name in gm.NEVER_MOVES:
        d = gm.NEVER_MOVES[name]
        assert not any(m[d] for m in c["stretch"] + c["mh"])
        assert np.array_equal(np.sort(x0[..., d].reshape(-1).view(np.uint64)), np.sort(x[..., d].reshape(-1).view(np.uint64)))
