"""The red / blue stretch move as the in-model move of hens_rj_step (-m gpu): device draws against their NumPy specification
(tests/production_draws_rj.py), the production chain replayed through the pinned oracle (OracleRJSampler(in_model="stretch") with
only its draw sources replaced), production against the teacher-forced path, resume, folded adaptation, the walker guard and the
sampler.  Bars are DESIGN section 2's, as in tests/test_hip_rj.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tolerance_log as tol
from tests.production_draws_rj import stretch_draws
from tests.test_hip_rj import RTOL_L, _replay_oracle_class, knife

pytestmark = pytest.mark.gpu
NAMES = ["gauss", "sine"]
BOXES = {"gauss": [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], "sine": [(0.5, 1.5), (1.0, 20.0), (0.0, 2 * np.pi)]}
KINDS = {"gauss": "pulse", "sine": "sine"}


def _model(T, W, nl_max, nl_min, ndata, seed, start_leaves, start=None):
    """The model and starting state of tests/test_hip_rj.py's _replay_rj; ``start``: dict(t, y, sigma, x, inds, betas) - data, state and
    ladder made elsewhere (tests/limit_records.py) in their place."""
    from eryn_amd.moves.tempering import make_ladder
    from eryn_amd.rj import TemplateBranch
    rs = np.random.RandomState(seed)
    t = np.linspace(-1, 1, ndata)
    gauss_inj = np.array([[3.3, -0.2, 0.1], [2.6, -0.1, 0.1], [3.4, 0.0, 0.1], [2.9, 0.3, 0.1]])
    sine_inj = np.array([[1.3, 10.1, 1.0], [0.8, 4.6, 1.2]])
    sigma = 2.0
    y = sum(a * np.exp(-((t - b) ** 2) / (2 * c ** 2)) for a, b, c in gauss_inj) + \
        sum(a * np.sin(2 * np.pi * b * t + c) for a, b, c in sine_inj) + sigma * rs.randn(ndata)
    brs = [TemplateBranch(k, KINDS[k], BOXES[k], nl_max[i], nl_min[i]) for i, k in enumerate(NAMES)]
    x = {k: np.zeros((T, W, nl_max[i], 3)) for i, k in enumerate(NAMES)}
    inds = {k: np.zeros((T, W, nl_max[i]), dtype=bool) for i, k in enumerate(NAMES)}
    inj = {"gauss": gauss_inj, "sine": sine_inj}
    for i, k in enumerate(NAMES):
        for n in range(min(start_leaves[i], nl_max[i])):
            x[k][:, :, n] = inj[k][n % len(inj[k])] + 1e-2 * rs.randn(T, W, 3) * [1, 1, 0.1 if k == "gauss" else 1]
            inds[k][:, :, n] = True
    if start is not None:
        assert all(start["x"][k].shape == x[k].shape for k in NAMES)
        return brs, start["t"], start["y"], start["sigma"], start["x"], start["inds"], np.array(start["betas"], dtype=np.float64)
    return brs, t, y, sigma, x, inds, make_ladder(3 * sum(start_leaves), ntemps=T)


def _oracle_branches(nl_max, nl_min):
    from oracle import eryn_oracle_rj as orj
    okind = {"pulse": orj.KIND_PULSE, "sine": orj.KIND_SINE}
    return [orj.Branch(k, okind[KINDS[k]], BOXES[k], nl_max[i], nl_min[i]) for i, k in enumerate(NAMES)]


def _engine(T, W, nl_max, nl_min, ndata, seed, start_leaves, schedule, betas=None, **kw):
    from eryn_amd.rj import RJEngine
    brs, t, y, sigma, x, inds, betas0 = _model(T, W, nl_max, nl_min, ndata, seed, start_leaves)
    if betas is not None:                                         # (a ladder of the caller's in place of the geometric one)
        betas0 = np.array(betas, dtype=np.float64)
    eng = RJEngine(T, W, brs, t, y, sigma, seed=seed, **kw)
    eng.upload(x, inds, betas=betas0)
    eng.eval_state()
    eng.set_in_model("stretch")
    eng.set_schedule(schedule)
    return eng, brs, t, y, sigma, betas0


def _replay_stretch_class():
    class ReplayStretch(_replay_oracle_class()):
        """The production replay class of tests/test_hip_rj.py plus the stretch move's four draw sources, read from what
        hens_rj_debug_draws_stretch exports; the structure the reference guarantees is asserted on the way."""

        def load(self, d, offsets, ds=None):
            super().load(d, offsets)
            self.ds = ds

        def _draw_split_labels(self):
            lab = self.ds["labels"].astype(np.int64)
            assert lab.shape == (self.T, self.W) and set(np.unique(lab)) <= {0, 1}
            for k in range(2):                                   # arange(W) % 2 shuffled: ceil((W - k) / 2) walkers of set k
                assert np.all((lab == k).sum(axis=1) == (self.W - k + 1) // 2)
            return lab

        def _draw_rint(self, bi, split, Ns, Nc):
            r = self.ds["rint"][split][bi]
            assert r.shape == (self.T, Ns) and r.min() >= 0 and r.max() < Nc
            return r

        def _draw_zz(self, split, Ns):
            u = self.ds["u_zz"][split]                           # one per moving walker
            assert u.shape == (self.T, Ns) and np.all((u >= 0) & (u < 1))
            return u

        def _draw_accept_split(self, split, Ns):
            u = self.ds["u_acc"][split]
            assert u.shape == (self.T, Ns) and np.all((u >= 0) & (u < 1))
            return u

    return ReplayStretch


# ---- 1. device draws = specification ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,W", [(3, 25), (2, 26), (2, 64)])
@pytest.mark.parametrize("nbranches", [2, 1])
def test_device_stretch_draws_are_the_specification(T, W, nbranches):
    from eryn_amd.rj import RJEngine, TemplateBranch
    t = np.linspace(-1, 1, 20)
    brs = [TemplateBranch(k, KINDS[k], BOXES[k], 2, 0) for k in NAMES[:nbranches]]
    seed = 0x5EED_0000_0000 + 977 * W + nbranches
    eng = RJEngine(T, W, brs, t, np.zeros(20), 1.0, seed=seed)
    eng.set_in_model("stretch")
    for schedule in ("separate_branches", "none"):               # (the in-model draws do not depend on the schedule)
        eng.set_schedule(schedule)
        for it in (0, 1, 63, 64):
            d, s = eng.debug_draws_stretch(it), stretch_draws(seed, it, T, W, nbranches)
            assert np.array_equal(d["labels"], s["labels"]), f"labels, iteration {it}"
            for h in range(2):
                assert np.array_equal(d["rint"][h], s["rint"][h]), f"rint of half {h}, iteration {it}"
                assert np.array_equal(d["u_zz"][h], s["u_zz"][h]), f"u_zz of half {h}, iteration {it}"
                assert np.array_equal(d["u_acc"][h], s["u_acc"][h]), f"u_acc of half {h}, iteration {it}"
    g = eng.debug_draws(5)                                        # a stretch context asks for no scale: zeros where the Gaussian step was
    assert not g["step"].any() and not g["u_mh"].any() and np.all((g["u_bd"] > 0) & (g["u_bd"] < 1))
    eng.close()


# ---- 2. production replay through the oracle -----------------------------------------------------------------------------------
def _replay_stretch(T, W, nl_max, nl_min, ndata, schedule, iters, seed, start_leaves, downloads=True, betas=None, lag=None, nu=None):
    """``betas``: the ladder to upload in place of the geometric one; ``lag`` / ``nu``: the adaptation's constants for the context and
    the oracle alike; the oracle returned carries the ladder uploaded and the one downloaded last (betas_uploaded, betas_device), the
    accepted proposals per rung (accepted_rung) and the accepted swaps per pair over its cascades (swaps_sum, cascades)."""
    from oracle import eryn_oracle_rj as orj
    adapt = {k: v for k, v in (("adaptation_lag", lag), ("adaptation_time", nu)) if v is not None}
    eng, brs, t, y, sigma, betas0 = _engine(T, W, nl_max, nl_min, ndata, seed, start_leaves, schedule, betas=betas, **adapt)
    x0, inds0, L0, P0, _ = eng.download()
    obr = _oracle_branches(nl_max, nl_min)
    o = _replay_stretch_class()(obr, x0, inds0, t, y, sigma, None, None, betas0, schedule=schedule, in_model="stretch", record=True,
                                **adapt)
    o.betas_uploaded = betas0.copy()
    assert np.array_equal(o.st.P, P0)
    tol.check_logl(L0, o.st.L, RTOL_L, "template log-like")
    offsets = {b.name: eng.off[i] for i, b in enumerate(brs)}
    rj = schedule != "none"
    mh_acc, bd_acc, done = np.zeros((T, W)), np.zeros((T, W)), 0
    half_acc, half_n, ninf, bd_n = [0, 0], [0, 0], 0, 0
    calls = (iters // 2, iters - iters // 2)
    for n in calls:
        it0 = eng.iteration()
        eng.step(n)
        eng.synchronize()
        for it in range(it0, it0 + n):
            o.load(eng.debug_draws(it), offsets, eng.debug_draws_stretch(it))
            acc, bi, racc = o.iteration()
            rec = o.trace.pop()
            mh_acc += acc
            for h in range(2):                                   # coverage, counted from the ORACLE's proposals
                assert not knife(rec[f"st_lnpdiff{h}"], rec[f"st_u_acc{h}"]).any(), "knife-edge accept test"
                half_acc[h] += int(rec[f"st_keep{h}"].sum())
                half_n[h] += rec[f"st_keep{h}"].size
                ninf += int(np.isinf(rec[f"st_logp{h}"]).sum())
            if rj:
                for sub in rec.get("rj_sub", [rec]):
                    assert not knife(sub["rj_lnpdiff"], sub["rj_u_acc"]).any(), "knife-edge accept test (birth / death)"
                bd_acc += racc
                bd_n += racc.size
        done += n
        what = f"hens_rj_step (stretch, {schedule}) vs oracle after {done} iterations"
        if not downloads:
            xr, indr, Lr = eng.debug_resident()
            for k in NAMES:
                assert np.array_equal(indr[k], o.st.inds[k]) and np.array_equal(xr[k], o.st.x[k]), f"{what} (resident): {k}"
            tol.check_logl(Lr, o.st.L, RTOL_L, f"{what}: resident log-likelihood vs the oracle")
            if done < iters:
                continue
        x1, inds1, L1, P1, betas1 = eng.download()
        for k in NAMES:
            assert np.array_equal(inds1[k], o.st.inds[k]), f"{what}: leaf masks of {k}"
            assert np.array_equal(x1[k], o.st.x[k]), f"{what}: coordinates of {k} (dead slots included)"
        assert np.array_equal(P1, o.st.P), f"{what}: log-prior"
        tol.check_logl(L1, o.st.L, RTOL_L, what)
        np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
        o.betas_device = betas1
        c = eng.counters()
        assert np.array_equal(c["accepted_mh"], mh_acc) and np.array_equal(c["accepted_bd"], bd_acc), f"{what}: accept counters"
        assert c["num_mh"] == done and c["num_bd"] == (done if rj else 0)
        assert np.array_equal(c["swaps_last"], o.swaps_accepted), f"{what}: swap counts of the last cascade"
    eng.close()
    share = sum(half_acc) / sum(half_n)
    print(f"stretch accept share {share:.3f}, per half {half_acc} of {half_n}, -inf prior share {ninf / sum(half_n):.3f}, "
          f"birth/death accepted {int(bd_acc.sum())} of {bd_n}")
    assert 0.15 <= share <= 0.85, f"accept share {share}"
    for h in range(2):
        assert 0 < half_acc[h] < half_n[h], f"half {h} must have accepted and rejected proposals"
    assert ninf > 0, "at least one proposal must have a -inf prior"
    if rj:
        assert 0 < bd_acc.sum() < bd_n, "both outcomes of the birth / death move must occur"
    else:
        assert np.array_equal(o.st.inds["gauss"], inds0["gauss"]) and np.array_equal(o.st.inds["sine"], inds0["sine"])
    o.accepted_rung = (mh_acc + bd_acc).sum(axis=1)
    return o


CASES = [  # T, W, nleaves_max, nleaves_min, ndata, schedule, iterations, start_leaves, downloads
    (3, 26, (2, 2), (0, 0), 60, "separate_branches", 8, (2, 1), True),
    (3, 26, (2, 2), (0, 0), 60, "separate_branches", 8, (2, 1), False),         # read through hens_rj_debug_resident
    (3, 25, (2, 2), (0, 1), 60, "separate_branches", 8, (2, 1), True),          # odd W: halves of 13 and 12
    (2, 44, (3, 4), (0, 0), 60, "iterate_branches", 8, (2, 2), True),
    (2, 44, (3, 4), (0, 0), 130, "together", 8, (2, 2), True),                  # uniform-grid likelihood
    (2, 44, (3, 4), (0, 0), 130, "none", 8, (2, 2), True),
    (2, 64, (2, 2), (0, 0), 60, "separate_branches", 8, (2, 1), True),
    (2, 144, (12, 12), (0, 0), 130, "separate_branches", 4, (2, 2), True),      # 72 coordinates: second pass of the per-coordinate loops
]


@pytest.mark.parametrize("T,W,nl_max,nl_min,ndata,schedule,iters,start_leaves,downloads", CASES)
def test_stretch_production_step_replayed_through_the_oracle(T, W, nl_max, nl_min, ndata, schedule, iters, start_leaves, downloads):
    """hens_rj_step with the stretch move: split, complements per branch, stretch factor, accept uniforms, the two half launches,
    cascade + adaptation, then the birth / death move of the schedule - every iteration's exported draws go through the pinned
    oracle, which must land on the device's state: coordinates (dead slots included), leaf masks, log-prior, accept counters and
    swap counts exactly, log-likelihood to RTOL_L, betas to 1e-13, no knife-edge accept test."""
    _replay_stretch(T, W, nl_max, nl_min, ndata, schedule, iters, seed=23, start_leaves=start_leaves, downloads=downloads)


# ---- 3. production = teacher-forced ----------------------------------------------------------------------------------------------
def test_stretch_production_step_is_the_teacher_forced_chain():
    """The exported draws of four iterations fed to a second context through hens_rj_stretch_split / hens_pt_sweep / hens_rj_bd_step:
    coordinates, masks, log-prior and accept masks identical, log-likelihood to RTOL_L."""
    T, W, nl_max, nl_min, seed = 3, 26, (2, 2), (0, 0), 29
    a, brs, t, y, sigma, betas0 = _engine(T, W, nl_max, nl_min, 60, seed, (2, 1), "separate_branches")
    b, *_ = _engine(T, W, nl_max, nl_min, 60, seed, (2, 1), "separate_branches")
    n_acc = 0
    for it in range(4):
        xa, ia, La, Pa, ba = a.download()
        acc0 = a.counters()["accepted_mh"].copy()
        bd0 = a.counters()["accepted_bd"].copy()
        at = a.counters()["adapt_time"]
        a.step(1)
        d, ds = a.debug_draws(it), a.debug_draws_stretch(it)
        # the in-model move, teacher-forced from the state the production step started from
        b.upload(xa, ia, La, Pa, ba)
        b.set_adapt_time(at)
        keep_w = np.zeros((T, W), dtype=bool)
        for h in range(2):
            keep = b.stretch_split(h, ds["labels"], ds["rint"][h], ds["u_zz"][h], ds["u_acc"][h])
            for tt in range(T):
                keep_w[tt, np.flatnonzero(ds["labels"][tt] == h)] = keep[tt]
        # cascade with adaptation: hens_pt_sweep takes the reference's form (iperm, i1perm per pair) of the column maps
        slot = d["slot_mh"].astype(np.int64)
        iperm = np.stack([slot[T - 1 - j] for j in range(T - 1)])
        i1perm = np.stack([slot[T - 2 - j] for j in range(T - 1)])
        b.pt_sweep(iperm, i1perm, d["uswap_mh"], adapt=True)
        # birth / death on the drawn branch with the exported coin / selector / birth draws
        xb, ib, Lb, Pb, bb = b.download()
        br = d["branch"]
        name = NAMES[br]
        nleaves = ib[name].sum(axis=-1)
        change = d["coin"][0].astype(np.int64)
        change = np.where(nleaves == nl_min[br], +1, np.where(nleaves == nl_max[br], -1, change))
        leaf = np.zeros((T, W), dtype=np.int64)
        for tt in range(T):
            for w in range(W):
                cand = np.flatnonzero(~ib[name][tt, w]) if change[tt, w] > 0 else np.flatnonzero(ib[name][tt, w])
                leaf[tt, w] = cand[(int(d["sel"][0][tt, w]) * len(cand)) >> 32]
        keep_bd = b.bd_step(br, change, leaf, d["birth"][0], d["u_bd"][0])
        slot = d["slot_bd"].astype(np.int64)
        b.pt_sweep(np.stack([slot[T - 1 - j] for j in range(T - 1)]), np.stack([slot[T - 2 - j] for j in range(T - 1)]),
                   d["uswap_bd"], adapt=False)
        x1, i1, L1, P1, b1 = a.download()
        x2, i2, L2, P2, b2 = b.download()
        what = f"production vs teacher-forced, iteration {it}"
        for k in NAMES:
            assert np.array_equal(i1[k], i2[k]), f"{what}: leaf masks of {k}"
            assert np.array_equal(x1[k], x2[k]), f"{what}: coordinates of {k}"
        assert np.array_equal(P1, P2), f"{what}: log-prior"
        tol.check_logl(L1, L2, RTOL_L, what)
        c = a.counters()
        assert np.array_equal(c["accepted_mh"] - acc0, keep_w), f"{what}: accept mask of the stretch move"
        assert np.array_equal(c["accepted_bd"] - bd0, keep_bd), f"{what}: accept mask of the birth / death move"
        n_acc += int(keep_w.sum())
    assert n_acc > 0
    a.close()
    b.close()


# ---- 4. resume ------------------------------------------------------------------------------------------------------------------
def test_stretch_chain_resumed_in_a_new_context_is_the_uninterrupted_chain():
    T, W, nl_max, nl_min, seed = 3, 26, (2, 2), (0, 0), 31
    a, *_ = _engine(T, W, nl_max, nl_min, 60, seed, (2, 1), "separate_branches")
    a.step(3)
    (x1, i1, L1, P1, b1), it1, at1 = a.download(), a.iteration(), a.counters()["adapt_time"]
    a.step(3)
    xa, ia, La, Pa, ba = a.download()
    ita = a.iteration()
    a.close()
    b, *_ = _engine(T, W, nl_max, nl_min, 60, seed, (2, 1), "separate_branches")
    b.upload(x1, i1, L1, P1, b1)
    b.set_iteration(it1)
    b.set_adapt_time(at1)
    b.step(3)
    xb, ib, Lb, Pb, bb = b.download()
    assert b.iteration() == ita == 6
    for k in NAMES:
        assert np.array_equal(ia[k], ib[k]) and np.array_equal(xa[k], xb[k]), f"{k} differs in the resumed chain"
    assert np.array_equal(La, Lb) and np.array_equal(Pa, Pb) and np.array_equal(ba, bb)
    assert not np.array_equal(xa["gauss"], x1["gauss"]), "the chain must have moved"
    b.close()


# ---- 5. adaptation folded into the first half launch vs a launch of its own ---------------------------------------------------
_FOLD_WORKER = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests.test_hip_rj_stretch import _engine
eng, *_ = _engine(4, 64, (2, 2), (0, 0), 130, 37, (2, 1), "separate_branches", adaptation_lag=20, adaptation_time=5)
for n in (1, 40, 30):                         # (crosses iteration % 64 == 63)
    eng.step(n)
eng.synchronize()
x1, inds1, L1, P1, betas1 = eng.download()
c = eng.counters()
np.savez(sys.argv[2], xg=x1["gauss"], xs=x1["sine"], ig=inds1["gauss"], js=inds1["sine"], L=L1, P=P1, betas=betas1,
         acc_mh=c["accepted_mh"], acc_bd=c["accepted_bd"], swaps_total=c["swaps_total"], swaps_last=c["swaps_last"])
eng.close()
"""


def test_stretch_adaptation_folded_into_the_next_launch_changes_nothing(tmp_path):
    """The ladder adaptation pending from the previous cascade rides in the stretch move's first half launch; HENS_NO_FOLD=1 keeps
    k_adapt as a launch of its own: the same chain in every bit."""
    from eryn_amd.moves.tempering import make_ladder
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for env in ({}, {"HENS_NO_FOLD": "1"}):
        out = str(tmp_path / f"{len(outs)}.npz")
        e = dict(os.environ, **env)
        if not env:
            e.pop("HENS_NO_FOLD", None)
        r = subprocess.run([sys.executable, "-c", _FOLD_WORKER, root, out], env=e, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(dict(np.load(out)))
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), f"folded adaptation vs k_adapt: `{k}` differs"
    assert outs[0]["acc_mh"].sum() > 0 and outs[0]["acc_bd"].sum() > 0 and outs[0]["swaps_total"].sum() > 0
    assert not np.array_equal(outs[0]["betas"], make_ladder(9, ntemps=4)), "the ladder must have moved"


# ---- 6. guard ----------------------------------------------------------------------------------------------------------------------
def test_stretch_step_refuses_too_few_walkers_before_it_launches():
    """red_blue.py:103-114 counts every leaf slot of every branch: 15 coordinates need 30 walkers."""
    from eryn_amd.rj import RJEngine, TemplateBranch
    t = np.linspace(-1, 1, 20)
    brs = [TemplateBranch("gauss", "pulse", BOXES["gauss"], 3, 0), TemplateBranch("sine", "sine", BOXES["sine"], 2, 0)]
    T, W = 2, 16
    x = {"gauss": np.zeros((T, W, 3, 3)), "sine": np.zeros((T, W, 2, 3))}
    inds = {"gauss": np.zeros((T, W, 3), dtype=bool), "sine": np.zeros((T, W, 2), dtype=bool)}
    x["gauss"][:, :, 0] = [3.0, 0.0, 0.1]
    inds["gauss"][:, :, 0] = True
    for dangerous in (False, True):
        eng = RJEngine(T, W, brs, t, np.zeros(20), 1.0, live_dangerously=dangerous)
        eng.upload(x, inds, betas=np.array([1.0, 0.5]))
        eng.eval_state()
        eng.set_in_model("stretch")
        if dangerous:
            eng.step(2)
            assert eng.iteration() == 2 and eng.counters()["num_mh"] == 2
        else:
            with pytest.raises(RuntimeError, match="unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions"):
                eng.step(2)
            assert eng.iteration() == 0 and eng.counters()["num_mh"] == 0, "nothing may have been launched"
        eng.close()


# ---- 7. sampler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rj_moves", ["separate_branches", None])
def test_rj_sampler_philox_mode_with_the_stretch_move(rj_moves):
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import RJEnsembleSampler, StretchLeafMove, TemplateLikelihood
    from eryn_amd.state import State
    T, W, N = 4, 64, 100
    t = np.linspace(-1, 1, N)
    rs = np.random.RandomState(3)
    y = 3.0 * np.exp(-((t - 0.1) ** 2) / (2 * 0.1 ** 2)) + 1.0 * np.sin(2 * np.pi * 5.0 * t + 1.0) + 1.5 * rs.randn(N)
    priors = {"gauss": {0: uniform_dist(2.5, 3.5), 1: uniform_dist(-1, 1), 2: uniform_dist(0.01, 0.21)},
              "sine": {0: uniform_dist(0.5, 1.5), 1: uniform_dist(1.0, 20.0), 2: uniform_dist(0.0, 2 * np.pi)}}
    nl = {"gauss": 2, "sine": 2}                                  # 12 coordinates: 64 >= 24 walkers
    s = RJEnsembleSampler(W, {k: 3 for k in NAMES}, TemplateLikelihood(KINDS, t, y, 1.5), priors,
                          tempering_kwargs=dict(ntemps=T), branch_names=NAMES, nleaves_max=nl,
                          nleaves_min=(dict(nl) if rj_moves is None else None), moves=StretchLeafMove(), rj_moves=rj_moves,
                          rng="philox", seed=8)
    coords = {k: np.zeros((T, W, 2, 3)) for k in NAMES}
    inds = {k: np.zeros((T, W, 2), dtype=bool) for k in NAMES}
    nstart = 2 if rj_moves is None else 1
    for n in range(nstart):
        coords["gauss"][:, :, n] = [3.0, 0.1 + 0.3 * n, 0.1] + 1e-2 * rs.randn(T, W, 3) * [1, 1, 0.1]
        coords["sine"][:, :, n] = [1.0, 5.0 + 2.0 * n, 1.0] + 1e-2 * rs.randn(T, W, 3)
        inds["gauss"][:, :, n] = inds["sine"][:, :, n] = True
    last = s.run_mcmc(State(coords, inds=inds), 10, burn=3, thin_by=2, store=True)
    assert len(s.chain) == 10 and s.iteration == 13
    assert s.engine.iteration() == 23 and s.moves[0].num_proposals == 23
    assert np.isfinite(last.log_like).all() and all(np.isfinite(c.log_like).all() for c in s.chain)
    assert s.moves[0].accepted.sum() > 0
    if rj_moves is None:
        assert s.rj_accepted == [] and s.rj_num_proposals_all == 0
        for c in s.chain:
            for k in NAMES:
                assert np.array_equal(c.branches[k].inds, inds[k]), "without an RJ move the leaf masks never change"
    else:
        assert s.rj_num_proposals_all == 23 and s.rj_accepted_all.sum() > 0
    s.engine.close()
