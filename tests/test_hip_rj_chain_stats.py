"""GPU tests of the diagnostics on a leaf-packing context's device chain (include/hipensemble.h: hens_rj_chain_leaves,
hens_rj_chain_leaf_moments, hens_rj_chain_moments; csrc/hens_rj_chain_stats.h: k_rj_chain_leaves, k_rj_chain_leaf_moments;
eryn_amd.backend.RJDeviceBackend: get_gelman_rubin_convergence_diagnostic, get_evidence_estimate, get_nleaves, get_nleaves_counts).

Chains come from RJEnsembleSampler(rng="philox", backend=RJDeviceBackend()) through the helpers of tests/test_hip_rj_chain_store.py.
One yardstick: eryn_amd/chain_stats.py over get_chain() / get_inds() of the same backend - the host copy the chain-store tests pin to
the host path.  Every device answer is compared with it bit for bit (counts exactly, NaN positions through np.isnan): no tolerance.
A chain is run once per case and shared by the tests; nothing below changes it.

Observed on an MI355X (the coverage conditions asserted below, counted from the host copy): see DESIGN 4.7."""
import numpy as np
import pytest

from eryn_amd import chain_stats
from tests.test_hip_rj_chain_store import WIDTH, case, make_sampler, names_of, start_state

pytestmark = pytest.mark.gpu

# the smallest shapes at which the kernels can still go wrong
CASES = {
    # 40 places: fewer than a wave; nl = 3: unaligned byte groups, nl = 4: the dword loads; nd = 3
    "odd_groups": case(("pulse", "sine"), (3, 4), nsteps=24),
    # every nd from 1 to 4; 66 places: the wave's tail and the rung boundary (place 33) inside a wave; 2 of 4 rungs stored
    "four_widths_W33": case(("offset", "ramp", "pulse", "burst"), (3, 2, 2, 2), W=33, rj="together", Ts=2, burn=10, thin=2, nsteps=12),
    # mask bit 31, 33 histogram bins: the largest LDS table.  A walker without an "offset" never reaches a stored step - its first
    # birth is always accepted (12 seeds tried) - so that branch keeps one leaf and the bins 0 and 32 are asked of "ramp"
    "slots64": case(("offset", "ramp"), (32, 32), (1, 0), rj="iterate_branches", nsteps=12),
    # one leaf per walker: the unprojected path; 120 series (16-byte lanes) and 99 (8-byte lanes, odd).  Under a birth / death move
    # the one leaf is born at once and never dies, so the chain with NaN in it is the one without such a move: masks from the
    # random start, moved by swaps
    "one_leaf_pulse": case(("pulse",), (1,), (0,), rj=None, burn=4, nsteps=12),
    "one_leaf_offset_W33": case(("offset",), (1,), (0,), T=3, W=33, burn=4, nsteps=12),
    # no birth / death move: the masks move only by swaps
    "no_rj_stretch": case(("pulse", "sine"), (3, 4), rj=None, move="stretch", thin=3, burn=2, nsteps=12),
}
PROJECTED = ("odd_groups", "four_widths_W33", "slots64")
# (ntemps, discard, thin) asked of the engine
SELECTIONS = {"odd_groups": [(1, 0, 1), (4, 0, 1), (1, 5, 3), (4, 5, 3)], "four_widths_W33": [(2, 0, 1), (1, 1, 2)], "slots64": [(4, 0, 1), (2, 2, 3)],
              "one_leaf_pulse": [(4, 0, 1), (1, 1, 3)], "one_leaf_offset_W33": [(3, 0, 1), (1, 1, 3)], "no_rj_stretch": [(4, 0, 3)]}
_RUNS = {}


def forced_start(c):
    """start_state with, on every rung and branch, walker 0 with as few leaves as the branch allows and walker 1 with every leaf in
    use (three of each where a branch has 32 slots: random masks never get there)."""
    st = start_state(c)
    for k, nl, nl_min in zip(names_of(c), c["nl_max"], c["nl_min"]):
        n = 3 if nl >= 32 else 1
        st.branches[k].inds[:, :n, nl_min:] = False
        st.branches[k].inds[:, n:2 * n] = True
    return st


def run(name, **kw):
    """The case's sampler behind its run, and the host copy of its chain."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        from eryn_amd.backend import RJDeviceBackend
        c = CASES[name]
        s = make_sampler(c, RJDeviceBackend(ntemps_store=c["Ts"], **kw))
        s.run_mcmc(forced_start(c), c["nsteps"], burn=c["burn"], thin_by=c["thin"])
        _RUNS[key] = s
    s = _RUNS[key]
    bk = s.backend
    return s, dict(x=bk.get_chain(), inds=bk.get_inds(), log_like=bk.get_log_like(), log_prior=bk.get_log_prior())


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    for s in _RUNS.values():
        s.engine.close()
    _RUNS.clear()


def same(a, b):
    """bit for bit, NaN where and only where the other has one"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def exact(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def kept(n, discard, thin):
    return discard, len(range(discard, n, thin)), thin


@pytest.mark.parametrize("name,sel", [(k, s) for k in sorted(SELECTIONS) for s in SELECTIONS[k]], ids=lambda v: v if isinstance(v, str) else "nt%d_d%d_t%d" % v)
def test_engine_calls_equal_the_module_bit_for_bit(name, sel):
    s, h = run(name)
    eng, c = s.engine, CASES[name]
    nt, discard, thin = sel
    first, count, thin = kept(c["nsteps"], discard, thin)
    steps = slice(first, None, thin)
    for k, kind in zip(names_of(c), c["kinds"]):
        x, inds = h["x"][k][steps, :nt], h["inds"][k][steps, :nt]
        assert x.shape == (count, nt, c["W"], inds.shape[3], WIDTH[kind])
        # leaf counts and the histogram
        want_n, want_h = chain_stats.leaf_counts(inds)
        got_n, got_h = eng.chain_leaves(k, first, count, thin, nt)
        assert exact(got_n, want_n) and exact(got_h, want_h), f"{name} {sel} {k}: chain_leaves"
        only_h = eng.chain_leaves(k, first, count, thin, nt, nleaves=False)
        assert only_h[0] is None and exact(only_h[1], want_h)
        # ordinal windows: one every walker fills (head and tail of its thirds), one some cannot, one nobody reaches
        totals = chain_stats.leaf_totals(want_h)
        low, top = int(totals.min()), int(totals.max())
        windows = [(0, max(low, 1)), (top // 3, top + 1), (top, top + 5)]
        r = chain_stats.third_split(c["W"], low)[2] if low else 0
        if r:
            windows += [(0, r), (low - r, low)]
        for lo, hi in windows:
            want = chain_stats.leaf_moments(x, inds, lo, hi)
            got = eng.chain_leaf_moments(k, first, count, thin, nt, lo, hi)
            for g, w, f in zip(got, want, ("sum", "m2", "n")):
                assert (exact if f == "n" else same)(g, w), f"{name} {sel} {k} window [{lo}, {hi}): {f} differs from chain_stats.leaf_moments"
            assert np.array_equal(got[2], np.clip(totals - lo, 0, hi - lo))
        # the chain as it lies (NaN of unused leaves propagates)
        got = eng.chain_moments(k, first, count, thin, nt)
        want = chain_stats.moments(x)
        for g, w, f in zip(got, want, ("sum", "m2", "n_finite")):
            assert same(g, w), f"{name} {sel} {k}: {f} differs from chain_stats.moments"
        assert np.array_equal(np.isnan(got[0]), np.broadcast_to(~inds.all(axis=0)[..., None], got[0].shape))
    for field in ("log_like", "log_prior"):
        got = eng.chain_moments(field, first, count, thin, nt)
        want = chain_stats.moments(h[field][steps, :nt], mask=True)
        for g, w, f in zip(got, want, ("sum", "m2", "n_finite")):
            assert same(g, w), f"{name} {sel}: {f} of {field} differs from chain_stats.moments"


def module_rhat(h, k, nd, steps, nt, per_walker):
    """Per rung what the module says of the host copy: Rhat, or the ValueError it raises."""
    out = {}
    for t in range(nt):
        try:
            out[t] = chain_stats.rj_psrf(h["x"][k][steps, t], h["inds"][k][steps, t], nd, per_walker, k, t)
        except ValueError as e:
            out[t] = str(e)
    return out


def assert_accessors_equal_the_module(bk, h, c, discard, thin, what, device=True):
    nt = bk.nstore
    steps = slice(discard, None, thin)
    for per_walker in (False, True):
        want = {k: module_rhat(h, k, WIDTH[kind], steps, nt, per_walker) for k, kind in zip(names_of(c), c["kinds"])}
        refusals = [v for k in want for v in want[k].values() if isinstance(v, str)]
        launches, downloads = bk.stats_launches, bk.downloads
        if refusals:                                       # (the first branch and rung the accessor meets that the module refuses)
            with pytest.raises(ValueError) as e:
                bk.get_gelman_rubin_convergence_diagnostic(discard=discard, thin=thin, doprint=False, per_walker=per_walker)
            assert str(e.value) in refusals, what
        else:
            got = bk.get_gelman_rubin_convergence_diagnostic(discard=discard, thin=thin, doprint=False, per_walker=per_walker)
            assert list(got) == names_of(c)
            for k in got:
                assert list(got[k]) == list(range(nt))
                for t in range(nt):
                    assert same(got[k][t], want[k][t]), f"{what} per_walker={per_walker}: Rhat of {k}, rung {t}: {got[k][t]} / {want[k][t]}"
        assert bk.downloads == downloads and (bk.stats_launches > launches) == device, what
    launches, downloads = bk.stats_launches, bk.downloads
    nle, counts = bk.get_nleaves(discard, thin, download=False), bk.get_nleaves_counts(discard, thin)
    for k in names_of(c):
        want = h["inds"][k][steps].sum(axis=-1, dtype=np.int64)
        nl = h["inds"][k].shape[-1]
        assert exact(nle[k], want), f"{what}: get_nleaves of {k}"
        assert exact(counts[k], np.array([np.bincount(want[:, t].ravel(), minlength=nl + 1) for t in range(nt)], dtype=np.int64)), f"{what}: counts of {k}"
    assert bk.downloads == downloads and (bk.stats_launches == launches + 2 * len(names_of(c))) == device, what


@pytest.mark.parametrize("name", sorted(CASES))
def test_accessors_on_the_device_chain_equal_the_module(name, capsys):
    s, h = run(name)
    bk, c = s.backend, CASES[name]
    assert bk._open == c["nsteps"] and bk.downloads == 1               # (the host copy above; the accessors below add none)
    for discard, thin in ((0, 1), (5, 3)):
        assert_accessors_equal_the_module(bk, h, c, discard, thin, f"{name} discard={discard} thin={thin}")
    assert capsys.readouterr().out == ""
    nt = bk.nstore
    for k, kind, nl, nl_min in zip(names_of(c), c["kinds"], c["nl_max"], c["nl_min"]):
        inds = h["inds"][k]
        totals = inds.sum(axis=(0, 3))                                 # [rung, walker]
        summed = bk.get_nleaves_counts()[k].sum(axis=0)
        print(f"{name} {k}: per-walker totals min {totals.min(axis=1)} max {totals.max(axis=1)}, summed histogram {summed.tolist()}")
        if name in PROJECTED:
            assert (totals.max(axis=1) - totals.min(axis=1) >= nl).all(), f"{name} {k}: per-walker totals hardly differ: {totals}"
            assert nl_min > 0 or (summed[0] > 0 and summed[nl] > 0), f"{name} {k}: bins 0 and {nl} of {summed}"
        if nl == 1:
            with np.errstate(all="ignore"):
                R = bk.get_gelman_rubin_convergence_diagnostic(doprint=False, per_walker=True)[k]
            unused = ~inds.all(axis=0)[..., 0]                         # [rung, walker]: a step without the leaf
            assert all(np.isnan(R[t]).all() == unused[t].any() for t in range(nt)), f"{name}: NaN where a walker's leaf was ever unused"
            if name == "one_leaf_pulse":
                assert unused.any() and not unused.any(axis=1).all(), f"{name}: rungs with NaN {unused.any(axis=1)}: both kinds must occur"
    if name == "slots64":
        assert all(v[..., 31].any() for v in h["inds"].values()), "mask bit 31 must be in use"
    if name == "no_rj_stretch":
        assert all((v.sum(axis=(1, 2, 3)) == v[0].sum()).all() for v in h["inds"].values()), "without a birth / death move the masks only move by swaps"
    for call in (bk.get_autocorr_time, bk.get_autocorr_thin_burn):
        with pytest.raises(ValueError, match="when using reversible jump"):
            call()


def test_both_remainders_of_the_third_split_are_met():
    """Over the file's projected cases: r != 0 in at least two (branch, rung) pairs and r = 0 in at least one."""
    seen = {}
    for name in PROJECTED:
        s, h = run(name)
        for k in names_of(CASES[name]):
            totals = h["inds"][k].sum(axis=(0, 3))
            for t in range(totals.shape[0]):
                M = int(totals[t].min())
                if (CASES[name]["W"] * M) // 3 >= 2:
                    seen[(name, k, t)] = (M, chain_stats.third_split(CASES[name]["W"], M)[2])
    print("(case, branch, rung): (M, r)", seen)
    assert sum(r != 0 for _, r in seen.values()) >= 2 and sum(r == 0 for _, r in seen.values()) >= 1, seen


def test_closed_segments_take_the_host_path_and_give_the_same_bits():
    """A run of 8 stored steps with room for 3: kept steps that reach into the closed segments run the module over the host copy,
    kept steps inside the open segment the kernels - and both equal the unsegmented backend's device path on the same chain."""
    from eryn_amd.backend import RJDeviceBackend
    c = dict(CASES["odd_groups"], nsteps=8)
    step_bytes = RJDeviceBackend.bytes_per_step(c["T"], c["W"], 21, 7)
    whole, seg = make_sampler(c, RJDeviceBackend()), make_sampler(c, RJDeviceBackend(max_bytes=3 * step_bytes + 5))
    for s in (whole, seg):
        s.run_mcmc(forced_start(c), 8, burn=c["burn"], thin_by=c["thin"])
    bw, bs = whole.backend, seg.backend
    assert bs.capacity == 3 and bs._open == 2 and bs.downloads == 2 and bw._open == 8 and bw.downloads == 0
    h = dict(x=bs.get_chain(), inds=bs.get_inds())
    assert bs.downloads == 3
    assert_accessors_equal_the_module(bs, h, c, 0, 1, "closed segments", device=False)
    assert_accessors_equal_the_module(bs, h, c, 2, 2, "closed segments", device=False)
    assert bs.stats_launches == 0
    assert_accessors_equal_the_module(bs, h, c, 6, 1, "the open segment of a segmented chain")
    assert bs.stats_launches > 0 and bs.downloads == 3
    for discard, thin in ((0, 1), (2, 2), (6, 1)):
        assert_accessors_equal_the_module(bw, h, c, discard, thin, "the same chain in one segment")
        a, b = (k.get_nleaves_counts(discard, thin) for k in (bw, bs))
        assert all(exact(a[k], b[k]) for k in a)
    assert bw.downloads == 0
    whole.engine.close(), seg.engine.close()


def test_protocol():
    from eryn_amd._lib import check
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    c = CASES["odd_groups"]
    s = make_sampler(c)
    eng = s.engine
    calls = (lambda: eng.chain_leaves("pulse", 0, 1), lambda: eng.chain_leaf_moments("pulse", 0, 1, 1, 1, 0, 1), lambda: eng.chain_moments("log_like", 0, 1))
    for call in calls:
        with pytest.raises(RuntimeError, match="no chain"):
            call()
    s.run_mcmc(start_state(c), 0)                        # (a state on the device)
    eng.chain_create(8, 3)
    for call in calls:                                   # an empty chain keeps nothing
        with pytest.raises(ValueError):
            call()
    eng.step_chain(6, 1)
    it0, ms0 = eng.iteration(), eng.chain_stats_ms()
    assert ms0 == dict(leaves_ms=-1.0, moments_ms=-1.0)
    bad = [dict(first=0, count=7), dict(first=-1, count=1), dict(first=6, count=1), dict(first=0, count=0), dict(first=0, count=-1), dict(first=0, count=4, thin=2),
           dict(first=0, count=1, thin=0), dict(first=0, count=1, ntemps=0), dict(first=0, count=1, ntemps=4), dict(first=0, count=2, thin=2**62)]
    for kw in bad:
        with pytest.raises(ValueError, match="kept steps"):
            eng.chain_leaves("sine", **kw)
        with pytest.raises(ValueError, match="kept steps"):
            eng.chain_leaf_moments("sine", kw["first"], kw["count"], kw.get("thin", 1), kw.get("ntemps", 3), 0, 5)
        with pytest.raises(ValueError, match="kept steps"):
            eng.chain_moments("sine", **kw)
        with pytest.raises(ValueError, match="kept steps"):
            eng.chain_moments("log_prior", **kw)
    with pytest.raises(ValueError, match="count <= 2\\^31"):       # (a u32 histogram bin cannot wrap)
        check(eng.lib.hens_rj_chain_leaves(eng.ctx, 0, 0, 2**31 + 1, 1, 1, None, None), eng.ctx)
    for branch in (2, -1, 7):
        with pytest.raises(ValueError, match=f"branch {branch} in"):
            eng.chain_leaves(branch, 0, 6)
        with pytest.raises(ValueError, match=f"branch {branch} in"):
            eng.chain_leaf_moments(branch, 0, 6, 1, 3, 0, 5)
        with pytest.raises(ValueError, match=f"branch {branch} in"):
            check(eng.lib.hens_rj_chain_moments(eng.ctx, 0, branch, 0, 6, 1, 3, None, None, None), eng.ctx)
    check(eng.lib.hens_rj_chain_moments(eng.ctx, 1, 7, 0, 6, 1, 3, None, None, None), eng.ctx)      # (logl: the branch is not read)
    for field in (-1, 3):
        with pytest.raises(ValueError, match=f"field {field} in"):
            check(eng.lib.hens_rj_chain_moments(eng.ctx, field, 0, 0, 6, 1, 3, None, None, None), eng.ctx)
    for lo, hi in ((0, 0), (5, 5), (6, 5), (-1, 5)):
        with pytest.raises(ValueError, match=rf"\[{lo}, {hi}\)"):
            eng.chain_leaf_moments("pulse", 0, 6, 1, 3, lo, hi)
    # every output may be null: the checks run, nothing is launched
    check(eng.lib.hens_rj_chain_leaves(eng.ctx, 0, 0, 6, 1, 3, None, None), eng.ctx)
    check(eng.lib.hens_rj_chain_leaf_moments(eng.ctx, 1, 0, 6, 1, 3, 0, 5, None, None, None), eng.ctx)
    assert eng.chain_stats_ms() == ms0, "a refused or empty call launched something"
    nle, hist = eng.chain_leaves("sine", 1, 3, 2)
    assert nle.shape == (3, 3, 10) and hist.shape == (3, 10, 5) and (hist.sum(axis=-1) == 3).all()
    ms = eng.chain_stats_ms()
    assert ms["leaves_ms"] > 0 and ms["moments_ms"] == -1.0
    assert eng.chain_leaf_moments("sine", 0, 6, 1, 3, 0, 2**62)[2].max() <= 24
    assert eng.chain_stats_ms()["moments_ms"] > 0
    assert eng.chain_moments("log_like", 0, 6)[2].shape == (3, 10) and eng.chain_stats_ms()["moments_ms"] > 0 and eng.iteration() == it0
    # the fixed-dimension family's calls stay closed to this context, with the text they had ...
    for call in (lambda: eng.lib.hens_chain_moments(eng.ctx, 0, 0, 1, 1, 1, None, None, None), lambda: eng.lib.hens_chain_act(eng.ctx, 0, 1, 1, 1, 50, None, None, None)):
        with pytest.raises(NotImplementedError, match="not built for a leaf-packing context"):
            check(call(), eng.ctx)
    eng.close()
    # ... and a fixed-dimension context refuses these
    flat = HipEnsemble(2, 16, 4, GaussianLikelihood(np.zeros(4), np.eye(4)), -5.0, 5.0, tempered=True)
    for call in (lambda: flat.lib.hens_rj_chain_leaves(flat.ctx, 0, 0, 1, 1, 1, None, None), lambda: flat.lib.hens_rj_chain_leaf_moments(flat.ctx, 0, 0, 1, 1, 1, 0, 1, None, None, None),
                 lambda: flat.lib.hens_rj_chain_moments(flat.ctx, 1, 0, 0, 1, 1, 1, None, None, None), lambda: flat.lib.hens_rj_chain_stats_ms(flat.ctx, None, None)):
        with pytest.raises(NotImplementedError, match="leaf-packing context"):
            check(call(), flat.ctx)
    flat.close()


def test_evidence_on_a_ladder_that_stands(monkeypatch):
    """stop_adaptation: from then on the ladder stands, and get_evidence_estimate is the module over get_log_like(), bit for bit."""
    import eryn_amd.rj as rj
    from eryn_amd.backend import RJDeviceBackend
    real = rj.RJEnsembleSampler
    monkeypatch.setattr(rj, "RJEnsembleSampler", lambda *a, tempering_kwargs=None, **kw: real(*a, tempering_kwargs=dict(tempering_kwargs, stop_adaptation=6), **kw))
    c = case(("pulse", "sine"), (3, 4), burn=2, nsteps=14)
    s = make_sampler(c, RJDeviceBackend())
    s.run_mcmc(start_state(c), c["nsteps"], burn=c["burn"])
    bk = s.backend
    with pytest.raises(ValueError, match="betas are allowed to vary"):
        bk.get_evidence_estimate()
    launches = bk.stats_launches
    got = bk.get_evidence_estimate(discard=6, thin=2)
    assert bk.stats_launches == launches + 1 and bk.downloads == 0
    L, betas = bk.get_log_like(discard=6, thin=2), bk.get_betas(discard=6, thin=2)
    assert (betas == betas[0]).all() and not np.array_equal(bk.get_betas()[0], betas[0])
    sm, _, nf = chain_stats.moments(L, mask=True)
    want = chain_stats.thermodynamic_integration_log_evidence(betas[0], chain_stats.rung_means(sm, nf))
    assert got == want and np.isfinite(got).all() and bk.get_evidence_estimate(discard=6, thin=2, return_error=False, method="TI") == want[0]
    few = make_sampler(c, RJDeviceBackend(ntemps_store=2))
    few.run_mcmc(start_state(c), 3)
    with pytest.raises(ValueError, match="every rung"):
        few.backend.get_evidence_estimate()
    s.engine.close(), few.engine.close()
