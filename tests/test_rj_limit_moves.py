"""The cases of tests/rj_limit_moves.py sized on the specifications alone (no GPU): every case of tests/test_hip_rj_limit_moves.py
meets its coverage conditions with no decision on a knife edge, over more proposals than the GPU file feeds the device - so the GPU
tests need no exemption and leave no case out."""
import numpy as np
import pytest

from tests import limit_records as lr
from tests import rj_limit_moves as rl
from tests import rj_mt_move as rm


# ---- A: the multiple-try birth / death move ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rl.MT_CASES))
def test_mt_cases_cover_every_edge_on_the_specification_alone(name):
    """MT_ROUNDS_CPU rounds of the case's stream (the GPU file runs the first MT_ROUNDS): on every pair of edges(model) an accepted
    birth into the slot, an accepted death of it, a birth landing at nleaves_max and a pick other than try 0, a forced death from every
    full 32-leaf branch - after MT_ROUNDS_SPARE rounds already -, no pick or accept decision on a knife edge in any round, and the
    specification's own float64 sums within their bounds of exact arithmetic."""
    c = rl.mt_case(name)
    p = rl.mt_problem(c)
    edges = rl.mt_pairs(c)
    nl = lr.MODELS[c["model"]]["nl_max"]
    assert [b.nleaves_max for b in p["obr"]] == list(nl) and c["K"] <= rm.MAX_TRY
    # the starts hold what the kernel's edges need: a full 32-leaf branch (candidates 0xffffffff), all-but-the-slot walkers on every edge
    cls = {tuple(v) for v in p["classes"].reshape(-1)}
    for b, s in lr.edges(c["model"]):
        assert {("all_but", b, s), ("pair", b, s), ("full", b, s)} <= cls, (name, b, s)
    assert set(edges) - set(lr.edges(c["model"])) <= {(b, s) for k, b, s in cls if k == "all_but"}, "the terms case's extra pair has its all-but walkers"
    spare = {}

    def on_proposal(o, bi, inputs, info, ex, sweep, pre, mid):
        rm.mm.assert_sums(info["lsw"], info["aux_lsw"], info["factors"], ex, f"{name} (NumPy)")

    def on_round(done, cnt, cov):
        if done == rl.MT_ROUNDS_SPARE:
            spare["missing"] = cov.missing(edges)
            print(f"{name}: after {done} rounds: coverage {cov.line(edges)}")

    cnt, cov = rl.mt_forced_run(c, rl.MT_ROUNDS_CPU, on_proposal, p=p, on_round=on_round)
    assert spare["missing"] == [], f"{name}: edges without coverage after {rl.MT_ROUNDS_SPARE} rounds"
    rl.mt_assert_covered(cnt, cov, c, name)


def test_mt_terms_case_sums_31_and_32_slots_with_the_try_at_both_ends():
    """The prior-terms case: branches of 31 and 32 slots (numpy_sum_sub over n = 31: remainder 7, n = 32: none), births proposed into
    slot 0 and into the top slot of either branch from walkers with every other slot in use."""
    c = rl.mt_case("terms_31_32_k5")
    p = rl.mt_problem(c)
    assert [b.nleaves_max for b in p["obr"]] == [31, 32] and all(hasattr(b, "spec") for b in p["obr"])
    assert all(g is not None for g in p["gens"]) and np.isfinite(rl.orj.compute_log_prior(p["x"], p["inds"], p["obr"])).all()
    cls = {tuple(v) for v in p["classes"].reshape(-1)}
    assert {("all_but", 0, 0), ("all_but", 1, 0), ("all_but", 1, 31), ("full", 1, 31)} <= cls
    tops = set()
    for tt in range(rl.T):
        for w in range(rl.W):
            for bi, b in enumerate(p["obr"]):
                m = p["inds"][b.name][tt, w]
                if m.sum() == b.nleaves_max - 1:
                    tops.add((bi, int(np.where(~m)[0][0])))
    assert {(0, 0), rl.TERMS_TOP, (1, 0), (1, 31)} <= tops, "a walker of 30 / 31 active leaves whose free slot is slot 0, and one whose free slot is the top one"


# ---- C: the group stretch move -----------------------------------------------------------------------------------------------------------
def group_chain(o, iters, on_record=None):
    """``iters`` iterations of a GroupOracle -> (knife-edge decisions of its moves and swaps, accepted group proposals, decisions)."""
    from tests.test_hip_leaf_kinds import _knife_accepts, knife
    knives = accepted = decisions = 0
    for _ in range(iters):
        o.iteration()
        rec = o.trace.pop()
        knives += int((knife(rec["lnpdiff"], rec["u_acc"]) & (rec["logl"] != o.fill)).sum()) + _knife_accepts(rec)
        accepted += int(rec["mh_accepted"].sum())
        decisions += rec["mh_accepted"].size
        if on_record is not None:
            on_record(rec)
    return knives + getattr(o, "knife_swaps", 0), accepted, decisions


def test_group_records_put_the_uniforms_on_both_sides_of_the_second_call():
    """62 | 63 | 64 slots: nslots + 1 < 64, == 64, > 64 - zz's uniform and the accept uniform in the first call's lanes 62 / 63, in lane
    63 and the second call's lane 0, in the second call's lanes 0 / 1."""
    assert [sum(r["nl_max"]) for r in rl.GROUP_RECORDS.values()] == [62, 63, 64]
    for name, r in rl.GROUP_RECORDS.items():
        p = rl.group_problem(name)
        assert [b.nleaves_max for b in p["obr"]] == list(r["nl_max"]) and all(p["x"][b.name].shape == (rl.T, rl.W, b.nleaves_max, b.ndim) for b in p["obr"])
    # the statement of the draws: distinct words per slot, zz and accept; a pick lies in [0, nf)
    picks, u_zz, u_acc = rl.group_draws(7, 3, 2, 5, (32, 16, 8, 8), (5, 0, 3, 1))
    assert [p.shape for p in picks] == [(2, 5, 32), (2, 5, 16), (2, 5, 8), (2, 5, 8)]
    assert picks[0].max() == 4 and not picks[1].any() and picks[2].max() == 2 and not picks[3].any()
    assert len(np.unique(np.concatenate([u_zz.ravel(), u_acc.ravel()]))) == 20 and ((u_zz >= 0) & (u_zz < 1)).all()


@pytest.mark.parametrize("name", sorted(rl.GROUP_RECORDS))
def test_group_record_cases_are_sized(name):
    """The teacher-forced chain of the GPU test on the specification alone (NumPy streams, every window held to check_window): no
    decision on a knife edge, both outcomes of the move, a rebuild and a newborn leaf's window."""
    from tests.test_hip_leaf_kinds import _counting
    from tests import rj_group_move as rgr
    p = rl.group_problem(name)
    o = rl.group_oracle(p, "separate_branches", rl.GROUP_RECORDS[name]["seed"], cls=_counting(rgr.GroupOracle))
    seen = dict(rebuilt=0, born=0)

    def on_record(rec):
        seen["rebuilt"] += bool(rec["rebuilt"])
        seen["born"] += 0 if rec["rebuilt"] else sum(int(v.sum()) for v in rec["born"].values())

    knives, accepted, decisions = group_chain(o, rl.GROUP_FORCED_ITERS + 1, on_record)
    print(f"{name}: accepted {accepted} of {decisions}, rebuilds {seen['rebuilt']}, newborn windows {seen['born']}; {knives} knife-edge")
    assert knives == 0 and 0 < accepted < decisions and seen["rebuilt"] >= 2 and seen["born"] > 0


@pytest.mark.parametrize("name", sorted(rl.TABLE_CASES))
def test_group_table_cases_reach_the_limits_they_are_there_for(name):
    """W = 300: two passes of the gather and tables of thousands of entries (a rank sort over many tiles); the one-branch tables: exactly
    255, 256 and 257 entries; with equal keys: one key across gather entry 256 (where there is one) and far from it, and -0.0 / +0.0 /
    -0.0 as ONE key whose rows keep their bits, in gather order.  One rebuild and two moves on the specification alone: no knife edge."""
    from tests import rj_group_move as rgr
    from tests.test_hip_leaf_kinds import _counting
    c = rl.TABLE_CASES[name]
    p = rl.table_problem(name)
    assert p["W"] == c["W"] > 256
    o = rl.group_oracle(p, "none", 1, iters_update=5, cls=_counting(rgr.GroupOracle))
    o.rebuild()
    sizes = {b.name: len(o.keys[b.name]) for b in p["obr"]}
    if "n" in c:
        assert sizes == {"pulse": c["n"]}
        keys, tab = o.keys["pulse"], o.tab["pulse"]
        assert np.array_equal(keys, np.sort(keys)) and (not c["ties"]) == bool(np.all(np.diff(keys) > 0))
        if c["ties"]:
            ws, ss = np.where(p["inds"]["pulse"][0])
            k = rl.GROUP_KEY["pulse"]
            gk = p["x"]["pulse"][0, ws, ss, k]                                   # keys in gather order
            run = gk == gk[rl.TIE_RUN[0]]
            assert run[list(rl.TIE_APART)].all() and run[rl.TIE_RUN[0]:min(rl.TIE_RUN[1], c["n"])].all()
            assert (c["n"] > 256) == bool(run[256:].any()), "the run reaches past gather entry 256 where the table has one"
            z = np.where(keys == 0.0)[0]
            assert len(z) == 3 and not np.signbit(keys[z]).any(), "-0.0 is keyed as +0.0"
            assert np.signbit(tab[z, k]).tolist() == [True, False, True], "the rows keep their bits, in gather order (the sort is stable)"
            # the stable order among the run: ascending gather index = ascending (walker, slot)
            rows = tab[keys == gk[rl.TIE_RUN[0]]]
            want = p["x"]["pulse"][0, ws[run], ss[run]]
            assert np.array_equal(rows, want)
    else:
        assert min(sizes.values()) > 16 * 256, sizes
    knives, accepted, decisions = group_chain(o, 2)
    print(f"{name}: table entries {sizes}; accepted {accepted} of {decisions}; {knives} knife-edge")
    assert knives == 0 and 0 < accepted < decisions


# ---- A, production: hens_rj_step under the multiple-try move on the limit records ----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rl.MT_REPLAYS))
def test_mt_replays_are_sized(name):
    """The free-running chain of the replay on NumPy streams (the device's Philox streams are others: the GPU test asserts the same
    from the oracle's side of the replay): births and forced deaths on every 32-leaf branch, both outcomes, no knife edge."""
    from tests.test_hip_leaf_kinds import _counting
    schedule, iters = rl.MT_REPLAYS[name]
    c = rl.mt_case(name)
    p = rl.mt_problem(c)
    o = rm.case_oracle(c, p, cls=_counting(rm.MTOracleRJSampler), schedule=schedule, in_model="gaussian")
    for _ in range(iters):
        o.iteration()
    cnt, cov = rm.Counts(), rl.MTCoverage(lr.MODELS[c["model"]]["nl_max"])
    for info in o.mt_infos:
        cnt.add(o, info, rm.exact_rj_mt(o, info))
        cov.add(o, info)
    rm.assert_sized(cnt, dict(c, inf_prior=False, nan_factor=False, edges=False), name)
    rl.mt_replay_covered(cov, c, name)
    print(f"{name}: {cnt.knife_picks + cnt.knife_accepts + o.knife_swaps} knife-edge")
    assert o.knife_swaps == 0


# ---- B: Gibbs blocks -------------------------------------------------------------------------------------------------------------------------
def test_gibbs_tables_reach_the_limits_they_are_there_for():
    from tests import rj_gibbs_move as rgm
    p = rl.gibbs_problem("four_branches_one_block_per_slot")
    t = rgm.table_of(p["blocks"], p["obr"])
    assert t.shape == (64, 120) and (t.sum(axis=0) == 1).all() and sorted(lr.MODELS["four_branches_64_slots"]["off"]) == [0, 32, 64, 96]
    assert np.cumsum([0, 32, 16, 8])[:].tolist() == [0, 32, 48, 56], "slot0 of the four branches"
    p = rl.gibbs_problem("pulses_RW128_128_blocks")
    t = rgm.table_of(p["blocks"], p["obr"])
    assert t.shape == (128, 126) and np.array_equal(t[:126], np.eye(126, dtype=bool)), "one block per record coordinate"
    assert t[126, :96].all() and not t[126, 96:].any() and t[127, 96:].all() and not t[127, :96].any(), "then one block per branch; block 127 is the last"
    assert lr.slot_coords("pulses_RW128", 0, 21) == (63, 65) and [int(np.flatnonzero(t[k])[0]) for k in (63, 64, 65)] == [63, 64, 65]
    assert 127 << 25 < 1 << 32 and (127 << 19) >> 19 == 127, "block 127 fills the keys' 7 bits"
    p = rl.gibbs_problem("ramp_across_64_splits")
    ms = {(n, tuple(np.flatnonzero(m.any(axis=-1)))) for blk in p["blocks"] for n, m in blk}
    assert ms == {("offset", tuple(range(16))), ("offset", tuple(range(16, 31))), ("ramp", tuple(range(16))), ("ramp", (16,)),
                  ("ramp", tuple(range(17, 31))), ("ramp", (31,))}
    assert lr.slot_coords("ramp_across_64", 1, 16) == (63, 64)
    for name, c in rl.GIBBS_CASES.items():
        assert len(rl.gibbs_problem(name)["blocks"]) == c["nblocks"] <= 128


@pytest.mark.parametrize("name", sorted(rl.GIBBS_CASES))
def test_gibbs_cases_are_sized(name):
    """The teacher-forced chain of the GPU test on the specification alone: no decision within the by-difference bar of its uniform,
    both outcomes; on ramp_across_64 every case of fix_logp_gibbs - a walker without any leaf, one without a moved leaf whose other
    branches hold leaves (-inf), and one whose only leaves sit in non-member slots of the block's own branch (the stored 0.0)."""
    from tests.test_hip_rj_gibbs import _knife
    c = rl.GIBBS_CASES[name]
    p = rl.gibbs_problem(name)
    o = rl.gibbs_oracle(p, c["seed"])
    names = [b.name for b in p["obr"]]
    facts = dict(inf=0, zero=0, empty=0, accepted=0, decisions=0)
    knives = 0
    for _ in range(max(c["forced"], 1)):
        o.iteration()
        rec = o.trace.pop()
        for r in rec["gibbs"]:
            knives += int((_knife(r["lnpdiff"], r["u_acc"], r["betas"][:, None] * r["logl"]) & np.isfinite(r["logp"])).sum())
            rl.gibbs_block_facts(facts, r, {n: r[f"upd_inds_{n}"] for n in names})
    print(f"{name}: {facts}; {knives} knife-edge")
    assert knives == 0 and 0 < facts["accepted"] < facts["decisions"] and facts["empty"] > 0
    if c["table"] == "splits":
        assert facts["inf"] > 0 and facts["zero"] > 0
        # the 0.0 rule leaves a stored log-prior of 0.0 on a walker that holds a leaf
        total = sum(v.sum(axis=-1) for v in o.st.inds.values())
        assert ((o.st.P == 0.0) & (total > 0)).any()


def test_gibbs_draw_statements_are_distinct_per_block():
    u = [rl.gibbs_accept_uniforms(9, 2, 2, 3, k) for k in (0, 1, 127)]
    assert all(v.shape == (2, 3) and ((v >= 0) & (v < 1)).all() for v in u) and len(np.unique(np.concatenate([v.ravel() for v in u]))) == 18
    z = [rl.gibbs_unit_normals(9, 2, 2, 3, 5, k) for k in (0, 127)]
    assert z[0].shape == (2, 3, 5) and not np.isclose(z[0], z[1]).any() and np.abs(z[0]).max() < 7


# ---- E: data-point limits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndata", rl.POINTS_NDATA)
def test_points_cases_are_sized(ndata):
    """257: point 256 is the first point of a lane's second chunk, lane 0's alone; 512: every lane's eighth point; 513: past the resident
    templates.  The composed specification (Gibbs-block in-model move, multiple-try birth / death) on NumPy streams: both outcomes of
    both moves, no knife edge."""
    from tests import rj_gibbs_move as rgm
    from tests.test_hip_leaf_kinds import _counting
    chunks = [(i // 256, (i % 256) // 64, i % 64) for i in range(ndata)]           # (chunk, point of the chunk, lane)
    if ndata == 257:
        assert chunks[256] == (1, 0, 0) and sum(ch == 1 for ch, _, _ in chunks) == 1
    if ndata == 512:
        assert chunks[511] == (1, 3, 63) and ndata == rl.RESIDENT_MAX
    assert (ndata > rl.RESIDENT_MAX) == (ndata == 513)
    c = rl.points_case(ndata)
    p = rm.case_problem(c)
    blocks = rgm.parse_setup([b.name for b in p["obr"]], p["obr"])
    cls = _counting(rl.points_oracle_class())
    o = cls(blocks, p["obr"], p["x"], p["inds"], p["t"], p["y"], p["sigma"], np.random.RandomState(c["seed"] + 101), np.random.RandomState(c["seed"] + 202),
            p["betas"], num_try=c["K"], gens=p["gens"], like_fn=p["like_fn"], schedule=rl.POINTS["schedule"], record=True)
    acc = dec = 0
    for _ in range(rl.POINTS["iters"]):
        o.iteration()
        for r in o.trace.pop()["gibbs"]:
            acc, dec = acc + int(r["accepted"].sum()), dec + r["accepted"].size
    cnt = rm.Counts()
    for info in o.mt_infos:
        cnt.add(o, info, rm.exact_rj_mt(o, info))
    rm.assert_sized(cnt, dict(c, inf_prior=False, nan_factor=False, edges=False), f"{ndata} points")
    assert 0 < acc < dec and o.knife_swaps == 0


# ---- D: periods past coordinate 64 ----------------------------------------------------------------------------------------------------------
def periodic_oracle(p, name, cls_of=lambda cls: cls, R=None, G=None):
    """tests/rj_periodic.production_oracle with the case's Gibbs table and the seam facts kept by the side of coordinate 64."""
    from tests import rj_gibbs_move as rgm
    from tests import rj_periodic as rp
    common = (p["obr"], p["x"], p["inds"], p["t"], p["y"], p["sigma"], R, G, p["betas"])
    kw = dict(record=True, schedule=p["schedule"], like_fn=p["like_fn"])
    if p["move"] == "group":
        o = cls_of(rp.PeriodicGroupOracle)(p["periods"], 3, p["key"], 3, *common, **kw)
    elif p["move"] == "gibbs":
        o = cls_of(rp.PeriodicGibbsOracle)(p["periods"], rgm.parse_setup(p["setup"], p["obr"]), *common, skip_empty=False, **kw)
    else:
        o = cls_of(rp.PeriodicOracle)(p["periods"], *common, in_model=p["move"], live_dangerously=True, **kw)
    off = np.cumsum([0] + [b.nleaves_max * b.ndim for b in p["obr"]])
    o.facts = rl.SeamBySide({b.name: int(off[i]) for i, b in enumerate(p["obr"])})
    return o


def periodic_covered(o, name):
    f = o.facts
    print(f"{name}: {f.line()}")
    assert f.low >= 1 and f.high >= 1, f"{name}: an accepted seam crossing of a phase below coordinate 64 and of one at or past it"
    # (the group move and the Gibbs blocks leave a dead slot where it is and wrap it: x % period; the red / blue stretch move stretches
    #  it toward the complement's slot like any other, stretch.py:136-153, so there the wrapped proposal is all there is to hold it to)
    assert f.dead_high >= 1 and (f.dead_ok or o.in_model == "stretch"), f"{name}: dead phases at or past coordinate 64 hold x % period behind an accept"
    assert f.rejected >= 1


@pytest.mark.parametrize("name", sorted(rl.PERIODIC_CASES))
def test_periodic_cases_are_sized(name):
    """pulses x 12 + sines x 12 (lorentz + chirp): the sine phases at record coordinates 38 .. 71, three of them past 64.  Every move on
    NumPy streams: an accepted seam crossing on either side of coordinate 64, dead phases past 64 rewritten as x % period."""
    from tests import rj_periodic as rp
    p = rl.periodic_problem(name)
    off = 12 * 3
    phases = [off + 3 * s + 2 for s in range(12)]
    assert phases[0] == 38 and phases[-1] == 71 and [c for c in phases if c >= 64] == [65, 68, 71]
    assert p["periods"][p["obr"][-1].name].tolist() == [0.0, 0.0, rp.TWO_PI] and p["wide"] == (name == "wide_stretch")
    o = periodic_oracle(p, name, R=np.random.RandomState(31), G=np.random.RandomState(32))
    o.live = True
    for _ in range(rl.PERIODIC_ITERS):
        o.iteration()
        o.trace.pop()
    periodic_covered(o, name)
