"""The limit models of tests/limit_records.py on the host (no GPU): the table's arithmetic against RJEngine's own, the mask round
trip at bit 31, the coverage the teacher-forced GPU cases rely on - counted from the oracle on the same host draws -, and the float64
oracle's own distance from exact arithmetic on every model's starts (the yardstick the 1e-12 and 4 B bars of
tests/test_hip_limit_records.py lean on)."""
import numpy as np
import pytest

from oracle import eryn_oracle_rj as orj
from tests import exact_leaf_kinds as xk
from tests import leaf_kinds as lk
from tests import limit_records as lr
from tests.test_hip_leaf_kinds import _knife_accepts


def _engine(model, T=2, W=4):
    """RJEngine's packing and layout without a context (the way tests/test_host_logic.py builds one)."""
    from eryn_amd.rj import RJEngine
    eng = RJEngine.__new__(RJEngine)
    eng.branches = [b.to_device() for b in lr.branches(model)]
    eng.T, eng.W = T, W
    eng.ncoord = sum(b.nleaves_max * b.ndim for b in eng.branches)
    rw = eng.ncoord + len(eng.branches)
    eng.RW = rw + (rw & 1)
    eng.off = np.cumsum([0] + [b.nleaves_max * b.ndim for b in eng.branches])[:-1]
    return eng


@pytest.mark.parametrize("model", sorted(lr.MODELS))
def test_the_table_states_the_layout_the_engine_computes(model):
    row = lr.MODELS[model]
    off, ncoord, slots, RW = lr.layout(model)
    assert (off, ncoord, slots, RW) == (row["off"], row["ncoord"], row["slots"], row["RW"]), "the row's stated arithmetic"
    assert lr.across_64(model) == row["across"]
    assert len(row["nl_max"]) <= 4 and max(row["nl_max"]) <= 32 and slots <= 64 and RW <= 128, "inside what the API admits"
    eng = _engine(model)
    assert tuple(int(v) for v in eng.off) == off and eng.ncoord == ncoord and eng.RW == RW
    # RJEngine's own constructor arithmetic is the same expression (eryn_amd/rj.py): one past the record is refused there
    for b, s in lr.edges(model):
        first, last = lr.slot_coords(model, b, s)
        assert off[b] <= first <= last < (off + (ncoord,))[b + 1]


def test_every_row_produces_the_edge_it_is_there_for():
    sc = lr.slot_coords
    m = "four_branches_64_slots"
    assert lr.MODELS[m]["slots"] == 64 and len(lr.MODELS[m]["nl_max"]) == 4 and lr.widths(m) == (1, 2, 4, 3)
    assert sc(m, 1, 15) == (62, 63) and sc(m, 2, 0) == (64, 67) and (0, 31) in lr.edges(m)
    assert sc("burst_across_64", 1, 15) == (61, 64) and all(sc("burst_across_64", 1, s)[0] % 2 == 1 for s in range(30))
    assert sc("ramp_across_64", 1, 16) == (63, 64) and (1, 31) in lr.edges("ramp_across_64")
    assert lr.MODELS["ramp_across_64"]["nl_max"] == (31, 32)                       # numpy_sum: n % 8 == 7 and n == 32
    assert sc("pulses_RW128", 0, 21) == (63, 65) and lr.layout("pulses_RW128")[1] + 2 == 128 and sc("pulses_RW128", 1, 0)[0] == 96
    assert [lr.layout(f"coords_{n}")[1] for n in (63, 64, 65)] == [63, 64, 65]
    assert sc("coords_65", 1, 0) == (64, 64)
    assert lr.MODELS["general_ndims_1234"]["slots"] == 64 and lr.widths("general_ndims_1234") == (1, 2, 3, 4)
    assert sc("general_RW128", 1, 15) == (61, 64) and lr.layout("general_RW128")[3] == 128 and lr.layout("general_RW128")[1] + 3 == 128
    for model in lr.MODELS:
        for b, n in enumerate(lr.MODELS[model]["nl_max"]):
            assert (b, 0) in lr.edges(model) and ((b, 31) in lr.edges(model)) == (n == 32)
        assert set(lr.across_64(model)) <= set(lr.edges(model))


@pytest.mark.parametrize("model", ["four_branches_64_slots", "ramp_across_64", "pulses_RW128", "general_ndims_1234"])
def test_records_round_trip_with_bit_31(model):
    """pack / unpack (the record's mask doubles) with bit 31 set and clear, and the masks 0, 2^31 and 2^32 - 1."""
    T, W = 2, 4
    eng = _engine(model, T, W)
    x, inds, _ = lr.start(model, T, W)
    B = [b for b, n in enumerate(lr.MODELS[model]["nl_max"]) if n == 32][0]
    name = eng.branches[B].name
    inds[name][0, 0] = False                                                       # mask 0
    inds[name][0, 1] = False
    inds[name][0, 1, 31] = True                                                    # 2^31
    inds[name][0, 2] = True                                                        # 2^32 - 1
    inds[name][0, 3] = True
    inds[name][0, 3, 31] = False                                                   # 2^31 - 1: bit 31 clear under 31 set bits
    rec = eng.pack(x, inds)
    assert rec.shape == (T, W, lr.MODELS[model]["RW"])
    assert rec[0, :, eng.ncoord + B].tolist() == [0.0, 2147483648.0, 4294967295.0, 2147483647.0]
    x2, inds2 = eng.unpack(rec)
    for b in eng.branches:
        assert np.array_equal(inds2[b.name], inds[b.name]) and np.array_equal(x2[b.name], x[b.name]), b.name
    x3, inds3 = eng.unpack(rec, nan_fill=True)
    assert np.isnan(x3[name][0, 1, :31]).all() and np.isfinite(x3[name][0, 1, 31]).all() and np.isfinite(x3[name][0, 2]).all()
    if rec.shape[-1] > eng.ncoord + len(eng.branches):
        assert np.all(rec[:, :, -1] == 0.0), "the pad"


def test_starts_hold_every_walker_class_on_every_edge():
    for model in lr.MODELS:
        brs = lr.branches(model)
        x, inds, classes = lr.start(model, lr.TF_T, lr.TF_W)
        seen = set()
        for tt in range(lr.TF_T):
            for w in range(lr.TF_W):
                c, B, s = classes[tt, w]
                seen.add((c, B, s))
                n = {b.name: int(inds[b.name][tt, w].sum()) for b in brs}
                if c == "empty":
                    assert sum(n.values()) == 0
                elif c == "last_only":
                    assert sum(n.values()) == n[brs[-1].name] == 1
                else:
                    m = inds[brs[B].name][tt, w]
                    nl = brs[B].nleaves_max
                    assert {"all_but": not m[s] and m.sum() == nl - 1, "pair": m[s] and m.sum() == min(2, nl),
                            "full": m.all(), "half": m[s]}[c], (model, c, B, s)
        assert {(c, B, s) for (B, s) in lr.edges(model) for c in lr.CLASSES} <= seen, model
        for b in brs:                                                              # every slot holds a leaf inside its box
            lo, hi = np.array([q[0] for q in b.box]), np.array([q[1] for q in b.box])
            assert np.all((x[b.name] > lo) & (x[b.name] < hi))


@pytest.mark.parametrize("case", lr.TF_CASES, ids=lr.case_id)
def test_teacher_forced_cases_cover_every_edge(case):
    """The oracle alone on the host draws of a teacher-forced case (what tests/test_hip_limit_records.py feeds the device move by
    move): every pair of edges(model) sees an accepted birth, an accepted death, an accepted in-model move and - Gaussian in-model
    move - a proposal rejected for that slot alone, by its lowest and by its highest coordinate; no decision on the knife edge."""
    model, ndata, schedule, in_model = case
    o, brs, _ = lr.tf_oracle(*case)
    cov, knives = lr.Coverage(brs), 0
    for _ in lr.tf_iterations(o, brs, model):
        o.iteration()
        rec = o.trace.pop()
        knives += _knife_accepts(rec)
        cov.add(rec)
    gaussian = in_model == "gaussian"
    print(f"{case}: {cov.line(lr.edges(model))}; knife-edge accepts {knives}, swaps {o.knife_swaps}")
    assert cov.missing(lr.required(model, sole=gaussian)) == []
    if gaussian:
        for b, s in lr.edges(model):
            assert cov.sole_coord[b][s, 0] >= 1 and cov.sole_coord[b][s, brs[b].ndim - 1] >= 1, "sole offender: lowest, highest coordinate"
    assert knives == 0 and o.knife_swaps == 0


EXACT_STATES = [(m, nd) for m in lr.DEVICE_MODELS for nd in ((40, 130) if m == "pulses_RW128" else (40,))]


@pytest.mark.parametrize("model,ndata", EXACT_STATES)
def test_the_oracle_is_within_one_bound_of_exact_arithmetic_at_the_limits(model, ndata):
    """float64 (tests/leaf_kinds.py, the oracle's likelihood) against the exact-arithmetic log-likelihood on the class start and on
    the 97 % start: <= 1 B and <= 1e-13 relative.  (B / |L*| is printed: a bound of a few 1e-13, so 1e-12 against the oracle and 4 B
    against exact arithmetic are both within a correct kernel's reach.)"""
    brs, t, y, sigma = lr.problem(model, ndata)
    worst_B = worst_rel = ratio = 0.0
    for x, inds in (lr.start(model, 2, 16)[:2], lr.dense_state(model, 2, 16)):
        Ls, B = xk.yardstick(brs, x, inds, t, y, sigma)
        L = lk.template_log_like(brs, x, inds, t, y, sigma)
        live = sum(v.sum(axis=-1) for v in inds.values()) > 0
        worst_B = max(worst_B, float(np.max(np.abs(L - Ls)[live] / B[live])))
        worst_rel = max(worst_rel, float(np.max(np.abs(L / Ls - 1)[live])))
        ratio = max(ratio, float(np.max((B / np.abs(Ls))[live])))
        P = orj.compute_log_prior(x, inds, [b.to_oracle() for b in brs])
        assert np.isfinite(P).all()
    print(f"{model} at {ndata} points: oracle vs exact {worst_B:.3g} B, {worst_rel:.3g} relative; B / |L*| <= {ratio:.3g}")
    assert worst_B <= 1.0 and worst_rel <= 1e-13
