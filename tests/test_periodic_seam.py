"""Periodic parameters at the seam, on the host (no GPU): the exact specification tests/periodic_seam.py against the fixture the REAL
reference recorded (tests/golden/periodic/seam.npz, tests/golden/make_golden_periodic.py) and against the oracle, bit pattern for bit
pattern; the one stated exception, the distance's zero sign, listed by input and shown to be gone after the wrap; the oracle on the
reference's lattice chain; and the sizing of every case tests/test_hip_periodic_seam.py runs on the GPU, from the oracle alone, at
twice the coverage the GPU test asks for."""
import os

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import periodic_seam as ps

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "periodic", "seam.npz")
SPARE = 2                                    # the factor of tests/test_prior_terms.py


@pytest.fixture(scope="module")
def fx():
    return np.load(FIXTURE, allow_pickle=False)


# ---- the specification ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(ps.FAMILIES)), ids=[f"{p:.6g}" for p in ps.FAMILIES])
def test_exact_arithmetic_is_the_reference_and_the_oracle_on_the_whole_matrix(i, fx):
    period = ps.FAMILIES[i]
    pairs, q = ps.edge_matrix(period)
    assert float(fx[f"m{i}_period"]) == period and ps.same_bits(pairs, fx[f"m{i}_pairs"]) and ps.same_bits(q, fx[f"m{i}_q"])
    assert len(pairs) > 250 and len(q) >= 24
    per = np.array([period])
    d_ref, w_ref = fx[f"m{i}_distance"], fx[f"m{i}_wrap"]
    d_orc = orc.periodic_distance(pairs[:, None, 0:1].copy(), pairs[:, None, 1:2].copy(), per)[:, 0, 0]
    w_orc = orc.periodic_wrap(q[:, None, None].copy(), per)[:, 0, 0]
    d_masked, w = ps.exact_matrix(period, "masked")
    d_select, _ = ps.exact_matrix(period, "select")
    assert ps.same_bits(d_orc, d_ref), "the oracle's distance is not the reference's"
    assert ps.same_bits(w_orc, w_ref), "the oracle's wrap is not the reference's"
    assert ps.same_bits(d_masked, d_ref), "exact arithmetic in the reference's masked-sum form is not the reference"
    assert ps.same_bits(w, w_ref), "the exact remainder is not the reference's"
    # the select form: the reference everywhere but on the listed inputs, where the two zeros have opposite signs
    exc = ps.zero_sign_exceptions(period)
    differ = np.flatnonzero(ps.bits(d_select) != ps.bits(d_ref))
    assert np.array_equal(differ, exc), f"select form differs from the reference on rows {differ}, stated exception {exc}"
    if period > 0.0:
        assert exc.size == 1 and pairs[exc[0], 0] == period and np.signbit(pairs[exc[0], 1]) and pairs[exc[0], 1] == 0.0
        assert d_ref[exc[0]] == 0.0 and np.signbit(d_ref[exc[0]]) and d_select[exc[0]] == 0.0 and not np.signbit(d_select[exc[0]])
        # the matrix sits where it claims: real ties, remainders of zero, remainders on the period itself
        h = period / 2.0
        assert int((np.abs(pairs[:, 1] - pairs[:, 0]) == h).sum()) >= 20
        assert int((w == period).sum()) >= 2 and int((w == 0.0).sum()) >= 8 and not np.signbit(w[w == 0.0]).any()
        assert np.all((w >= 0.0) & (w <= period))
        assert ps.exact_wrap(-1e-300, period) == period, "NumPy has -1e-300 % p == p"
    else:
        assert ps.same_bits(d_select, pairs[:, 1] - pairs[:, 0]) and ps.same_bits(w, q), "not periodic: untouched"


def test_a_tie_keeps_the_long_way():
    for p in ps.DYADIC:
        h = p / 2.0
        assert ps.exact_distance(0.0, h, p) == h and ps.exact_distance(h, 0.0, p) == -h
        assert ps.exact_distance(0.0, np.nextafter(h, np.inf), p) < 0.0 and ps.exact_distance(0.0, np.nextafter(h, 0.0), p) > 0.0
        assert ps.exact_distance(p / 8.0, 5.0 * p / 8.0, p) == h, "an eighth and five eighths are a real tie on a dyadic period"


def test_the_zero_sign_is_erased_by_the_wrap():
    """s == period, c == -0.0: the two forms' distances are -0.0 and +0.0, the proposals +0.0 and -0.0, and the wrapped proposal is
    +0.0 for both, with every draw - the difference cannot reach a stored position"""
    for period in ps.DYADIC + (ps.TWO_PI,):
        for a, us in ps.DRAWS.items():
            for u in us:
                zz = ps.stretch_factor(a, u)
                q_s, w_s = ps.exact_proposal(period, -0.0, zz, period, "select")
                q_m, w_m = ps.exact_proposal(period, -0.0, zz, period, "masked")
                assert q_s == 0.0 and q_m == 0.0 and np.signbit(q_s) != np.signbit(q_m)
                assert ps.same_bits(w_s, w_m) and w_s == 0.0 and not np.signbit(w_s)
                per = np.array([period])
                s, c = np.full((1, 1, 1), period), np.full((1, 1, 1), -0.0)
                qo = c - orc.periodic_distance(s, c, per) * zz
                assert ps.same_bits(qo.ravel()[0], q_m) and ps.same_bits(orc.periodic_wrap(qo.copy(), per).ravel()[0], w_s)


def test_dyadic_draws_are_exact():
    for (a, u), zz in ps.EXACT_ZZ.items():
        assert ps.stretch_factor(a, u) == zz and u in ps.DRAWS[a]
    # ... and land proposals exactly on 0, on the period and on its multiples
    for p in ps.DYADIC:
        assert ps.exact_proposal(0.0, p / 4.0, 1.0, p)[0] == 0.0
        assert ps.exact_proposal(0.0, 5.0 * p / 8.0, 1.0, p)[0] == p                 # the short way round: new_s = p
        assert ps.exact_proposal(p / 8.0 + 2.0 * p, 5.0 * p / 8.0, 1.0, p)[0] == p / 8.0 + p
        assert ps.exact_proposal(-p / 4.0, 0.0, 0.25, p) == (-p / 16.0, p - p / 16.0)


def test_lattice_probabilities():
    """of the 64 ordered pairs of lattice points 8 are at exactly half a period and 12 beyond it"""
    i, j = np.meshgrid(np.arange(8), np.arange(8))
    assert int((np.abs(i - j) == 4).sum()) == 8 and int((np.abs(i - j) > 4).sum()) == 12
    per = ps.row_periods(7)
    x = ps.lattice_state(4, 64, 7, per, np.random.RandomState(0))
    pc = per > 0
    assert np.array_equal(x[..., pc] / per[pc] * 8.0, np.round(x[..., pc] / per[pc] * 8.0)) and np.all(np.abs(x[..., ~pc]) < 1.0)
    d = np.abs(x[:, :32, pc] - x[:, 32:, pc])
    assert 0.08 < (d == per[pc] / 2.0).mean() < 0.17 and 0.13 < (d > per[pc] / 2.0).mean() < 0.25


def test_row_periods_never_repeat_next_door():
    for D in (5, 8, 11, 12, 16, 32, 64, 128):
        fam = [set(), set()]
        for shift in ps.SHIFTS:
            per = ps.row_periods(D, shift)
            assert np.all(per[1:] != per[:-1]), "neighbours share a period: a swapped index would not show"
            for d in range(D):
                fam[d % 2].add(per[d])
        assert fam[0] | fam[1] == set(ps.FAMILIES)
        if D >= 8:                           # (a row of 5 has two odd coordinates: four families between the two shifts)
            assert fam[0] == fam[1] == set(ps.FAMILIES), "every family on both halves of a 16-byte lane"


# ---- the reference's lattice chain ---------------------------------------------------------------------------------------------------------
class _Chain:
    """the fixture's ``chain_`` keys under their names in the p* fixtures"""

    def __init__(self, fx):
        self._fx = fx
        self.files = [k[len("chain_"):] for k in fx.files if k.startswith("chain_")]

    def __getitem__(self, k):
        return self._fx["chain_" + k]


def test_oracle_reproduces_the_lattice_chain_bit_for_bit(fx, monkeypatch):
    from tests.test_oracle_golden import build_mh_oracle
    ch = _Chain(fx)
    T, W, D, n = int(ch["T"]), int(ch["W"]), int(ch["D"]), int(ch["nsteps"])
    assert (T, W, D, n) == (3, 16, 5, 12) and np.array_equal(ch["period"] > 0, [True, False, True, False, True])
    # three quarters of the 100 kB the fixture was given: 41 kB of it are the chain's positions and MH proposals, doubles that do not
    # compress, at the shape and length the chain was asked to have
    assert os.path.getsize(FIXTURE) < 75_000
    cnt = ps.new_counts()
    ps.install(monkeypatch, cnt)
    o = build_mh_oracle(ch)
    picked = np.zeros(2, dtype=int)
    for it in range(n):
        o.iteration()
        rec, pre = o.trace[-1], f"it{it}_"
        assert rec["move"] == int(ch[pre + "move"])
        picked[rec["move"]] += 1
        if "mh_q" in rec:
            assert ps.same_bits(rec["mh_q"], ch[pre + "mh_q"])
        for k in ("x", "L"):
            assert ps.same_bits(rec[k], ch[pre + k]), f"{k} after iteration {it}"
        assert ps.same_bits(o.betas, ch[pre + "betas"]), "the ladder, adapted from the swap counts"
    assert picked.min() >= 2, "both moves were picked"
    ps.assert_counts(cnt, ("tie", "fix_neg", "fix_pos", "wrap_neg", "wrap_ge"), 10, "the reference's lattice chain")


# ---- sizing, oracle only: a. the teacher-forced sites -----------------------------------------------------------------------------------
@pytest.mark.parametrize("site", sorted(ps.FORCED_SITES))
def test_forced_sites_are_sized_with_a_factor_of_two_to_spare(site, monkeypatch):
    s = ps.FORCED_SITES[site]
    kind = s.get("kind", "stretch")
    cnt = ps.new_counts()
    ps.install(monkeypatch, cnt)
    on_period, coords, fams, rows = 0, set(), set(), {}
    for shift in ps.SHIFTS:
        W = ps.forced_width(s["D"], shift)
        assert W // 2 > 128 and (W // 2) % 64 != 0 and 200 <= W <= 400, "two tiles of moving walkers and a ragged one, a few hundred walkers"
        assert W == ps.BLOCK * len(ps.forced_families(s["D"], shift)) and len(ps.edge_matrix(1.0)[0]) % ps.BLOCK == 0
        loose, tight = ps.site_problem(site, shift, False), ps.site_problem(site, shift, True)
        for call in ps.forced_calls(s["D"], shift, kind):
            st = ps.forced_state(call, loose)
            out, x, L, P = ps.forced_oracle(call, loose, st)
            assert out["keep"].all(), "a proposal left the loose box: the case is not what it claims"
            out_t, *_ = ps.forced_oracle(call, tight, st)
            per = loose.period
            sits = ((out["q"] == per) & (per > 0)).any(axis=-1)
            assert np.array_equal(~out_t["keep"], sits), "the tight box refuses exactly the proposals wrapped onto a period"
            on_period += int(sits.sum())
            coords |= set(call["d"].ravel().tolist())
            fams |= set(per[call["d"]].ravel().tolist())
            assert np.array_equal(call["fam"], per[call["d"]]), "a placement on a coordinate of another period"
            draw = (call["a"], float(call["u_zz"][0, 0])) if kind == "stretch" else None
            for p in ps.forced_families(s["D"], shift):
                rows.setdefault((shift, draw, p), set()).update(call["row"][call["fam"] == p].tolist())
            if kind == "stretch":            # the oracle's proposals on the seam coordinates are exact arithmetic's
                tt, kk = np.meshgrid(np.arange(call["d"].shape[0]), np.arange(call["d"].shape[1]), indexing="ij")
                assert ps.same_bits(out["q"][tt, kk, call["d"]], ps.forced_reference(call))
            else:
                tt, kk = np.meshgrid(np.arange(call["d"].shape[0]), np.arange(call["d"].shape[1]), indexing="ij")
                want = np.array([[ps.exact_wrap(call["q"][t, k], per[call["d"][t, k]]) for k in range(kk.shape[1])] for t in range(2)])
                assert ps.same_bits(out["q"][tt, kk, call["d"]], want)
    assert coords == set(range(s["D"])) and fams == set(ps.FAMILIES), "every coordinate, every period family"
    # every row of every period's matrix (without a period: every row inside the box), with every draw, under both shifts of the row
    draws = [(a, u) for a in ps.DRAWS for u in ps.DRAWS[a]] if kind == "stretch" else [None]
    assert set(rows) == {(sh, dr, p) for sh in ps.SHIFTS for dr in draws for p in ps.forced_families(s["D"], sh)}
    for (sh, dr, p), seen in rows.items():
        n = len(ps.site_matrix(p, kind))
        assert seen == set(range(n)), f"{site}: shift {sh}, draw {dr}, period {p}: {len(seen)} of {n} rows of the matrix are run"
        assert n == len(ps.edge_matrix(p)[0 if kind == "stretch" else 1]) or p == 0.0
    ps.assert_counts(cnt, ps.FORCED_CLAIMS[kind], SPARE * ps.LEAST * 2, site)      # (counted once per box: twice)
    assert on_period >= SPARE * ps.LEAST, f"{site}: {on_period} proposals wrapped onto a period"


# ---- b. production stepping from the lattice ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ps.LATTICE_CASES))
def test_lattice_cases_are_sized_with_a_factor_of_two_to_spare(name, monkeypatch):
    cnt = ps.oracle_lattice_case(monkeypatch, name)
    ps.assert_counts(cnt, ps.LATTICE_CLAIMS, SPARE * ps.LEAST, name)
