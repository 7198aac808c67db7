"""The newer leaf-packing moves at the record's limits: the cases, starts and coverage conditions of tests/test_rj_limit_moves.py (no
GPU: every case sized on the specification alone) and tests/test_hip_rj_limit_moves.py, stated once.  Host only, NumPy.

Models, branches, data and starts are tests/limit_records.py's (``start``'s walker classes all_but / pair / full / half and the
``empty`` and ``last_only`` walkers); the pairs to cover are ``edges(model)``: slot 0 of every branch, slot 31 of every 32-leaf
branch, every slot across coordinate 64.  The moves' rules are the existing specification modules', imported and not restated.

Section A - the multiple-try birth / death move (tests/rj_mt_move.py; k_rj_mt).  What the limits reach in the kernel: the mask of a
full 32-leaf branch (``nl >= 32 ? 0xffffffff : (1 << nl) - 1``), ``1 << leaf`` at leaf 31, the branch's sum of slot log-priors over
31 and 32 slots with the try in slot 0 and in the top slot, the membership bits shifted by ``slot0`` up to 56, a try's coordinates
written across coordinate 64.  Every proposal starts from the class start again (a teacher-forced proposal uploads its state anyway),
so that every round deals every edge its all_but, pair and full walkers; MT_ROUNDS rounds over the branches.
"""
import numpy as np

from oracle import eryn_oracle_rj as orj
from tests import leaf_kinds as lk
from tests import limit_records as lr
from tests import rj_mt_move as rm
from tests import rj_prior_terms as rpt

T, W, NDATA = 2, 48, 40

# ---- A: k_rj_mt ----------------------------------------------------------------------------------------------------------------------------
# the GPU file runs MT_ROUNDS rounds; tests/test_rj_limit_moves.py runs MT_ROUNDS_CPU of the same stream, asks for the coverage after
# MT_ROUNDS_SPARE of them already and for no decision on a knife edge over all of them.  The seeds are those at which that holds.
MT_ROUNDS_SPARE, MT_ROUNDS, MT_ROUNDS_CPU = 2, 3, 4
MT_CASES = {
    "four_branches_64_slots_k7": dict(model="four_branches_64_slots", ndata=40, K=7, prior="box", seed=1),
    "pulses_RW128_nd130_k5": dict(model="pulses_RW128", ndata=130, K=5, prior="box", seed=2),
    "ramp_across_64_k64": dict(model="ramp_across_64", ndata=40, K=64, prior="box", seed=1),
    "burst_across_64_k2": dict(model="burst_across_64", ndata=40, K=2, prior="box", seed=1),
    # prior terms with a generator of its own on offset x 31 + ramp x 32 (ramp_across_64's layout and class masks): the branch's sum
    # of slot log-priors (numpy_sum_sub) runs over n = 31 and n = 32 with the try in slot 0 and in slot 30 / 31
    "terms_31_32_k5": dict(model="ramp_across_64", ndata=40, K=5, prior="terms", seed=1),
}
TERMS_KINDS, TERMS_NL = ("offset", "ramp"), (31, 32)
TERMS_TOP = (0, 30)          # the 31-slot branch's top slot: no pair of ``edges``, covered in the terms case beside them
# generators wider than the priors of tests/rj_prior_terms.ENTRIES (a ramp's slope beyond its support: tries with a -inf prior)
TERMS_GEN = {0: [("normal", 0.0, 1.0)], 1: [("uniform", -1.25, 1.25), ("normal", 0.0, 0.8)]}


def mt_case(name):
    """The case as tests/test_hip_rj_mt.py's helpers take one (T, W, K, seed, nprop and the flags of ``rj_mt_move.assert_sized``)."""
    c = MT_CASES[name]
    nb = len(lr.MODELS[c["model"]]["nl_max"])
    return dict(c, T=T, W=W, nprop=MT_ROUNDS * nb, inf_prior=False, nan_factor=False, edges=True)


def mt_problem(c):
    """tests/rj_mt_move.case_problem's dict on a limit model: branches, data and class start of tests/limit_records.py (the terms case:
    the coordinates drawn from the priors, the masks ``start``'s), plus ``classes``."""
    model, seed = c["model"], c["seed"]
    betas = 0.35 ** np.arange(T)
    _, inds, classes = lr.start(model, T, W, seed)
    if c["prior"] == "terms":
        assert lr.MODELS[model]["kinds"] == TERMS_KINDS and lr.MODELS[model]["nl_max"] == TERMS_NL
        rs = np.random.RandomState(1000 + seed)
        obr = rpt.branches_of(TERMS_KINDS, TERMS_NL, (0, 0))
        t = np.linspace(-1, 1, c["ndata"])
        y = lr.SIGMA[c["ndata"]] * rs.randn(c["ndata"])
        for b in obr:
            y = y + lk.leaf_value(b.kind_name, b.rvs(1, rs)[0], t)
        x, _ = rpt.start_state(obr, T, W, rs)
        for w in range(W):                                  # the warm rung's all-but-slot-0 offsets: all but the TOP slot (30) instead
            if tuple(classes[1, w]) == ("all_but", 0, 0):
                inds[obr[0].name][1, w] = np.arange(TERMS_NL[0]) != TERMS_NL[0] - 1
                classes[1, w] = ("all_but",) + TERMS_TOP
        gens = [rm.pt.make_spec(TERMS_GEN[i]) for i in range(len(obr))]
        return dict(obr=obr, dbr=rpt.device_branches(obr), t=t, y=y, sigma=lr.SIGMA[c["ndata"]], x=x, inds=inds, betas=betas, gens=gens,
                    dev_gens={b.name: g for b, g in zip(obr, gens)}, like_fn=lk.like_fn(TERMS_KINDS), scale=rpt.scales(obr), classes=classes)
    brs, t, y, sigma = lr.problem(model, c["ndata"], seed)
    x, inds, classes = lr.start(model, T, W, seed)
    scale = [np.array([0.02 * (hi - lo) for lo, hi in b.box]) for b in brs]
    obr = [b.to_oracle(cov=np.diag(s ** 2)) for b, s in zip(brs, scale)]
    return dict(obr=obr, dbr=[b.to_device() for b in brs], t=t, y=y, sigma=sigma, x=x, inds=inds, betas=betas, gens=[None] * len(brs),
                dev_gens=None, like_fn=lk.like_fn(lr.like_kinds(model)), scale=scale, classes=classes)


class MTCoverage:
    """Per (branch, slot), from the specification's ``info`` of every proposal: accepted births into the slot, proposed and accepted
    deaths of it, births landing at nleaves_max (the edge factor), births whose pick is not try 0; per branch the forced deaths of a
    walker with 32 leaves (the candidates' mask 0xffffffff)."""
    KEYS = ("birth_acc", "death_prop", "death_acc", "birth_at_max", "pick_beyond_0")

    def __init__(self, nl_max):
        self.nl_max = tuple(nl_max)
        self.n = {k: [np.zeros(n, dtype=int) for n in self.nl_max] for k in self.KEYS}
        self.forced_32 = np.zeros(len(self.nl_max), dtype=int)

    def add(self, o, info):
        bi = info["bi"]
        b = o.branches[bi]
        ch, leaf, keep, pick = info["change"], info["leaf"], info["keep"], info["pick"].reshape(info["change"].shape)
        nold = rm.o_nleaves_before(info, b)
        birth, death = ch == +1, ch == -1
        for key, m in (("birth_acc", birth & keep), ("death_prop", death), ("death_acc", death & keep),
                       ("birth_at_max", birth & (nold == b.nleaves_max - 1)), ("pick_beyond_0", birth & (pick != 0))):
            np.add.at(self.n[key][bi], leaf[m], 1)
        if b.nleaves_max == 32:
            self.forced_32[bi] += int((death & (nold == 32)).sum())

    def line(self, pairs):
        return "; ".join(f"({b}, {s}): " + " ".join(f"{k} {int(self.n[k][b][s])}" for k in self.KEYS) for b, s in pairs) + \
            f"; forced deaths at 32 leaves per branch {self.forced_32.tolist()}"

    def missing(self, pairs):
        """What is asked of every pair and did not happen (``limit_records.required``'s rule: the one leaf of a one-leaf branch cannot
        die, there the PROPOSED death counts)."""
        out = []
        for b, s in pairs:
            for k in ("birth_acc", "death_acc", "birth_at_max", "pick_beyond_0"):
                key = "death_prop" if (k == "death_acc" and self.nl_max[b] == 1) else k
                if self.n[key][b][s] < 1:
                    out.append((b, s, key))
        out += [(b, None, "forced_32") for b, n in enumerate(self.nl_max) if n == 32 and self.forced_32[b] < 1]
        return out


def mt_forced_run(c, rounds, on_proposal=None, p=None, on_round=None):
    """tests/rj_mt_move.forced_run on a limit case: ``rounds`` rounds over the branches, every proposal from the class start, a sweep
    without adaptation behind each -> (Counts, MTCoverage).  on_round(rounds done, Counts, MTCoverage) after every round."""
    p = p or mt_problem(c)
    o = rm.case_oracle(c, p)
    L0, P0 = o.st.L.copy(), o.st.P.copy()
    cnt, cov = rm.Counts(), MTCoverage(lr.MODELS[c["model"]]["nl_max"])
    for n in range(rounds * len(o.branches)):
        bi = n % len(o.branches)
        o.st = orj.RJState(p["x"], p["inds"], L0, P0, p["betas"])
        inputs = o.draw_inputs(bi)
        info, pre, mid, sweep = {}, {}, {}, {}
        o._snapshot(pre, "")
        rm.mt_bd_step(o, bi, *inputs, gen=o.gens[bi], info=info)
        ex = rm.exact_rj_mt(o, info)
        cnt.add(o, info, ex)
        cov.add(o, info)
        o._snapshot(mid, "")
        o._pt(False, sweep)
        if on_proposal is not None:
            on_proposal(o, bi, inputs, info, ex, sweep, pre, mid)
        if on_round is not None and bi == len(o.branches) - 1:
            on_round(n // len(o.branches) + 1, cnt, cov)
    return cnt, cov


def mt_pairs(c):
    """The pairs a case must cover: ``edges(model)`` (the terms case: and the 31-slot branch's top slot)."""
    return lr.edges(c["model"]) + ([TERMS_TOP] if c["prior"] == "terms" else [])


def mt_assert_covered(cnt, cov, c, what):
    rm.assert_sized(cnt, c, what)
    print(f"{what}: coverage {cov.line(mt_pairs(c))}; {cnt.knife_picks + cnt.knife_accepts} knife-edge")
    assert cov.missing(mt_pairs(c)) == [], f"{what}: edges without coverage"
    if c["prior"] == "terms":
        assert cnt.inf_prior >= 1, f"{what}: no try with a -inf prior"


# hens_rj_step under the move, replayed through the specification (the production launch: coin, candidates' mask and leaf slot are the
# kernel's own there - a birth on a 32-leaf branch picks among ~mask & 0xffffffff): name -> (schedule, iterations)
MT_REPLAYS = {"pulses_RW128_nd130_k5": ("iterate_branches", 4), "ramp_across_64_k64": ("iterate_branches", 4),
              "four_branches_64_slots_k7": ("separate_branches", 4)}


def mt_replay_covered(cov, c, what):
    """What a replay must have seen on every 32-leaf branch, counted from the specification's side: a birth (proposed into a slot the
    kernel picked out of ~mask & full) and a forced death of a full branch."""
    nl = lr.MODELS[c["model"]]["nl_max"]
    births = [int(sum(cov.n["birth_acc"][b]) + sum(cov.n["birth_at_max"][b])) for b in range(len(nl))]
    print(f"{what}: births accepted or landing at the ceiling per branch {births}, forced deaths at 32 leaves {cov.forced_32.tolist()}")
    for b, n in enumerate(nl):
        assert n != 32 or (births[b] >= 1 and cov.forced_32[b] >= 1), f"{what}: branch {b} (32 leaves)"


# ---- B: Gibbs blocks of the in-model Gaussian move (tests/rj_gibbs_move.py; k_rj_gibbs) ------------------------------------------------
def limit_problem(model, ndata=NDATA, seed=1, W_=W):
    """A limit model's data and class start as the Gibbs / periodic harnesses take a problem."""
    brs, t, y, sigma = lr.problem(model, ndata, seed)
    x, inds, classes = lr.start(model, T, W_, seed)
    scale = [np.array([0.02 * (hi - lo) for lo, hi in b.box]) for b in brs]
    kinds = lr.like_kinds(model)
    plain = set(kinds) <= {"pulse", "sine"}
    return dict(brs=brs, obr=[b.to_oracle(cov=np.diag(s ** 2)) for b, s in zip(brs, scale)], dbr=[b.to_device() for b in brs], t=t, y=y,
                sigma=sigma, x=x, inds=inds, classes=classes, betas=0.35 ** np.arange(T), scale=scale, kinds=kinds,
                like_fn=None if plain else lk.like_fn(kinds), T=T, W=W_)


def _slots(b, sel):
    """The block entry (name, mask [nl, ndim]) of branch b with every coordinate of the slots ``sel`` true."""
    m = np.zeros((b.nleaves_max, b.ndim), dtype=bool)
    m[list(sel)] = True
    return (b.name, m)


def gibbs_setup(table, obr):
    """``gibbs_sampling_setup`` of a case.  "slots": one block per leaf slot of every branch (membership ballot bits 0 .. nslots - 1);
    "coordinates": one block per record coordinate (partial masks: a slot is a member of as many blocks as it has parameters) and then
    one whole-branch block per branch - 128 blocks on pulses_RW128, block 127 the last key the 7 key bits hold; "splits": each branch's
    slots split at slot 16 (ramp slot 16 = coordinates 63 | 64 a block of its own) and at the 32-leaf edge (slot 31 a block of its own)."""
    if table == "slots":
        return [_slots(b, [s]) for b in obr for s in range(b.nleaves_max)]
    if table == "coordinates":
        out = []
        for b in obr:
            for s in range(b.nleaves_max):
                for d in range(b.ndim):
                    m = np.zeros((b.nleaves_max, b.ndim), dtype=bool)
                    m[s, d] = True
                    out.append((b.name, m))
        return out + [b.name for b in obr]
    if table == "splits":
        out = []
        for b in obr:
            n = b.nleaves_max
            cuts = [range(0, 16), range(16, n)] if n < 32 else [range(0, 16), [16], range(17, 31), [31]]
            out += [_slots(b, c) for c in cuts]
        return out
    raise KeyError(table)


# name: model, table, blocks it must have, iterations teacher-forced / replayed, full covariances in the replay
GIBBS_CASES = {
    "four_branches_one_block_per_slot": dict(model="four_branches_64_slots", table="slots", nblocks=64, forced=2, replay=3, chol=False, seed=1),
    "pulses_RW128_128_blocks": dict(model="pulses_RW128", table="coordinates", nblocks=128, forced=1, replay=3, chol=False, seed=1),
    "pulses_RW128_128_blocks_full_covariances": dict(model="pulses_RW128", table="coordinates", nblocks=128, forced=0, replay=3, chol=True, seed=2),
    "ramp_across_64_splits": dict(model="ramp_across_64", table="splits", nblocks=6, forced=3, replay=4, chol=False, seed=1),
}
GIBBS_REPLAY_SEED = 23
PURPOSE_MH_NORMAL = 12


def gibbs_problem(name):
    from tests import rj_gibbs_move as rgm
    c = GIBBS_CASES[name]
    p = limit_problem(c["model"], seed=c["seed"])
    p["setup"] = gibbs_setup(c["table"], p["obr"])
    p["blocks"] = rgm.parse_setup(p["setup"], p["obr"])
    p["chol"] = None
    if c["chol"]:                                           # (tests/test_hip_rj_gibbs.py's construction)
        rs = np.random.RandomState(c["seed"])
        p["chol"] = np.stack([np.diag(s) + np.tril(0.4 * s[:, None] * rs.randn(3, 3), -1) for s in p["scale"]])
        for b, Lc in zip(p["obr"], p["chol"]):
            b.cov = Lc @ Lc.T
    return p


def gibbs_oracle(p, seed, cls=None, **kw):
    from tests import rj_gibbs_move as rgm
    R, G = np.random.RandomState(500 + seed), np.random.RandomState(600 + seed)
    return (cls or rgm.GibbsOracle)(p["blocks"], p["obr"], p["x"], p["inds"], p["t"], p["y"], p["sigma"], R, G, p["betas"], record=True,
                                    schedule="none", like_fn=p["like_fn"], **kw)


def gibbs_block_facts(facts, r, inds):
    """fix_logp_gibbs's cases among one block's walkers: ``inf`` (no moved leaf, leaves in branches outside the block: -inf), ``zero``
    (no moved leaf, the walker's only leaves in non-member slots of the block's own branches: the stored 0.0 of DESIGN 4.13), ``empty``
    (no leaf at all)."""
    total = sum(v.sum(axis=-1) for v in inds.values())
    nomove = r["here"] == 0
    facts["inf"] += int((nomove & (r["total"] != 0)).sum())
    facts["zero"] += int((nomove & (r["total"] == 0) & (total != 0)).sum())
    facts["empty"] += int((total == 0).sum())
    facts["accepted"] += int(r["accepted"].sum())
    facts["decisions"] += int(r["accepted"].size)


def gibbs_accept_uniforms(seed, it, T_, W_, block, rung_begin=0):
    """Block ``block``'s accept uniform under hens_rj_step (hens_rj_gibbs.h: rj_gibbs_acc_key = rj_acc_key(RJ_MODE_MH, 0) | block << 19)."""
    from tests.production_draws import philox4x32_10, u01
    d = philox4x32_10(it & 0xFFFFFFFF, it >> 32, rm._wid(T_, W_, rung_begin), rm.PURPOSE_RJ_ACC | (1 << 8) | (block << 19), seed & 0xFFFFFFFF, seed >> 32)
    return u01(d[0], d[1])


def gibbs_unit_normals(seed, it, T_, W_, ncoord, block, rung_begin=0):
    """The unit normal of every record coordinate in block ``block`` [T, W, ncoord]: tests/production_draws.mh_normal_ideal's first value
    on words 0, 1 of the call keyed rj_normal_key(i) | block << 25 (rj_normal_key(i) = 12 | (i | 0x10000) << 8, tests/rj_mt_move.
    iteration_keys); the device's float32 units are within tests/production_draws.MH_NORMAL_E of it."""
    from tests.production_draws import mh_normal_ideal, philox4x32_10
    z = np.zeros((T_, W_, ncoord))
    for i in range(ncoord):
        d = philox4x32_10(it & 0xFFFFFFFF, it >> 32, rm._wid(T_, W_, rung_begin), PURPOSE_MH_NORMAL | ((i | 0x10000) << 8) | (block << 25),
                          seed & 0xFFFFFFFF, seed >> 32)
        z[:, :, i] = mh_normal_ideal(d[0], d[1])[0]
    return z


# ---- E: the data-point limits of the resident templates under k_rj_mt and k_rj_gibbs ------------------------------------------------------
# a lane keeps 2 chunks of 4 points, 64 lanes apart: point 256 is lane 0's first of chunk 1; 512 fills every lane; 513 has no resident
# templates (full evaluation).  pulse x 3 + sine x 2, multiple-try birth / death with K = 5 and one Gibbs block per branch.
POINTS = dict(kinds=("pulse", "sine"), nl_max=(3, 2), nl_min=(0, 0), T=2, W=9, K=5, iters=4, seed=4, sigma=3.0, schedule="iterate_branches")
POINTS_NDATA = (257, 512, 513)
RESIDENT_MAX = 512


def points_case(ndata):
    return rm.case(POINTS["kinds"], POINTS["T"], POINTS["W"], POINTS["K"], ndata, POINTS["nl_max"], POINTS["nl_min"], sigma=POINTS["sigma"],
                   seed=POINTS["seed"], nprop=0)


def points_oracle_class(*bases):
    """The multiple-try specification with the Gibbs-block in-model move (``bases``: replay classes in front of them)."""
    from tests import rj_gibbs_move as rgm

    class GibbsMT(*bases, rgm.GibbsOracle, rm.MTOracleRJSampler):
        pass
    return GibbsMT


# ---- D: periods past coordinate 64 (tests/rj_periodic.py) ------------------------------------------------------------------------------------
# pulses x 12 + sines x 12: the sine phases are record coordinates 38, 41 .. 71 - slots 0 .. 8 below 64, slots 9, 10, 11 at 65, 68, 71;
# lorentz + chirp of the same shape for the WIDE instantiation.  tests/rj_periodic.production_problem's seam start.
PERIODIC_NL = (12, 12)
PERIODIC_CASES = {
    "stretch": dict(kinds=("pulse", "sine"), nl=PERIODIC_NL, move="stretch", schedule="together"),
    "group": dict(kinds=("pulse", "sine"), nl=PERIODIC_NL, move="group", schedule="separate_branches"),
    "gibbs": dict(kinds=("pulse", "sine"), nl=PERIODIC_NL, move="gibbs", schedule="separate_branches"),
    "wide_stretch": dict(kinds=("lorentz", "chirp"), nl=PERIODIC_NL, move="stretch", schedule="separate_branches"),
}
PERIODIC_ITERS, PERIODIC_SEED = 6, 17


def periodic_problem(name):
    from tests import rj_periodic as rp
    p = rp.production_problem(PERIODIC_CASES[name], T=T, W=W, seed=2000 + sorted(PERIODIC_CASES).index(name))
    # the Gibbs table: one block per branch, then one block per sine slot
    p["setup"] = [b.name for b in p["obr"]] + [_slots(p["obr"][-1], [s]) for s in range(p["obr"][-1].nleaves_max)]
    return p


class SeamBySide:
    """tests/rj_periodic.SeamFacts and, beside it, the accepted seam crossings of ACTIVE periodic coordinates and the accepted walkers'
    DEAD periodic coordinates whose bits the proposal changed, by the side of record coordinate 64 they lie on (``low`` / ``high``,
    ``dead_low`` / ``dead_high``); a changed dead coordinate must hold x % period (``dead_ok``)."""

    def __init__(self, coord0):
        from tests import rj_periodic as rp
        self.base, self.coord0 = rp.SeamFacts(), dict(coord0)
        self.low = self.high = self.dead_low = self.dead_high = 0
        self.dead_ok = True

    def __getattr__(self, k):
        return getattr(self.base, k)

    def proposal(self, periods, x_old, raw, q, inds, keep):
        from tests import rj_periodic as rp
        self.base.proposal(periods, x_old, raw, q, inds, keep)
        keep = np.asarray(keep, dtype=bool)
        for name, per in periods.items():
            idx = np.flatnonzero(per > 0)
            if not idx.size:
                continue
            nl, nd = raw[name].shape[-2], len(per)
            high = (self.coord0[name] + np.arange(nl)[:, None] * nd + idx[None, :]) >= 64           # [nl, periodic parameters]
            act = np.asarray(inds[name], dtype=bool)[..., None]
            r = raw[name][..., idx]
            cr = act & ((r < 0.0) | (r >= per[idx])) & keep[..., None, None]
            self.low += int(cr[..., ~high].sum())
            self.high += int(cr[..., high].sum())
            qd, xd = q[name][..., idx], x_old[name][..., idx]
            ch = ~act & keep[..., None, None] & (rp.bits(qd) != rp.bits(xd))
            self.dead_low += int(ch[..., ~high].sum())
            self.dead_high += int(ch[..., high].sum())
            self.dead_ok = self.dead_ok and bool(np.array_equal(rp.bits(qd[ch]), rp.bits(rp.wrap(x_old[name], per)[..., idx][ch])))

    def line(self):
        return (f"accepted seam crossings below / from coordinate 64: {self.low} / {self.high}; dead phases rewritten below / from 64: "
                f"{self.dead_low} / {self.dead_high}; {self.base.as_dict()}")


# ---- C: the group stretch move (tests/rj_group_move.py; hens_rj_group.h) -----------------------------------------------------------------
# C1: records of 62 | 63 | 64 slots.  A walker's production call has a lane per key - slot s < nslots its pick, lane nslots zz's uniform,
# lane nslots + 1 the accept uniform: at 62 slots both come out of the one call (lanes 62, 63), at 63 the accept uniform moves to a
# second call's lane 0, at 64 zz's moves there too (lanes 0, 1).  The 62-slot control is ramp_across_64 without its last offset slot.
PURPOSE_RJ_GROUP, RJ_MODE_GROUP, RJ_GROUP_ZZ = 29, 4, 64
GROUP_KEY = {"offset": 0, "ramp": 0, "burst": 1, "pulse": 1, "sine": 1}      # the key parameter per leaf kind (a ramp's level, a centre, a frequency)
GROUP_RECORDS = {
    "slots_62": dict(model="ramp_across_64", kinds=("offset", "ramp"), nl_max=(30, 32), seed=1),
    "slots_63": dict(model="ramp_across_64", kinds=("offset", "ramp"), nl_max=(31, 32), seed=1),
    "slots_64": dict(model="four_branches_64_slots", kinds=("offset", "ramp", "burst", "pulse"), nl_max=(32, 16, 8, 8), seed=1),
}
GROUP_NFRIENDS, GROUP_UPDATE, GROUP_A = 5, 2, 2.0
GROUP_FORCED_ITERS, GROUP_REPLAY_ITERS, GROUP_REPLAY_SEED = 3, 4, 7


def group_draws(seed, it, T_, W_, nl_max, nf, rung_begin=0):
    """The specification's statement of the move's production draws (hens_rj_group.h: rj_group_lane_key): per branch picks [T, W, nl]
    - slot s of the RECORD (branch after branch): word 0 of the call keyed PURPOSE_RJ_GROUP | s << 8 through rj_pick(word, nf_b), 0 where
    the branch's table is empty -, zz's uniform u01(words 0, 1) of the call keyed PURPOSE_RJ_GROUP | 64 << 8, the accept uniform
    u01(words 0, 1) of the call keyed rj_acc_key(RJ_MODE_GROUP, 0).  Which lane of which call holds a value is the kernel's business."""
    from tests.production_draws import philox4x32_10, u01
    from tests.production_draws_rj import rj_pick
    wid = rm._wid(T_, W_, rung_begin)
    call = lambda key: philox4x32_10(it & 0xFFFFFFFF, it >> 32, wid, key, seed & 0xFFFFFFFF, seed >> 32)      # noqa: E731
    picks, s = [], 0
    for b, n in enumerate(nl_max):
        p = np.zeros((T_, W_, n), dtype=np.int64)
        for k in range(n):
            if nf[b] > 0:
                p[:, :, k] = rj_pick(call(PURPOSE_RJ_GROUP | (s << 8))[0], nf[b])
            s += 1
        picks.append(p)
    z, a = call(PURPOSE_RJ_GROUP | (RJ_GROUP_ZZ << 8)), call(rm.PURPOSE_RJ_ACC | (RJ_MODE_GROUP << 8))
    return picks, u01(z[0], z[1]), u01(a[0], a[1])


def _group_dict(brs, t, y, sigma, x, inds, T_, W_, kinds):
    return dict(obr=[b.to_oracle() for b in brs], dbr=[b.to_device() for b in brs], t=t, y=y, sigma=sigma, x=x, inds=inds, T=T_, W=W_,
                betas=0.35 ** np.arange(T_), key={b.name: GROUP_KEY[k] for b, k in zip(brs, kinds)}, like_fn=lk.like_fn(kinds), kinds=kinds)


def group_problem(name, W_=W):
    """A record of GROUP_RECORDS on its model's data and class start (62 slots: the offsets' last slot left out)."""
    from tests import leaf_kind_cases as cases
    r = GROUP_RECORDS[name]
    _, t, y, sigma = lr.problem(r["model"], NDATA, r["seed"])
    x, inds, _ = lr.start(r["model"], T, W_, r["seed"])
    brs = cases.branches_of(r["kinds"], r["nl_max"])
    x = {b.name: x[b.name][:, :, :b.nleaves_max].copy() for b in brs}
    inds = {b.name: inds[b.name][:, :, :b.nleaves_max].copy() for b in brs}
    return _group_dict(brs, t, y, sigma, x, inds, T, W_, r["kinds"])


# C2: the table's limits.  k_rj_group_gather walks the cold rung 256 walkers at a time (W > 256: a second pass on top of the first's
# count); k_rj_group_rank sorts by rank over 256-entry tiles, the stable order among equal keys decided by the entries' gather index
# across tiles.  (name: walkers, and for the one-branch tables the cold rung's entries and whether keys are made equal.)
TABLE_W = 257
TABLE_CASES = {"ramp_across_64_w300": dict(W=300)}
TABLE_CASES.update({f"pulse_{n}_entries": dict(W=TABLE_W, n=n, ties=False) for n in (255, 256, 257)})
TABLE_CASES.update({f"pulse_{n}_entries_equal_keys": dict(W=TABLE_W, n=n, ties=True) for n in (255, 256, 257)})
TIE_RUN = (250, 262)            # gather indices [250, 262) share one key: the run lies across gather entry 256 where there is one
TIE_APART = (3, 100)            # ... and these two carry it as well, far from the run
ZEROS = ((20, -0.0), (40, 0.0), (128, -0.0))      # keys -0.0 / +0.0 / -0.0 in this gather order: one key, +0.0, the rows keep their bits


def table_problem(name):
    from tests import leaf_kind_cases as cases
    c = TABLE_CASES[name]
    if "n" not in c:
        return group_problem("slots_63", c["W"])
    n, W_ = c["n"], c["W"]
    rs = np.random.RandomState(n + (1000 if c["ties"] else 0))
    brs = cases.branches_of(("pulse",), (2,))
    t = np.linspace(-1, 1, NDATA)
    y = cases.make_data(brs, t, lr.SIGMA[NDATA], rs)
    x, inds = cases.random_state(brs, T, W_, rs)
    cold = np.zeros(2 * W_, dtype=bool)
    cold[:n] = True
    rs.shuffle(cold)                                        # walkers with 0, 1 and 2 cold leaves: the scan adds all three
    inds["pulse"][0] = cold.reshape(W_, 2)
    if c["ties"]:
        ws, ss = np.where(inds["pulse"][0])                 # gather order: ascending (walker, slot)
        k = GROUP_KEY["pulse"]
        run = np.concatenate([np.array(TIE_APART), np.arange(TIE_RUN[0], min(TIE_RUN[1], n))])
        x["pulse"][0, ws[run], ss[run], k] = x["pulse"][0, ws[run[0]], ss[run[0]], k]
        for g, v in ZEROS:
            x["pulse"][0, ws[g], ss[g], k] = v
    return _group_dict(brs, t, y, lr.SIGMA[NDATA], x, inds, T, W_, ("pulse",))


def group_oracle(p, schedule, seed, iters_update=GROUP_UPDATE, cls=None, **kw):
    """The specification's sampler on a problem's start, ``check=True``: every window it computes is held to ``check_window``."""
    from tests import rj_group_move as rgr
    R, G = np.random.RandomState(300 + seed), np.random.RandomState(400 + seed)
    return (cls or rgr.GroupOracle)(GROUP_NFRIENDS, p["key"], iters_update, p["obr"], p["x"], p["inds"], p["t"], p["y"], p["sigma"], R, G,
                                    p["betas"], record=True, schedule=schedule, like_fn=p["like_fn"], group_a=GROUP_A, check=True, **kw)


# ---- F: a second model on one context---------------------------------------------------------------------------------------------------
SECOND_MODEL = dict(kinds=("pulse", "sine"), nl_max=(3, 2), T=2, W=9, ndata=(40, 600), iters=3, seed=5)
