"""The specification of Gibbs parameter blocks (host only, NumPy): what include/hipensemble.h's hens_set_gibbs / hens_gibbs_select
and the block loop of hens_step compute, composed of the oracle's ``stretch_split`` / ``mh_step`` / ``pt_sweep`` /
``adapt_ladder`` (imported, not edited) around the mask.

One block of one move (move.py:113-221 under red_blue.py:119-333 / mh.py:79-193; one branch, nleaves_max == 1), mask m with n_b
true coordinates: the move proposes as usual, the old values go back in every coordinate outside the block (move.py:321-324),
prior and likelihood see the whole row, the stretch move's factor is (n_b - 1) log zz (stretch.py:55-72).

How the oracle is composed.  Both proposals are coordinate-wise - q_d = c_d - (c_d - s_d) zz, q_d = s_d + step_d - so the block's
proposal IS the oracle's move on the sub-vectors x[..., m] (its factor then reads (n_b - 1) log zz by itself, and a one-coordinate
block's is exactly 0), provided the oracle's prior and likelihood are shown the whole row.  ``_whole_rows`` does that: for the call's
duration ``oracle.box_log_prior`` is a closure that puts every proposed sub-vector back into its walker's old row - the moving
walkers in the order the oracle enumerates them - evaluates the case's prior there and remembers which rows were inside; the
likelihood closure rebuilds the same rows for the rows the oracle hands it (those inside).  A frozen coordinate is therefore the
old row's bits: it is never touched by arithmetic (x + 0.0 would turn -0.0 into +0.0).

The draws of the production path.  Block b of iteration ``it`` draws from the functions a context without a table uses
(tests/production_draws.py) with the block in the purpose word of the Philox counter: ``PURPOSE_STRETCH | b << 8`` (complement
index, u_zz, accept uniform; one call per split position), ``PURPOSE_MH_ACC | b << 8``, ``PURPOSE_MH_NORMAL | pair << 8 | b << 16``
(the coordinate pair already sits at bit 8).  Block 0's words are the words without a table.  The split labels and both position
lists (``own``), the move choice and the PT draws are the iteration's.

Books.  The device counts a walker once per accepted block proposal and num_proposals once per block (``BlockBooks``).  The
reference's books differ for the red-blue move - ``accepted`` is the running OR over the blocks so far, added after every block
(red_blue.py:306-327) - and its MH move returns the last block's mask (``replay_fixture``).
"""
import contextlib
import os

import numpy as np

from oracle import eryn_oracle as orc
from tests import prior_terms as pt
from tests import production_draws as pd
from tests import replay_utils as ru
from tests import rj_prior_terms as rpt

PURPOSE_STRETCH, PURPOSE_MH_ACC, PURPOSE_MH_NORMAL = pd.PURPOSE_STRETCH, pd.PURPOSE_MH_ACC, pd.PURPOSE_MH_NORMAL


# ---- the block draw words ----------------------------------------------------------------------------------------------------------------
def stretch_word(b):
    return PURPOSE_STRETCH | (b << 8)


def mh_acc_word(b):
    return PURPOSE_MH_ACC | (b << 8)


def mh_normal_word(pair, b):
    return PURPOSE_MH_NORMAL | (pair << 8) | (b << 16)


def block_plan(seed, it, T, W, cb, b):
    """own, cw, u_zz, u_acc [T, W] by split position of block ``b``: the iteration's position lists (tests/production_draws.plan),
    the complement index and the two uniforms from the block's word (csrc/hens_kernels.h: k_plan_block)."""
    base = pd.plan(seed, it, T, W, cb)
    if b == 0:
        return base
    N0 = (W + 1) // 2
    w = np.arange(W)
    s0 = w < N0
    own, cw, uz, ua = base["own"], np.empty((T, W), dtype=np.int64), np.empty((T, W)), np.empty((T, W))
    for t in range(T):
        d = pd.philox4x32_10(it & 0xFFFFFFFF, it >> 32, t * W + w, stretch_word(b), seed & 0xFFFFFFFF, seed >> 32)
        uz[t], ua[t] = pd.u01(d[0], d[1]), pd.u01(d[2], d[3])
        r22 = ((d[1].astype(np.uint64) & np.uint64(0x7FF)) << np.uint64(11)) | (d[3].astype(np.uint64) & np.uint64(0x7FF))
        r = ((r22 * np.where(s0, W - N0, N0).astype(np.uint64)) >> np.uint64(22)).astype(np.int64)
        cw[t] = own[t][np.where(s0, N0, 0) + r]
    return dict(own=own, cw=cw, u_zz=uz, u_acc=ua)


def mh_block_draws(seed, it, T, W, RW, b, rung_begin=0):
    """(z [T, W, RW] the standard normals in float64 - the device's lie within tests/production_draws.MH_NORMAL_E of them - and
    u [T, W] the accept uniforms) of block ``b`` of a Gaussian-move iteration."""
    z, u = np.empty((T, W, RW)), np.empty((T, W))
    for t in range(T):
        c2, c3, half = pd.mh_normal_address(rung_begin + t, W, RW)
        d = pd._call(seed, it, c2, c3 | (b << 16))
        zx, zy = pd.mh_normal_ideal(np.where(half == 1, d[2], d[0]), np.where(half == 1, d[3], d[1]))
        z[t, :, 0::2] = zx
        z[t, :, 1::2] = zy[:, :RW // 2]
        du = pd._call(seed, it, (rung_begin + t) * W + np.arange(W), mh_acc_word(b))
        u[t] = pd.u01(du[0], du[1])
    return z, u


# ---- one block of one move, on the oracle --------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _whole_rows(rows, mask, prior, loglike):
    """``rows`` [N, D]: the moving walkers' old rows in the oracle's order.  Yields the likelihood closure; while open, the oracle's
    ``box_log_prior`` evaluates ``prior`` (a tests/prior_terms specification) on the whole rows."""
    seen = {}

    def whole(q_sub, sel):
        full = rows[sel].copy()
        full[:, mask] = q_sub
        return full

    def box_log_prior(q_sub, lo, hi):
        logp = pt.log_prior(prior, whole(q_sub, slice(None)))
        seen["valid"] = np.flatnonzero(~np.isinf(logp))
        return logp

    def like(q_sub_valid):
        assert q_sub_valid.shape[0] == seen["valid"].size
        return loglike(whole(q_sub_valid, seen["valid"]))

    saved = orc.box_log_prior
    orc.box_log_prior = box_log_prior
    try:
        yield like
    finally:
        orc.box_log_prior = saved


def stretch_block_split(x, L, P, betas, labels, split, rint, u_zz, u_acc, a, mask, prior, loglike):
    """One red-blue half-step of a block; mutates x, L, P.  Returns the oracle's dict (q: the proposed sub-vectors) with ``S`` and
    ``logp_whole`` / ``lnpdiff`` of the whole-row proposals."""
    T, W, D = x.shape
    mask = np.asarray(mask, dtype=bool)
    S, _ = orc.split_index_lists(labels, split)
    tt = np.arange(T)[:, None]
    xs = np.ascontiguousarray(x[..., mask])
    lo, hi = prior["lo"][mask], prior["hi"][mask]
    with _whole_rows(x[tt, S].reshape(-1, D), mask, prior, loglike) as like:
        out = orc.stretch_split(xs, L, P, betas, labels, split, rint, u_zz, u_acc, a, lo, hi, like)
    x[..., mask] = xs
    return out


def mh_block(x, L, P, betas, step, u_acc, mask, prior, loglike):
    """One full-ensemble Gaussian proposal of a block (``step`` [T, W, D]: drawn for every coordinate, mh.py:113-124); mutates x, L, P."""
    T, W, D = x.shape
    mask = np.asarray(mask, dtype=bool)
    xs = np.ascontiguousarray(x[..., mask])
    with _whole_rows(x.reshape(-1, D).copy(), mask, prior, loglike) as like:
        out = orc.mh_step(xs, L, P, betas, np.ascontiguousarray(np.asarray(step).reshape(T, W, D)[..., mask]), u_acc,
                          prior["lo"][mask], prior["hi"][mask], like)
    x[..., mask] = xs
    return out


class BlockBooks:
    """The device's books and the coverage the GPU tests assert, counted from the specification's side: per move, block and rung
    the accepted and the rejected proposals; the proposals outside the prior's support; knife-edge decisions."""

    def __init__(self, T, W, nb_stretch, nb_mh):
        self.accepted, self.mh_accepted = np.zeros((T, W)), np.zeros((T, W))
        self.num_proposals = self.num_proposals_mh = 0
        self.acc = {"stretch": np.zeros((max(nb_stretch, 1), T), dtype=int), "mh": np.zeros((max(nb_mh, 1), T), dtype=int)}
        self.rej = {k: np.zeros_like(v) for k, v in self.acc.items()}
        self.outside = self.knives = 0
        self.min_margin = np.inf

    def add(self, move, b, keep, out, logu, walkers=None):
        from tests.parity_utils import knife_edge
        self.acc[move][b] += keep.sum(axis=1)
        self.rej[move][b] += (~keep).sum(axis=1)
        self.outside += int(np.isinf(out["logp"]).sum())
        self.knives += int(knife_edge(out["lnpdiff"], logu).sum())
        ru._margin(self, out["lnpdiff"], logu)
        tgt = self.accepted if move == "stretch" else self.mh_accepted
        if walkers is None:
            tgt += keep
        else:
            tgt[np.arange(keep.shape[0])[:, None], walkers] += keep


def stretch_iteration(st, books, masks, refs, a, prior, loglike):
    """The stretch move of one iteration: block after block, ``refs[b]`` the block's draws in the reference's terms
    (tests/replay_utils.draws_to_reference: one labelling, the block's rint / u_zz / u_acc)."""
    for b, mask in enumerate(masks):
        for sp in (0, 1):
            ref = refs[b]
            out = stretch_block_split(st.x, st.L, st.P, st.betas, refs[0]["labels"], sp, ref[f"rint{sp}"], ref[f"u_zz{sp}"], ref[f"u_acc{sp}"],
                                      a, mask, prior, loglike)
            with np.errstate(divide="ignore"):
                books.add("stretch", b, out["keep"], out, np.log(ref[f"u_acc{sp}"]), walkers=out["S"])
        books.num_proposals += 1


def mh_iteration(st, books, masks, steps, us, prior, loglike):
    for b, mask in enumerate(masks):
        out = mh_block(st.x, st.L, st.P, st.betas, steps[b], us[b], mask, prior, loglike)
        with np.errstate(divide="ignore"):
            books.add("mh", b, out["keep"], out, np.log(us[b]))
        books.num_proposals_mh += 1


def pt_tail(st, ref):
    """The ONE cascade and ladder adaptation behind the last block (tests/dist_move.pt_tail)."""
    from tests.dist_move import pt_tail as tail
    tail(st, ref)


def assert_coverage(books, what=""):
    """In every block and rung both an accepted and a rejected proposal, at least one proposal outside the support, no knife edge."""
    print(f"{what}: accepted / rejected per (block, rung): stretch {books.acc['stretch'].tolist()} / {books.rej['stretch'].tolist()}, "
          f"mh {books.acc['mh'].tolist()} / {books.rej['mh'].tolist()}; outside {books.outside}; closest margin {books.min_margin:.2e}")
    for move in ("stretch", "mh"):
        if books.acc[move].sum() + books.rej[move].sum() == 0:
            continue
        assert (books.acc[move] > 0).all(), f"{what}: a (block, rung) of the {move} move without an accepted proposal"
        assert (books.rej[move] > 0).all(), f"{what}: a (block, rung) of the {move} move without a rejected proposal"
    assert books.outside > 0, f"{what}: no proposal outside the prior's support"
    assert books.knives == 0, f"{what}: {books.knives} decisions on the knife edge"


# ---- the GPU cases -----------------------------------------------------------------------------------------------------------------------
def _mask(D, coords):
    m = np.zeros(D, dtype=bool)
    m[list(coords)] = True
    return m


def case(T, W, D, like, prior, stretch, mh, weight=0.5, iters=6, seed=2024):
    return dict(T=T, W=W, D=D, like=like, prior=prior, stretch=[_mask(D, c) for c in stretch], mh=[_mask(D, c) for c in mh],
                weight=weight, iters=iters, seed=seed)


# the issue's table: the smallest shapes at which the kernel can still go wrong
CASES = {
    # D = 5 padded to 8 (pads inert, uncounted in n_b), a one-coordinate block (factor exactly 0), halves of 35: a partial tile
    "3x70x5_diag_terms": case(3, 70, 5, "diag", "terms", [(0, 1), (2,), (3, 4)], [(0, 1), (2,), (3, 4)]),
    # odd W (66 | 65), even / odd coordinates: every lane's pair half frozen; the dense likelihood on the matrix pipe
    "2x131x32_dense_box": case(2, 131, 32, "dense", "box", [range(0, 32, 2), range(1, 32, 2)], [range(0, 32, 2), range(1, 32, 2)]),
    # eight waves, the largest LDS
    "2x130x128_rosen_box": case(2, 130, 128, "rosen", "box", [range(0, 64), range(64, 128), (127,)], [range(0, 64), range(64, 128), (127,)]),
    # a log-uniform coordinate frozen in one block and moving in another (tests/prior_terms.PriorProblem: 2 is log-uniform at every D),
    # overlapping blocks, coordinate 63 in none
    "3x40x64_dense_terms": case(3, 40, 64, "dense", "terms", [range(0, 40), range(30, 63)], [range(2, 34), range(0, 3), range(20, 63)]),
}
NEVER_MOVES = {"3x40x64_dense_terms": 63}


def case_problem(c):
    from tests.dist_move import DistProblem
    return DistProblem(c["D"], c["like"], c["prior"], "box")


def mh_scale(prob):
    """The Gaussian move's isotropic standard deviation on the problem's scales."""
    return 0.25 * float(prob.sig.min())


def free_run(c, seed=None):
    """The case on the specification alone with the production draws of its seed - the CPU sizing: -> (books, problem, x0, x)."""
    seed = c["seed"] if seed is None else seed
    prob = case_problem(c)
    T, W, D = c["T"], c["W"], c["D"]
    RW = next(w for w in (8, 16, 32, 64, 128) if w >= D) if c["like"] != "rosen" else D
    x = prob.x0(T, W).copy()
    P = pt.log_prior(prob.prior, x.reshape(-1, D)).reshape(T, W)
    assert np.isfinite(P).all(), "a start outside the prior's support"
    L = prob.loglike(x.reshape(-1, D)).reshape(T, W)
    st = ru.OracleState(x, L, P, orc.make_ladder(D, ntemps=T))
    books = BlockBooks(T, W, len(c["stretch"]), len(c["mh"]))
    cb = pd.label_cb(T, W)
    for it in range(c["iters"]):
        slot, u_swap = pd.pt_draws(seed, it, T, W)
        if pd.is_mh(seed, it, c["weight"]):
            zs = [mh_block_draws(seed, it, T, W, RW, b) for b in range(len(c["mh"]))]
            mh_iteration(st, books, c["mh"], [mh_scale(prob) * z[..., :D] for z, _ in zs], [u for _, u in zs], prob.prior, prob.loglike)
            ref = ru.draws_to_reference(dict(block_plan(seed, it, T, W, cb, 0), pt_slot=slot, u_swap=u_swap), T, W)
        else:
            refs = [ru.draws_to_reference(dict(block_plan(seed, it, T, W, cb, b), pt_slot=slot, u_swap=u_swap), T, W) for b in range(len(c["stretch"]))]
            stretch_iteration(st, books, c["stretch"], refs, 2.0, prob.prior, prob.loglike)
            ref = refs[0]
        pt_tail(st, ref)
    return books, prob, prob.x0(T, W), st.x


# ---- the fixtures from the real reference (tests/golden/make_golden_gibbs.py -> tests/golden/gibbs/) ------------------------------------------
FIXTURES = ["g1_stretch_blocks", "g2_gauss_blocks", "g3_mix_overlap", "g4_stretch_terms"]


def load_fixture(name):
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gibbs", name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def fixture_prior(fx):
    return pt.make_spec(rpt.fixture_entries(fx["prior_kind"], fx["prior_p0"], fx["prior_p1"]))


def fixture_loglike(fx):
    mu, invcov = fx["mu"], fx["invcov"]
    return lambda x: orc.gaussian_log_like(x, mu, invcov)


def fixture_gauss_step(fx, it, b):
    """The step of block b of Gaussian iteration ``it``: sqrt(cov) randn (gaussian.py:166-167), [T, W, D]."""
    T, W, D = int(fx["T"]), int(fx["W"]), int(fx["D"])
    return (1.0 * np.sqrt(float(fx["cov"])) * fx[f"it{it}_b{b}_z"]).reshape(T, W, D)


def replay_fixture(fx):
    """The fixture's chain on the specification with the reference's books: yields per iteration (x, L, P after the move, the mask
    propose() returns, x, L, P, betas after the sweep); returns through ``books`` the moves' accepted / num_proposals."""
    T, W, D = int(fx["T"]), int(fx["W"]), int(fx["D"])
    prior, loglike = fixture_prior(fx), fixture_loglike(fx)
    st = ru.OracleState(fx["x0"], fx["L0"], fx["P0"], fx["betas0"])
    books = dict(accepted_stretch=np.zeros((T, W)), accepted_gauss=np.zeros((T, W)), num_proposals_stretch=0, num_proposals_gauss=0)
    tt = np.arange(T)[:, None]
    for it in range(int(fx["nsteps"])):
        pre = f"it{it}_"
        if int(fx[pre + "kind"]):
            ret = np.zeros((T, W), dtype=bool)
            for b, mask in enumerate(fx["masks_gauss"]):
                out = mh_block(st.x, st.L, st.P, st.betas, fixture_gauss_step(fx, it, b), fx[pre + f"b{b}_uacc"], mask, prior, loglike)
                ret = out["keep"]                                           # mh.py:171,193: the last block's
                books["accepted_gauss"] += out["keep"]                      # mh.py:186
                books["num_proposals_gauss"] += 1
        else:
            ret = np.zeros((T, W), dtype=bool)
            for b, mask in enumerate(fx["masks_stretch"]):
                for sp in (0, 1):
                    out = stretch_block_split(st.x, st.L, st.P, st.betas, fx[pre + "labels"], sp, fx[pre + f"b{b}_rint{sp}"], fx[pre + f"b{b}_uzz{sp}"],
                                              fx[pre + f"b{b}_uacc{sp}"], float(fx["a"]), mask, prior, loglike)
                    ret[tt, out["S"]] |= out["keep"]                        # red_blue.py:306-308: the running OR
                books["accepted_stretch"] += ret                            # red_blue.py:326-327: after EVERY block
                books["num_proposals_stretch"] += 1
        move = (st.x.copy(), st.L.copy(), st.P.copy(), ret)
        _, sw = orc.pt_sweep(st.x, st.L, st.P, st.betas, fx[pre + "iperm"], fx[pre + "i1perm"], fx[pre + "u_swap"])
        st.betas = orc.adapt_ladder(st.betas, sw, W, st.time)
        st.time += 1
        yield it, move, (st.x.copy(), st.L.copy(), st.P.copy(), st.betas.copy(), sw), books
