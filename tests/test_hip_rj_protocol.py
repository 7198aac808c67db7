"""The call protocol of the leaf-packing entry points (include/hipensemble.h, hens_rj_*): which call is refused in which state,
with which error code and text, and that a refused call leaves no trace - a context that continues after a refusal is compared
with a twin of the same seed that never made the refused calls (coordinates, leaf masks, log-probabilities, ladder, every counter
and the iteration counter, bit for bit).  Also: the counters the teacher-forced moves advance, and that a teacher-forced move
invalidates the resident templates hens_rj_step keeps across calls.

Small on purpose: 2 rungs x 24 walkers, a pulse branch of 2 leaves and a sine branch of 1 (9 record coordinates: 24 >= 2 x 9
walkers, so the red / blue stretch move runs without live_dangerously), 32 data points."""
import ctypes as C
import re

import numpy as np
import pytest

from eryn_amd import _lib
from eryn_amd._lib import check, f64, ptr

T, W, NDATA, SEED, SIGMA = 2, 24, 32, 11, 1.0
NAMES = ["gauss", "sine"]
NL = {"gauss": 2, "sine": 1}
BOX = {"gauss": [(2.5, 3.5), (-1.0, 1.0), (0.05, 0.25)], "sine": [(0.5, 1.5), (1.0, 5.0), (0.0, 2 * np.pi)]}
SCALE = np.full((2, 3), 1e-2) * [[1, 1, 0.1], [1, 1, 1]]
PENDING = "hens_rj_accept must follow hens_rj_propose"
HALF = "a half-step is pending"


def _problem():
    rs = np.random.RandomState(42)
    t = np.linspace(-1, 1, NDATA)
    y = 3.0 * np.exp(-((t + 0.2) ** 2) / (2 * 0.1 ** 2)) + 1.1 * np.sin(2 * np.pi * 2.5 * t + 1.0) + SIGMA * rs.randn(NDATA)
    x, inds = {}, {}
    for k in NAMES:
        lo, hi = np.array(BOX[k]).T
        x[k] = lo + rs.rand(T, W, NL[k], 3) * (hi - lo)
        inds[k] = rs.rand(T, W, NL[k]) < 0.5
    inds["gauss"][:, :, 0] = True                       # (every walker starts with a leaf)
    return t, y, x, inds


def template_like(x_list, t, y, sigma):
    """The template model as a user function in the reference's calling convention: the active leaves of one walker per branch."""
    pulses, sines = x_list
    tm = np.zeros_like(t)
    if pulses is not None:
        for a, b, c in np.atleast_2d(pulses):
            tm = tm + a * np.exp(-((t - b) ** 2) / (2 * c ** 2))
    if sines is not None:
        for a, b, c in np.atleast_2d(sines):
            tm = tm + a * np.sin(2 * np.pi * b * t + c)
    return -0.5 * np.sum(((tm - y) / sigma) ** 2)


def host_like():
    from eryn_amd.rj import CallableLikelihood
    t, y, _, _ = _problem()
    return CallableLikelihood(template_like, args=[t, y, SIGMA])


def make(scale=True, upload=True, like=None):
    from eryn_amd.moves.tempering import make_ladder
    from eryn_amd.rj import RJEngine, TemplateBranch
    t, y, x, inds = _problem()
    brs = [TemplateBranch("gauss", "pulse", BOX["gauss"], NL["gauss"]), TemplateBranch("sine", "sine", BOX["sine"], NL["sine"])]
    e = RJEngine(T, W, brs, t, y, SIGMA, seed=SEED)
    e.host_like = like
    if scale:
        e.set_mh_scale(SCALE)
    if upload:
        e.upload(x, inds, betas=make_ladder(9, ntemps=T))
        e.eval_state()
    return e


def snapshot(e):
    x, inds, L, P, betas = e.download()
    return dict(x=x, inds=inds, L=L, P=P, betas=betas, counters=e.counters(), iteration=e.iteration())


def assert_twins(a, b, counters=True):
    sa, sb = snapshot(a), snapshot(b)
    for k in sa["x"]:
        assert np.array_equal(sa["inds"][k], sb["inds"][k]), f"leaf masks of {k}"
        assert np.array_equal(sa["x"][k], sb["x"][k]), f"coordinates of {k}"
    for k in ("L", "P", "betas"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["iteration"] == sb["iteration"]
    if counters:
        for k, v in sa["counters"].items():
            assert np.array_equal(v, sb["counters"][k]), f"counter {k}"


def refused(exc, text):
    return pytest.raises(exc, match=re.escape(text))


# ---- draws of the teacher-forced moves (a pure function of the RandomState: twins get the same) ---------------------------
def mh_draws(rs, names=NAMES, nl=NL, nd=None):
    nd = nd or {k: 3 for k in names}
    return {k: 0.02 * rs.randn(T, W, nl[k], nd[k]) for k in names}, rs.rand(T, W)


def bd_draws(rs, inds_b, box):
    """change / leaf / birth / u_acc of one branch: a coin per walker, a birth into the first free slot, a death of the first
    active leaf, nothing where the leaf budget does not allow it."""
    n, nl = inds_b.sum(-1), inds_b.shape[-1]
    birth = rs.rand(T, W) < 0.5
    change = np.where(birth, np.where(n < nl, 1, 0), np.where(n > 0, -1, 0)).astype(np.int8)
    leaf = np.where(change > 0, np.argmin(inds_b, -1), np.argmax(inds_b, -1)).astype(np.int32)
    lo, hi = np.array(box).T
    return change, leaf, lo + rs.rand(T, W, len(box)) * (hi - lo), rs.rand(T, W)


def stretch_draws(rs, nb=2):
    labels = np.stack([rs.permutation(np.arange(W) % 2) for _ in range(T)]).astype(np.uint8)
    n0 = (W + 1) // 2
    halves = [(rs.randint(0, W - ns, size=(nb, T, ns)).astype(np.int64), rs.rand(T, ns), rs.rand(T, ns)) for ns in (n0, W - n0)]
    return labels, halves


# ---- hens_rj_propose / hens_rj_accept by hand (RJEngine._host_move runs the pair in one go) ---------------------------------
def propose(e, move, **d):
    d = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    dr = _lib.HensRjDraws(**{k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in d.items()})
    q, logp, moved = np.empty((T, W, e.RW)), np.empty((T, W)), np.empty((T, W), dtype=np.uint8)
    check(e.lib.hens_rj_propose(e.ctx, int(move), C.byref(dr), ptr(q), ptr(logp), ptr(moved)), e.ctx)
    return q, logp, moved


def accept(e, like, q, logp, moved):
    x, inds = e.unpack(q)
    logl = f64(like(x, inds, logp, [b.name for b in e.branches], only=moved.astype(bool)))
    keep = np.empty((T, W), dtype=np.uint8)
    check(e.lib.hens_rj_accept(e.ctx, ptr(logl), ptr(keep)), e.ctx)
    return keep.astype(bool)


def mh_args(e, draws):
    steps, u = draws
    return dict(step=f64(e.steps_to_records(steps)), u_acc=f64(u))


def stretch_args(split, labels, halves):
    rint, u_zz, u_acc = halves[split]
    return dict(split=split, labels=labels, rint=rint, u_zz=f64(u_zz), u_acc=f64(u_acc))


# ---- the protocol -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_accept_without_propose_is_refused():
    e, twin = make(), make()
    code = e.lib.hens_rj_accept(e.ctx, ptr(np.zeros((T, W))), None)
    assert code == _lib.ERR_STATE
    with refused(RuntimeError, PENDING):
        check(code, e.ctx)
    e.step(2)
    twin.step(2)
    assert_twins(e, twin)
    e.close(), twin.close()


@pytest.mark.gpu
def test_everything_is_refused_while_an_accept_is_pending():
    e, twin = make(), make()
    like = host_like()
    rs = np.random.RandomState(5)
    mh = mh_draws(rs)
    _, inds, _, _, _ = e.download()
    bd = bd_draws(rs, inds["gauss"], BOX["gauss"])
    both = [bd_draws(rs, inds[k], BOX[k]) for k in NAMES]
    labels, halves = stretch_draws(rs)
    pend = propose(e, _lib.RJ_MOVE_MH, **mh_args(e, mh))
    with refused(RuntimeError, PENDING):
        propose(e, _lib.RJ_MOVE_MH, **mh_args(e, mh))
    with refused(RuntimeError, PENDING):
        e.mh_step(*mh)
    with refused(RuntimeError, PENDING):
        e.bd_step(0, *bd)
    with refused(RuntimeError, PENDING):
        e.bd_all_step(np.stack([b[0] for b in both]), np.stack([b[1] for b in both]), [b[2] for b in both], bd[3])
    with refused(RuntimeError, PENDING):
        e.stretch_split(0, labels, *halves[0])
    with refused(RuntimeError, PENDING):
        e.step(1)
    assert e.lib.hens_rj_step(e.ctx, 1) == _lib.ERR_STATE
    keep = accept(e, like, *pend)
    keep_twin = accept(twin, like, *propose(twin, _lib.RJ_MOVE_MH, **mh_args(twin, mh)))
    assert np.array_equal(keep, keep_twin)
    assert_twins(e, twin)
    e.step(2)                                           # ... and the chain goes on as the twin's
    twin.step(2)
    assert_twins(e, twin)
    e.close(), twin.close()


@pytest.mark.gpu
def test_stretch_halves_run_in_order_on_the_device_path():
    e, twin = make(), make()
    rs = np.random.RandomState(6)
    mh = mh_draws(rs)
    _, inds, _, _, _ = e.download()
    bd = bd_draws(rs, inds["gauss"], BOX["gauss"])
    labels, halves = stretch_draws(rs)
    with refused(RuntimeError, "split calls must run 0, 1 in order (expected 0)"):
        e.stretch_split(1, labels, *halves[1])
    k0 = e.stretch_split(0, labels, *halves[0])
    with refused(RuntimeError, HALF):
        e.mh_step(*mh)
    with refused(RuntimeError, HALF):
        e.bd_step(0, *bd)
    with refused(RuntimeError, HALF):
        e.step(1)
    with refused(RuntimeError, HALF):                   # (split 0 again: the readiness check comes before the order check, so
        e.stretch_split(0, labels, *halves[0])          #  "... in order (expected 1)" is never the text a caller sees)
    k1 = e.stretch_split(1, labels, *halves[1])
    t0 = twin.stretch_split(0, labels, *halves[0])
    t1 = twin.stretch_split(1, labels, *halves[1])
    assert np.array_equal(k0, t0) and np.array_equal(k1, t1)
    assert_twins(e, twin)
    e.close(), twin.close()


@pytest.mark.gpu
def test_stretch_halves_run_in_order_on_the_host_callable_path():
    like = host_like()
    e, twin = make(like=like), make(like=like)
    e.host_like = None                                  # (the refused calls below are the device path's entry points)
    rs = np.random.RandomState(7)
    mh = mh_draws(rs)
    _, inds, _, _, _ = e.download()
    bd = bd_draws(rs, inds["gauss"], BOX["gauss"])
    labels, halves = stretch_draws(rs)
    with refused(RuntimeError, "split calls must run 0, 1 in order (expected 0)"):
        propose(e, _lib.RJ_MOVE_STRETCH, **stretch_args(1, labels, halves))
    k0 = accept(e, like, *propose(e, _lib.RJ_MOVE_STRETCH, **stretch_args(0, labels, halves)))
    with refused(RuntimeError, HALF):
        e.mh_step(*mh)
    with refused(RuntimeError, HALF):
        e.bd_step(0, *bd)
    with refused(RuntimeError, HALF):
        e.step(1)
    with refused(RuntimeError, HALF):
        propose(e, _lib.RJ_MOVE_MH, **mh_args(e, mh))
    with refused(RuntimeError, HALF):                   # (split 0 again: as on the device path)
        propose(e, _lib.RJ_MOVE_STRETCH, **stretch_args(0, labels, halves))
    k1 = accept(e, like, *propose(e, _lib.RJ_MOVE_STRETCH, **stretch_args(1, labels, halves)))
    t0 = accept(twin, like, *propose(twin, _lib.RJ_MOVE_STRETCH, **stretch_args(0, labels, halves)))
    t1 = accept(twin, like, *propose(twin, _lib.RJ_MOVE_STRETCH, **stretch_args(1, labels, halves)))
    assert np.array_equal(k0, t0) and np.array_equal(k1, t1)
    assert k0.sum() + k1.sum() > 0
    assert_twins(e, twin)
    e.close(), twin.close()


@pytest.mark.gpu
def test_bad_move_code_is_refused_and_nothing_stays_pending():
    like = host_like()
    e, twin = make(), make()
    mh = mh_draws(np.random.RandomState(8))
    with refused(ValueError, "move must be HENS_RJ_MOVE_MH, _BD, _BD_ALL or _STRETCH"):
        propose(e, 7, **mh_args(e, mh))
    keep = accept(e, like, *propose(e, _lib.RJ_MOVE_MH, **mh_args(e, mh)))
    keep_twin = accept(twin, like, *propose(twin, _lib.RJ_MOVE_MH, **mh_args(twin, mh)))
    assert np.array_equal(keep, keep_twin)
    assert_twins(e, twin)
    e.close(), twin.close()


@pytest.mark.gpu
def test_model_without_a_device_likelihood_steps_with_propose_and_accept_only():
    from eryn_amd.rj import CallableLikelihood, LeafBranch, RJEngine
    t, y, _, _ = _problem()

    def ramps_and_offsets(x_list, t, y, sigma):
        ramps, offsets = x_list
        tm = np.zeros_like(t)
        if ramps is not None:
            for a, b in np.atleast_2d(ramps):
                tm = tm + (a + b * t)
        if offsets is not None:
            for (a,) in np.asarray(offsets).reshape(-1, 1):
                tm = tm + a
        return -0.5 * np.sum(((tm - y) / sigma) ** 2)

    names, nl, nd = ["ramp", "offset"], {"ramp": 2, "offset": 3}, {"ramp": 2, "offset": 1}
    box = {"ramp": [(0.0, 1.0), (0.0, 2.0)], "offset": [(-1.0, 1.0)]}

    def fresh():
        rs = np.random.RandomState(9)
        e = RJEngine(T, W, [LeafBranch(k, box[k], nl[k]) for k in names], None, None, SIGMA, seed=SEED)
        e.host_like = CallableLikelihood(ramps_and_offsets, args=[t, y, SIGMA])
        x, inds = {}, {}
        for k in names:
            lo, hi = np.array(box[k]).T
            x[k] = lo + rs.rand(T, W, nl[k], nd[k]) * (hi - lo)
            inds[k] = rs.rand(T, W, nl[k]) < 0.5
        e.upload(x, inds, betas=np.array([1.0, 0.5]))
        e.eval_state()
        return e

    e, twin = fresh(), fresh()
    text = "no device likelihood (hens_rj_set_model_general)"
    with refused(RuntimeError, text):
        e.step(1)
    steps, u = mh_draws(np.random.RandomState(10), names, nl, nd)
    st, keep = f64(e.steps_to_records(steps)), np.empty((T, W), dtype=np.uint8)
    code = e.lib.hens_rj_mh_step(e.ctx, ptr(st), ptr(f64(u)), ptr(keep))
    assert code == _lib.ERR_STATE
    with refused(RuntimeError, text):
        check(code, e.ctx)
    k = e.mh_step(steps, u)                             # (host_like is set: hens_rj_propose / hens_rj_accept)
    kt = twin.mh_step(steps, u)
    assert k.shape == (T, W) and k.any() and np.array_equal(k, kt)
    assert_twins(e, twin)
    assert e.counters()["num_mh"] == 1
    e.close(), twin.close()


@pytest.mark.gpu
def test_step_without_a_step_scale_is_refused():
    e = make(scale=False)
    with refused(RuntimeError, "in-model step scale not set"):
        e.step(1)
    assert e.lib.hens_rj_step(e.ctx, 1) == _lib.ERR_STATE
    e.close()


@pytest.mark.gpu
def test_leaf_packing_calls_on_a_gaussian_context_are_refused():
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    D = 4
    eng = HipEnsemble(T, W, D, GaussianLikelihood(np.zeros(D), np.eye(D)), -5.0, 5.0, seed=SEED)
    eng.upload(np.random.RandomState(1).uniform(-1, 1, size=(T, W, D)), betas=np.array([1.0, 0.5]))
    eng.eval_state()
    text = "needs a context created with HENS_LIKE_TEMPLATE"
    lib, ctx = eng.lib, eng.ctx
    buf, keep = np.zeros((T, W, 16)), np.zeros((T, W), dtype=np.uint8)
    dr = _lib.HensRjDraws(step=buf.ctypes.data, u_acc=buf.ctypes.data)
    for code in (lib.hens_rj_step(ctx, 1), lib.hens_rj_mh_step(ctx, ptr(buf), ptr(buf), ptr(keep)),
                 lib.hens_rj_propose(ctx, _lib.RJ_MOVE_MH, C.byref(dr), ptr(buf), ptr(buf), ptr(keep)),
                 lib.hens_rj_set_schedule(ctx, 0)):
        assert code == _lib.ERR_STATE
        with refused(RuntimeError, text):
            check(code, ctx)
    eng.close()


@pytest.mark.gpu
def test_counters_of_the_teacher_forced_moves():
    e = make()
    rs = np.random.RandomState(12)

    def counts():
        c = e.counters()
        return c["num_mh"], c["num_bd"], e.iteration(), c["accepted_bd"]

    def inds_now():
        return e.download()[1]

    assert counts()[:3] == (0, 0, 0)
    e.mh_step(*mh_draws(rs))
    assert counts()[:3] == (1, 0, 0)                    # (a tempered ladder: the PT sweep behind the move closes the iteration)
    e.bd_step(1, *bd_draws(rs, inds_now()["sine"], BOX["sine"]))
    assert counts()[:3] == (1, 1, 0)
    both = [bd_draws(rs, inds_now()[k], BOX[k]) for k in NAMES]
    e.bd_all_step(np.stack([b[0] for b in both]), np.stack([b[1] for b in both]), [b[2] for b in both], both[0][3])
    assert counts()[:3] == (1, 2, 0)
    labels, halves = stretch_draws(rs)
    e.stretch_split(0, labels, *halves[0])
    assert counts()[:3] == (1, 2, 0)                    # (one MOVE: counted with its second half)
    e.stretch_split(1, labels, *halves[1])
    assert counts()[:3] == (2, 2, 0)
    # "iterate_branches": ONE move walks through the branches - counted, with its accepts, at the last one
    e.set_schedule("iterate_branches")
    before = counts()
    k0 = e.bd_step(0, *bd_draws(rs, inds_now()["gauss"], BOX["gauss"]))
    mid = counts()
    assert mid[:3] == before[:3] and np.array_equal(mid[3], before[3]) and k0.shape == (T, W)
    k1 = e.bd_step(1, *bd_draws(rs, inds_now()["sine"], BOX["sine"]))
    after = counts()
    assert after[:3] == (2, 3, 0) and after[3].sum() == before[3].sum() + k1.sum()
    e.step(3)
    assert counts()[:3] == (5, 6, 3)
    e.close()


@pytest.mark.gpu
def test_teacher_forced_moves_invalidate_the_resident_templates():
    """hens_rj_step keeps every walker's template resident across calls; a teacher-forced move changes the walkers behind its
    back.  A context that goes on stepping after such a move must land where a FRESH context lands that was handed the downloaded
    state (and has no templates to be stale): bit for bit, after an in-model move and after a birth / death move."""
    def reseated(e):
        x, inds, L, P, betas = e.download()
        it, at = e.iteration(), e.counters()["adapt_time"]
        e.close()
        f = make(upload=False)
        f.upload(x, inds, L, P, betas)
        f.set_iteration(it)
        f.set_adapt_time(at)
        return f

    a, b = make(), make()
    rs = np.random.RandomState(13)
    mh = mh_draws(rs)
    assert np.array_equal(a.mh_step(*mh), b.mh_step(*mh))
    b = reseated(b)
    a.step(3)
    b.step(3)
    assert_twins(a, b, counters=False)
    bd = bd_draws(rs, a.download()[1]["gauss"], BOX["gauss"])
    ka, kb = a.bd_step(0, *bd), b.bd_step(0, *bd)
    assert np.array_equal(ka, kb)
    b = reseated(b)
    a.step(3)
    b.step(3)
    assert_twins(a, b, counters=False)
    assert a.iteration() == 6
    a.close(), b.close()
