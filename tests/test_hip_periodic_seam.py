"""Periodic parameters at the seam, on the device (-m gpu): ``periodic_diff`` / ``periodic_wrap`` (csrc/hens_kernels.h) at every site
they are pasted into, against exact arithmetic and the oracle, bit pattern for bit pattern.

Every other periodic test starts from continuous random positions, which reach a difference of exactly half a period, a remainder
of exactly zero or a proposal wrapped onto the period itself with probability zero.  tests/periodic_seam.py puts walkers there
(its docstring has the specification and the argument for the one place the device's select form and the reference's masked sum
differ, a zero's sign that the wrap absorbs); tests/test_periodic_seam.py holds that module to the real reference and sizes every
case below from the oracle alone at twice the coverage asked for here.

a. The teacher-forced matrix, site by site (``periodic_seam.FORCED_SITES``): T = 2, W = 56 walkers per period of the row (336: 168
   moving walkers a rung, two tiles and a ragged one; 280 for a row of 5) - every walker pair carrying ONE row of ONE period's matrix
   on ONE coordinate of that period, rotating over the row; each call hands every period a block of 56 rows, five calls walk the
   280 rows of every period's matrix, and that with every draw; neighbouring coordinates never share a period.  Dyadic periods and dyadic stretch factors (a = 4: u = 0, 1/4, 1/2; a = 9: u = 1/4) make the
   ties real and land proposals exactly on 0, on the period and on its multiples.  With accept uniforms of 0 the oracle keeps
   every proposal inside the box, so masks, positions and P are exact and L is held at ``tolerance_log.RTOL_L``.  Each site runs
   under the box [0, period] and again under [0, nextafter(period, 0)]: a proposal wrapped onto the period itself (NumPy has
   -1e-300 % 1.0 == 1.0) is kept in the first and refused in the second.
b. ``hens_step`` with its own draws from lattice starts {0, 1/8, ..., 7/8} period, replayed through the oracle
   (tests/replay_utils.py); every call uploads a fresh lattice at the current iteration counter, so ties meet several counters and
   adaptation states.  One case per launch path (``periodic_seam.LATTICE_CASES``), named by ``timing()``.
c. (A rank of the ladder pipeline from a lattice start is not here: tests/pipeline_worker.py builds its own start positions, and
   handing it others would change its protocol.)

Every test prints its coverage counts, taken from the ORACLE's intermediates.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import periodic_seam as ps
from tests import replay_utils as ru
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAST_WIDTHS = (8, 16, 32, 64, 128)


# ---- a. the teacher-forced matrix ---------------------------------------------------------------------------------------------------------
def _site_engine(site, prob, T, W):
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood, HostLikelihood
    s = ps.FORCED_SITES[site]
    like = HostLikelihood(prob.loglike, prob.D) if s.get("host") else GaussianLikelihood(prob.mu, prob.precision)
    eng = HipEnsemble(T, W, prob.D, like, prob.lo, prob.hi, a=4.0, pad_rows=s["pad"], prior_terms=getattr(prob, "spec", None))
    eng.set_periodic(prob.period)
    if site.startswith("fast") or site.startswith("mh_D32"):
        assert eng.RW in FAST_WIDTHS and eng.RW >= prob.D
    elif site.startswith("generic") and not s.get("terms"):
        assert eng.RW == prob.D and prob.D not in FAST_WIDTHS
    elif s.get("host"):
        # hens_propose_split has ONE kernel, k_propose, and refuses a context whose likelihood is not the host's (csrc/hens.hip)
        from eryn_amd import _lib
        assert int(like.kind) == _lib.LIKE_HOST and eng.RW == prob.D
    # (the prior-terms site: test_the_prior_terms_site_steps_in_the_generic_kernel)
    return eng


def _seam(a, call, moving):
    tt, kk = np.meshgrid(np.arange(call["d"].shape[0]), np.arange(call["d"].shape[1]), indexing="ij")
    return a[tt, moving(kk), call["d"]]


@pytest.mark.parametrize("site", sorted(ps.FORCED_SITES))
def test_seam_matrix_teacher_forced(site, monkeypatch):
    s = ps.FORCED_SITES[site]
    D, kind, T = s["D"], s.get("kind", "stretch"), 2
    cnt = ps.new_counts()
    ps.install(monkeypatch, cnt)
    refused, ncalls, worst = 0, 0, 0.0
    for shift in ps.SHIFTS:
        W = ps.forced_width(D, shift)
        for tight in (False, True):
            prob = ps.site_problem(site, shift, tight)
            eng = _site_engine(site, prob, T, W)
            for call in ps.forced_calls(D, shift, kind):
                what = f"{site} shift {shift} {'tight' if tight else 'loose'} box, call {ncalls}"
                state = ps.forced_state(call, prob)
                out, xo, Lo, Po = ps.forced_oracle(call, prob, state)
                assert out["keep"].all() or tight, what + ": a proposal left the loose box"
                refused += int((~out["keep"]).sum())
                eng.upload(*state)                        # (ends the red-blue move the last call left half done)
                eng.set_stretch_scale(call["a"])
                if s.get("host"):                         # k_propose: the proposals themselves
                    q, inbox = eng.propose_split(0, call["labels"], call["rint"], call["u_zz"])
                    assert ps.same_bits(q, out["q"]), what + f": {int((ps.bits(q) != ps.bits(out['q'])).sum())} proposals differ"
                    assert ps.same_bits(_seam(q, call, lambda k: k), ps.forced_reference(call)), what + ": not exact arithmetic's"
                    assert np.array_equal(inbox, out["keep"]), what + ": in-prior mask"
                    ncalls += 1
                    continue
                if kind == "mh":
                    keep = eng.mh_step(call["step"], np.zeros((T, W)))
                else:
                    keep = eng.stretch_split(0, call["labels"], call["rint"], call["u_zz"], np.zeros(call["d"].shape))
                xd, Ld, Pd, _ = eng.download()
                assert np.array_equal(keep, out["keep"]), what + f": accept mask differs in {int((keep != out['keep']).sum())} places"
                bad = ps.bits(xd) != ps.bits(xo)
                assert not bad.any(), what + f": positions differ at (t, w, d) {np.argwhere(bad)[:4].tolist()}: " \
                                             f"{xd[bad][:4]} for {xo[bad][:4]}"
                assert ps.same_bits(Pd, Po), what + ": log-prior"
                worst = max(worst, tol.check_logl(Ld, Lo, tol.RTOL_L, what))
                if kind == "stretch":                     # the kept rows' seam coordinates: exact arithmetic, not only the oracle
                    got, want = _seam(xd, call, lambda k: 2 * k), ps.forced_reference(call)
                    assert np.array_equal(ps.bits(got)[keep], ps.bits(want)[keep]), what + ": not exact arithmetic's"
                ncalls += 1
            eng.close()
    # (the oracle ran every call under both boxes: the counts are double the matrix's)
    ps.assert_counts(cnt, ps.FORCED_CLAIMS[kind], 2 * ps.LEAST, site)
    print(f"{site}: {ncalls} calls, {refused} proposals on a period refused by the tight box, max_rel_L {worst:.2e}")
    assert refused >= ps.LEAST


_WHICH = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests import periodic_seam as ps
from tests.test_hip_periodic_seam import _site_engine
site = "generic_D16_prior_terms"
prob = ps.site_problem(site, 0, False)
call = ps.forced_calls(16, 0)[0]
eng = _site_engine(site, prob, 2, ps.forced_width(16, 0))
with ps.prior_of(prob):
    eng.upload(*ps.forced_state(call, prob))
eng.stretch_split(0, call["labels"], call["rint"], call["u_zz"], np.zeros(call["d"].shape))
eng.close()
"""


def test_the_prior_terms_site_steps_in_the_generic_kernel():
    """HENS_PRIOR_LOG=1 in a child process (the library reads its switches once): with prior terms AND periods the half-step of the
    matrix's site goes to the generic k_stretch, not to k_stretch_prior, which has no periodic form"""
    r = subprocess.run([sys.executable, "-c", _WHICH, ROOT], env=dict(os.environ, HENS_PRIOR_LOG="1"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    kernels = {line.rsplit(": ", 1)[1] for line in r.stderr.splitlines() if line.startswith("hens: prior terms, D = 16")}
    assert kernels == {"k_stretch"}, f"launches under prior terms and periods went to {sorted(kernels)}:\n" + r.stderr[-1500:]


# ---- b. production stepping from the lattice ------------------------------------------------------------------------------------------------
def run_lattice_case(name, monkeypatch):
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    c = ps.LATTICE_CASES[name]
    T, W, D = c["T"], c["W"], c["D"]
    prob = ps.lattice_problem(c)
    cnt = ps.new_counts()
    ps.install(monkeypatch, cnt)
    eng = HipEnsemble(T, W, D, GaussianLikelihood(prob.mu, prob.precision), prob.lo, prob.hi, seed=c["seed"], **c["kw"])
    eng.set_periodic(prob.period)
    mh = ps.mh_proposal(prob, *c["mh"]) if c["mh"] else None
    if mh:
        eng.set_mh_proposal(*mh)
    if c["nsplits"] != 2:
        eng.set_nsplits(c["nsplits"])
    st, kinds, done = None, [], 0
    betas = orc.make_ladder(D, ntemps=T) if T > 1 else None
    for j, n in enumerate(c["calls"]):
        # a fresh lattice at the current iteration counter, adaptation time and ladder
        eng.upload(prob.lattice(T, W, c["seed"] + j), betas=betas)
        eng.eval_state()
        x, L, P, betas = eng.download()
        if st is None:
            st = ru.OracleState(x, L, P, betas)
        else:
            st.x, st.L, st.P, st.betas = x.copy(), L.copy(), P.copy(), None if betas is None else betas.copy()
        c0 = eng.counters()
        st.accepted, st.swaps_total, st.swaps_last = c0["accepted"].copy(), c0["swaps_total"].copy(), c0["swaps_last"].copy()
        if mh:
            st.mh_accepted = eng.mh_counters()["accepted"].copy()
        if T > 1:
            assert int(c0["adapt_time"]) == st.time == done, "the upload moved the adaptation time"
        it0 = eng.iteration()
        assert it0 == done, "the upload moved the iteration counter"
        eng.step(n)
        eng.synchronize()
        kinds += ru.replay(eng, st, it0, n, prob.loglike, prob.lo, prob.hi, mh=mh is not None, period=prob.period, nsplits=c["nsplits"])
        x, L, P, betas = eng.download()
        done += n
        what = f"{name} after {done} iterations"
        ru.assert_state_equal(st, x, L, P, betas, counters=eng.counters(), mh_counters=eng.mh_counters() if mh else None, what=what)
        assert ps.same_bits(x, st.x), what + ": a zero of the other sign among the positions"
        assert st.min_margin > 1e-12, "a decision sat on the knife edge; pick another seed for this case"
    assert "stretch" in kinds and (mh is None or "mh" in kinds)
    assert st.accepted.sum() + st.mh_accepted.sum() > 0 and (T == 1 or st.swaps_total.sum() > 0)
    ps.assert_counts(cnt, ps.LATTICE_CLAIMS, ps.LEAST, name)
    if mh:
        eng.set_mh_proposal(None, None, 0.0)
    eng.set_profiling(True)
    eng.step(2)
    tm = eng.timing()
    eng.close()
    path = (tm["n_stretch"], tm["n_pt"], tm["n_fused"])
    rep = tol.report()
    print(f"{name}: launches of two iterations (n_stretch, n_pt, n_fused) = {path}")
    print("max_rel_L %.3e values %d" % (max([v["max_rel_L"] for v in rep.values()] + [0.0]), sum(v["values"] for v in rep.values())))
    assert path == tuple(c["path"]), f"{name} stepped on another launch path: {path}"


@pytest.mark.parametrize("name", sorted(n for n, c in ps.LATTICE_CASES.items() if not c["env"]))
def test_production_stepping_from_the_lattice(name, monkeypatch):
    run_lattice_case(name, monkeypatch)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import pytest
from tests.test_hip_periodic_seam import run_lattice_case
mp = pytest.MonkeyPatch()
try:
    run_lattice_case(sys.argv[2], mp)
finally:
    mp.undo()
"""


@pytest.mark.parametrize("name", sorted(n for n, c in ps.LATTICE_CASES.items() if c["env"]))
def test_production_stepping_from_the_lattice_behind_a_switch(name):
    """the paths a switch selects, each in a fresh child process (the library reads its switches once): the one-launch iteration
    refused (HENS_NO_ITER=1: the two in-place launches at the one-launch shape), the three copying launches (HENS_NO_FUSED=1)"""
    from tests.test_hip_hetero_box import _child_env, _note_child
    c = ps.LATTICE_CASES[name]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name], env=_child_env(c["env"]), capture_output=True, text=True, timeout=300)
    _note_child(r, name)
