"""The leaf-packing models at the record's limits (32 leaves per branch, 64 slots, 4 branches, 128 record doubles), their starts and
the coverage counters of tests/test_limit_records.py (no GPU) and tests/test_hip_limit_records.py.  Host only, NumPy.

A record is ``ncoord`` coordinates - branch b's slots from ``off[b]``, slot s of width nd at ``off[b] + s nd`` - then one mask double
per branch; RW = ncoord + nbranches rounded up to even.  k_rj gives coordinate i to lane i & 63 of pass i >> 6, so what matters is where
a slot sits relative to coordinate 64.  Every row states its arithmetic; tests/test_limit_records.py holds it to RJEngine's own.

  four_branches_64_slots  offset x 32, ramp x 16, burst x 8, pulse x 8     off 0, 32, 64, 96    120 coordinates, 64 slots, RW 124
      64 slots (s_leafv, s_par full); four branches; offset mask bit 31; ramp slot 15 = coordinates 62, 63: the branch ends exactly at
      64; burst's box looked up past 64 (off = 64, never by shuffle); widths 1, 2, 4, 3 in one record
  burst_across_64         offset x 1, burst x 30                           off 0, 1             121 coordinates, 31 slots, RW 124
      burst slot 15 = coordinates 61 - 64: three lanes of ballot word 0 and one of word 1 (four bits wanted from lane 61); every burst
      slot at an odd offset; a 120-double segment
  ramp_across_64          offset x 31, ramp x 32                           off 0, 31            95 coordinates, 63 slots, RW 98
      ramp slot 16 = coordinates 63, 64; ramp mask bit 31; numpy_sum over n = 31 (remainder 7) and n = 32 (no remainder)
  pulses_RW128            pulse x 32, sine x 10                            off 0, 96            126 coordinates, 42 slots, RW 128
      the record maximum without a pad; pulse slot 21 = coordinates 63 - 65; pulse mask bit 31; the sine branch entirely in the second
      pass.  40 data points (strided) and 130 (uniform-grid recurrence, s_par per slot, birth / death by difference)
  coords_63               pulse x 21                                       off 0                63 coordinates, 21 slots, RW 64
  coords_64               burst x 16                                       off 0                64 coordinates, 16 slots, RW 66
  coords_65               burst x 16, offset x 1                           off 0, 64            65 coordinates, 17 slots, RW 68
      the in-model accept uniform is drawn by lane ncoord & 63 of pass ncoord >> 6: lane 63; lane 0 of a second pass; lane 1
  general_ndims_1234      host-callable, widths 1, 2, 3, 4; 32, 16, 8, 8   off 0, 32, 64, 88    120 coordinates, 64 slots, RW 124
      hens_rj_propose / hens_rj_accept at 64 slots, birth rows of stride 4
  general_RW128           host-callable, widths 1, 4, 2; 1, 30, 2 leaves   off 0, 1, 121        125 coordinates, 33 slots, RW 128
      the record maximum; the 4-wide slot 15 = coordinates 61 - 64.  (Widths 4, 2 with 30 and 3 leaves put slot 15 at 60 - 63 and
      slot 16 at 64 - 67: neither straddles, and a leading 1-wide branch in front of them makes 130 doubles; so one leaf of the last
      branch went.)
"""
import numpy as np

from tests import leaf_kind_cases as cases
from tests import leaf_kinds as lk

GENERAL_BOX = {1: [(-3.0, 3.0)], 2: [(-1.0, 1.0), (-2.0, 2.0)], 3: [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)],
               4: [(0.5, 3.0), (-1.0, 1.0), (0.05, 0.5), (1.0, 8.0)]}
# name: kinds (a leaf kind's name, or a width for a host-callable branch), nleaves_max, then the stated arithmetic and the slots across 64
MODELS = {
    "four_branches_64_slots": dict(kinds=("offset", "ramp", "burst", "pulse"), nl_max=(32, 16, 8, 8), off=(0, 32, 64, 96), ncoord=120,
                                   slots=64, RW=124, across=[]),
    "burst_across_64": dict(kinds=("offset", "burst"), nl_max=(1, 30), off=(0, 1), ncoord=121, slots=31, RW=124, across=[(1, 15)]),
    "ramp_across_64": dict(kinds=("offset", "ramp"), nl_max=(31, 32), off=(0, 31), ncoord=95, slots=63, RW=98, across=[(1, 16)]),
    "pulses_RW128": dict(kinds=("pulse", "sine"), nl_max=(32, 10), off=(0, 96), ncoord=126, slots=42, RW=128, across=[(0, 21)]),
    "coords_63": dict(kinds=("pulse",), nl_max=(21,), off=(0,), ncoord=63, slots=21, RW=64, across=[]),
    "coords_64": dict(kinds=("burst",), nl_max=(16,), off=(0,), ncoord=64, slots=16, RW=66, across=[]),
    "coords_65": dict(kinds=("burst", "offset"), nl_max=(16, 1), off=(0, 64), ncoord=65, slots=17, RW=68, across=[]),
    "general_ndims_1234": dict(kinds=(1, 2, 3, 4), nl_max=(32, 16, 8, 8), off=(0, 32, 64, 88), ncoord=120, slots=64, RW=124, across=[]),
    "general_RW128": dict(kinds=(1, 4, 2), nl_max=(1, 30, 2), off=(0, 1, 121), ncoord=125, slots=33, RW=128, across=[(1, 15)]),
}
DEVICE_MODELS = [m for m, r in MODELS.items() if isinstance(r["kinds"][0], str)]
GENERAL_MODELS = [m for m in MODELS if m not in DEVICE_MODELS]
# noise widths: a leaf moves the log-likelihood by a fraction of a unit, so that births and deaths are accepted at every budget, and the
# float64 oracle stays within a small fraction of B of exact arithmetic with up to 64 leaves in use (tests/test_limit_records.py)
SIGMA = {40: 8.0, 130: 8.0}


# the host function of a host-callable model: tests/leaf_kinds.py's kinds of the same widths (GENERAL_BOX holds their boxes)
HOST_KIND = {1: "offset", 2: "ramp", 3: "pulse", 4: "burst"}


def is_general(model):
    return model in GENERAL_MODELS


def like_kinds(model):
    """The leaf kinds of the model's likelihood: its own, or the host function's."""
    return tuple(k if isinstance(k, str) else HOST_KIND[k] for k in MODELS[model]["kinds"])


def widths(model):
    return tuple(lk.KINDS[k][1] if isinstance(k, str) else int(k) for k in MODELS[model]["kinds"])


class GeneralBranch:
    """A host-callable branch (no leaf kind): name, box, budget - what the oracle and eryn_amd.rj.LeafBranch need."""

    def __init__(self, name, box, nleaves_max, nleaves_min=0):
        self.name, self.kind, self.box = name, None, [tuple(map(float, b)) for b in box]
        self.ndim, self.nleaves_max, self.nleaves_min = len(self.box), int(nleaves_max), int(nleaves_min)

    def to_oracle(self, cov=None):
        from oracle import eryn_oracle_rj as orj
        return orj.Branch(self.name, 0, self.box, self.nleaves_max, self.nleaves_min, cov=cov)

    def to_device(self):
        from eryn_amd.rj import LeafBranch
        return LeafBranch(self.name, self.box, self.nleaves_max, self.nleaves_min)


def branches(model):
    """One branch per entry of the row, named after its kind (a host-callable one: ``w<width>``); no floor under any budget."""
    row = MODELS[model]
    if is_general(model):
        return [GeneralBranch(f"w{k}", GENERAL_BOX[k], n) for k, n in zip(row["kinds"], row["nl_max"])]
    return cases.branches_of(row["kinds"], row["nl_max"])


def layout(model):
    """(off[b], ncoord, slots, RW) from the widths and budgets alone."""
    nd, nl = widths(model), MODELS[model]["nl_max"]
    off = tuple(int(v) for v in np.cumsum([0] + [n * d for n, d in zip(nl, nd)])[:-1])
    ncoord = sum(n * d for n, d in zip(nl, nd))
    rw = ncoord + len(nd)
    return off, ncoord, sum(nl), rw + (rw & 1)


def slot_coords(model, b, s):
    """(first, last) record coordinate of slot s of branch b."""
    off, nd = layout(model)[0], widths(model)
    return off[b] + s * nd[b], off[b] + s * nd[b] + nd[b] - 1


def across_64(model):
    """The slots with a coordinate on each side of 64."""
    out = []
    for b, n in enumerate(MODELS[model]["nl_max"]):
        for s in range(n):
            first, last = slot_coords(model, b, s)
            if first < 64 <= last:
                out.append((b, s))
    return out


def edges(model):
    """The (branch, slot) pairs a case must cover: slot 0 of every branch (the first slot of a branch that begins at or past 64 among
    them), the top slot of every 32-leaf branch, every slot across coordinate 64."""
    out = [(b, 0) for b in range(len(MODELS[model]["nl_max"]))]
    out += [(b, 31) for b, n in enumerate(MODELS[model]["nl_max"]) if n == 32]
    out += across_64(model)
    return sorted(set(out))


def problem(model, ndata, seed=0):
    """(branches, t, y, sigma): the data of tests/leaf_kind_cases.make_data on linspace(-1, 1, ndata)."""
    brs = branches(model)
    t = np.linspace(-1, 1, ndata)
    sigma = SIGMA[ndata]
    y = cases.make_data(cases.branches_of(like_kinds(model), MODELS[model]["nl_max"]), t, sigma, np.random.RandomState(1000 + seed))
    return brs, t, y, sigma


# walker classes per edge (B, s), in the proportion they are dealt: what each forces is said in ``start``
CLASSES = ("all_but", "all_but", "all_but", "pair", "pair", "pair", "pair", "full", "half")


def start(model, T, W, seed=0, p_active=0.5):
    """(x, inds, classes): every slot's coordinates uniform in its box (well inside: the middle 90 %), masks by walker class.  Walkers
    are dealt, in (t, w) order and over and over, one per entry of CLASSES for every pair (B, s) of ``edges(model)``; branches other
    than B hold a random half (``p_active``) unless said otherwise:
      all_but  every slot of B but s in use: every birth on B goes to s and lands at nleaves_max (the edge factor fires)
      pair     exactly {s, one other slot} of B in use (a branch of one leaf: {s}): a death takes s half the time
      full     every slot of B in use: the death is forced, the mask of the candidates 2^nl - 1 (0xffffffff at 32 leaves)
      half     s in use among a random half: the in-model move carries s
    and, first of all on every rung, one walker without any leaf and one with leaves in the last branch only (fix_logp_gibbs).
    ``classes[t, w]`` = (class, B, s)."""
    brs = branches(model)
    rs = np.random.RandomState(7000 + seed)
    x, inds = {}, {}
    for b in brs:
        lo, hi = np.array([q[0] for q in b.box]), np.array([q[1] for q in b.box])
        x[b.name] = lo + (hi - lo) * (0.05 + 0.9 * rs.rand(T, W, b.nleaves_max, b.ndim))
        inds[b.name] = rs.rand(T, W, b.nleaves_max) < p_active
    deal = [(c, B, s) for (B, s) in edges(model) for c in CLASSES]
    classes = np.empty((T, W), dtype=object)
    k = 0
    for tt in range(T):
        for w in range(W):
            if w == 0:
                for b in brs:
                    inds[b.name][tt, w] = False
                classes[tt, w] = ("empty", -1, -1)
                continue
            if w == 1:
                for b in brs:
                    inds[b.name][tt, w] = False
                inds[brs[-1].name][tt, w, rs.randint(brs[-1].nleaves_max)] = True
                classes[tt, w] = ("last_only", -1, -1)
                continue
            c, B, s = deal[k % len(deal)]
            k += 1
            m = inds[brs[B].name][tt, w]
            n = brs[B].nleaves_max
            if c == "all_but":
                m[:] = True
                m[s] = False
            elif c == "pair":
                m[:] = False
                m[s] = True
                if n > 1:
                    m[(s + 1 + rs.randint(n - 1)) % n] = True
            elif c == "full":
                m[:] = True
            else:
                m[s] = True
            classes[tt, w] = (c, B, s)
    return x, inds, classes


def dense_state(model, T, W, seed=0, p_active=0.97):
    """Random walkers with 97 % of the slots in use, walker (0, 0) without a leaf, walker (0, 1) with leaves in the last branch only
    (the rules of tests/leaf_kind_cases.accuracy_case)."""
    brs = branches(model)
    x, inds = cases.random_state(brs, T, W, np.random.RandomState(8000 + seed), p_active=p_active)
    for b in brs:
        inds[b.name][0, 0] = False
        inds[b.name][0, 1] = b is brs[-1]
    return x, inds


def offender_steps(brs, x, b, s, d, high):
    """An in-model step that leaves every coordinate where it is but coordinate d of slot s of branch b, which goes a quarter of its
    box's width past the upper (``high``) or lower edge: the proposal of every walker with the slot in use has one sole offender."""
    steps = {q.name: np.zeros(x[q.name].shape) for q in brs}
    lo, hi = brs[b].box[d]
    cur = x[brs[b].name][:, :, s, d]
    steps[brs[b].name][:, :, s, d] = (hi - cur) + 0.25 * (hi - lo) if high else (lo - cur) - 0.25 * (hi - lo)
    return steps


class Coverage:
    """Counts, per (branch, slot), from the oracle's trace records: proposed and accepted births, proposed and accepted deaths, accepted
    in-model moves of a walker with the slot in use, and in-model proposals whose only out-of-box coordinates belong to the slot
    (``sole``; ``sole_coord[b][s, d]``: ... and it is coordinate d alone)."""
    KEYS = ("birth_prop", "birth_acc", "death_prop", "death_acc", "inmodel_acc", "sole")

    def __init__(self, brs):
        self.brs = list(brs)
        self.n = {k: [np.zeros(b.nleaves_max, dtype=int) for b in self.brs] for k in self.KEYS}
        self.sole_coord = [np.zeros((b.nleaves_max, b.ndim), dtype=int) for b in self.brs]
        self.inmodel_by_rung = None                      # [T, 2]: rejected, accepted in-model proposals per rung

    def add(self, rec):
        brs = self.brs
        acc = np.asarray(rec["mh_accepted"], dtype=bool)
        if self.inmodel_by_rung is None:
            self.inmodel_by_rung = np.zeros((acc.shape[0], 2), dtype=int)
        self.inmodel_by_rung[:, 1] += acc.sum(axis=1)
        self.inmodel_by_rung[:, 0] += (~acc).sum(axis=1)
        for bi, b in enumerate(brs):
            self.n["inmodel_acc"][bi] += (rec[f"pre_inds_{b.name}"] & acc[:, :, None]).sum(axis=(0, 1))
        if "mh_q" in rec:                                # (the Gaussian move: the proposal of every walker)
            out = []
            for b in brs:
                lo, hi = np.array([q[0] for q in b.box]), np.array([q[1] for q in b.box])
                q = rec["mh_q"][b.name]
                out.append(rec[f"pre_inds_{b.name}"][..., None] & ~((q >= lo) & (q <= hi)))
            slots_out = sum(o.any(axis=-1).sum(axis=-1) for o in out)
            coords_out = sum(o.sum(axis=(-1, -2)) for o in out)
            for bi in range(len(brs)):
                one = out[bi].any(axis=-1) & (slots_out == 1)[:, :, None]
                self.n["sole"][bi] += one.sum(axis=(0, 1))
                self.sole_coord[bi] += (out[bi] & (coords_out == 1)[:, :, None, None]).sum(axis=(0, 1))
        for sub in rec.get("rj_sub", [rec]):
            if "rj_accepted" not in sub:
                continue
            bis = sub["rj_branches"] if "rj_branches" in sub else [sub["rj_branch"]]
            chs = sub["rj_change_all"] if "rj_branches" in sub else [sub["rj_change"]]
            lfs = sub["rj_leaf_all"] if "rj_branches" in sub else [sub["rj_leaf"]]
            ok = np.asarray(sub["rj_accepted"], dtype=bool)
            for bi, ch, lf in zip(bis, chs, lfs):
                for sign, key in ((+1, "birth"), (-1, "death")):
                    np.add.at(self.n[key + "_prop"][bi], lf[ch == sign], 1)
                    np.add.at(self.n[key + "_acc"][bi], lf[(ch == sign) & ok], 1)

    def at(self, b, s):
        return {k: int(self.n[k][b][s]) for k in self.KEYS}

    def line(self, pairs):
        return "; ".join(f"({b}, {s}): " + " ".join(f"{k} {v}" for k, v in self.at(b, s).items()) for b, s in pairs)

    def missing(self, wanted):
        """Those of ``wanted`` [(branch, slot, key)] that never happened."""
        return [(b, s, k) for b, s, k in wanted if self.n[k][b][s] < 1]


def required(model, sole=False):
    """[(branch, slot, key)]: an accepted birth, an accepted death and an accepted in-model move on every pair of ``edges(model)``
    (``sole``: and a proposal rejected for that slot alone).  The one leaf of a one-leaf branch cannot die: the branch is then empty,
    and fix_logp_gibbs gives such a proposal the log-prior -inf while another branch holds a leaf, the fill likelihood -1e300 when
    none does - so there the PROPOSED death is what is asked for."""
    nl = MODELS[model]["nl_max"]
    keys = ("birth_acc", "death_acc", "inmodel_acc") + (("sole",) if sole else ())
    return [(b, s, "death_prop" if (k == "death_acc" and nl[b] == 1) else k) for b, s in edges(model) for k in keys]


# ---- the teacher-forced cases (tests/test_hip_limit_records.py section a; sized in tests/test_limit_records.py) -------------------------
# (model, data points, schedule, in-model move): T x W walkers from ``start``, TF_ITERS iterations on host draws, then for every pair of
# ``edges(model)`` two iterations whose in-model step is ``offender_steps`` on the slot's lowest (downwards) and highest (upwards)
# coordinate.  Seeds: those of TF_SEEDS, else TF_SEED.
TF_T, TF_W, TF_ITERS, TF_SEED = 2, 48, 8, 3
def case_id(c):
    return "-".join(map(str, c))


TF_CASES = [(m, 40, "iterate_branches", "gaussian") for m in DEVICE_MODELS] + [
    ("pulses_RW128", 130, "iterate_branches", "gaussian"), ("four_branches_64_slots", 40, "together", "gaussian"),
    ("four_branches_64_slots", 40, "separate_branches", "gaussian"), ("burst_across_64", 40, "separate_branches", "stretch"),
    ("pulses_RW128", 130, "together", "stretch"),
    # hens_rj_propose / hens_rj_accept around the host function (tests/test_hip_limit_records.py section b)
    ("general_ndims_1234", 40, "iterate_branches", "gaussian"), ("general_ndims_1234", 40, "together", "gaussian"),
    ("general_RW128", 40, "iterate_branches", "gaussian"), ("general_RW128", 40, "separate_branches", "stretch")]
TF_SEEDS = {}


def tf_oracle_class(base):
    class Forced(base):
        """The oracle whose in-model Gaussian step is ``forced`` ({name: [T, W, nl, nd]}) while that is set."""
        forced = None

        def _draw_steps(self, b, n):
            if self.forced is not None:
                return self.forced[b.name][self.st.inds[b.name]]
            return super()._draw_steps(b, n)
    return Forced


def tf_oracle(model, ndata, schedule, in_model):
    """The recording oracle of a teacher-forced case on its host streams (knife-edge swaps counted, the stretch move living
    dangerously: W < 2 ncoord), its branches, and the start's walker classes."""
    from oracle import eryn_oracle_rj as orj
    from tests.test_hip_leaf_kinds import _counting
    seed = TF_SEEDS.get((model, ndata, schedule, in_model), TF_SEED)
    brs, t, y, sigma = problem(model, ndata, seed)
    x, inds, classes = start(model, TF_T, TF_W, seed)
    obr = [b.to_oracle(cov=np.diag([(0.02 * (hi - lo)) ** 2 for lo, hi in b.box])) for b in brs]
    cls = tf_oracle_class(_counting(orj.OracleRJSampler))
    o = cls(obr, x, inds, t, y, sigma, np.random.RandomState(100 + seed), np.random.RandomState(200 + seed), 0.35 ** np.arange(TF_T),
            record=True, schedule=schedule, in_model=in_model, like_fn=lk.like_fn(like_kinds(model)))
    o.live = in_model == "stretch"
    return o, brs, classes


def tf_iterations(o, brs, model):
    """Generator over the case's iterations: sets ``o.forced`` and yields a label; the caller runs ``o.iteration()``."""
    for it in range(TF_ITERS):
        o.forced = None
        yield f"it{it}"
    if o.in_model == "gaussian":
        for b, s in edges(model):
            for d, high in ((0, False), (brs[b].ndim - 1, True)):
                o.forced = offender_steps(brs, o.st.x, b, s, d, high)
                yield f"offender ({b}, {s}) coordinate {d} {'up' if high else 'down'}"
    o.forced = None
