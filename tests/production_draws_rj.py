"""NumPy specification of the PRODUCTION draws of the red / blue stretch move of ``hens_rj_step`` (test infrastructure).

The leaf-packing sampler's stretch move (``hens_rj_set_in_model(HENS_RJ_INMODEL_STRETCH)``) draws from the library's own
counter-based stream, not from the reference's Mersenne Twisters: every draw is a pure function of
(seed, iteration, global rung, walker, half, branch), so a resumed or re-sharded context regenerates it, nothing is planned
on the host and nothing is read from draw arrays.  This file states the construction independently of the HIP code
(eryn_amd/csrc/hens_rj.h: rj_split_walker, rj_split_complement, rj_stretch_key, rj_acc_key, k_rj<RJ_MODE_STRETCH, 0>,
k_rj_debug_stretch) with the generator and the keyed permutation of tests/production_draws.py; ``hens_rj_debug_draws_stretch``
must return exactly these arrays (tests/test_hip_rj_stretch.py).

Construction (n0 = ceil(W / 2); wid = global rung * W + walker; a Philox call is
philox4x32_10(iter lo, iter hi, wid, key word; seed lo, seed hi)):

* Split.  Rung t's shuffled order is the keyed permutation ``order[p] = prp(p, prp_key(seed, iter, PURPOSE_RJ_SPLIT, t))``
  of the walkers.  The walkers at positions [0, n0) are set 0, the others set 1: a uniformly random balanced labelling like
  the reference's shuffle of ``arange(W) % 2`` (red_blue.py:119-124), in closed form - position k of half h holds walker
  ``order[h n0 + k]``, so a wavefront finds its walker without a table.
* Complement of branch b for a walker of half h: word 0 of the call keyed ``PURPOSE_RJ_STRETCH | h << 8 | b << 16`` goes
  through ``rj_pick(word, Nc) = (word * Nc) >> 32`` to a POSITION of the other half (Nc walkers); the complement is the walker
  there - a different draw per branch (stretch.py:93-100, 205).
* u_zz: ``u01(word 1, word 2)`` of branch 0's call (stretch.py:128-132: the first branch only, one factor per walker).
* Accept uniform: ``u01(word 0, word 1)`` of the call keyed ``PURPOSE_RJ_ACC | RJ_MODE_STRETCH << 8 | h << 16`` (red_blue.py:294).

The draws are keyed by the WALKER, not by its position in a list: the exported form of ``hens_rj_stretch_split`` (movers in
ascending walker order, ``rint`` an index into the other set's ascending list) is a relabelling of the same values.
"""
import numpy as np

from tests.production_draws import idx_bits_of, philox4x32_10, prp, prp_key, u01

PURPOSE_RJ_ACC, PURPOSE_RJ_SPLIT, PURPOSE_RJ_STRETCH = 21, 25, 26
RJ_MODE_STRETCH = 3


def rj_pick(word, n):
    """Uniform on [0, n) from one 32-bit word (hens_rj.h: rj_pick)."""
    return ((np.asarray(word, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def split_order(seed, it, rung, W):
    """order[p]: the walker at position p of global rung ``rung``'s shuffled order."""
    return prp(np.arange(W), prp_key(seed, it, PURPOSE_RJ_SPLIT, rung), idx_bits_of(W), W)


def stretch_draws(seed, it, T, W, nbranches, rung_begin=0):
    """Everything the stretch move of iteration ``it`` draws on rungs rung_begin .. rung_begin + T - 1, in the form
    ``hens_rj_stretch_split`` takes: ``labels`` [T, W] uint8; per half h (list index) ``rint`` [nbranches, T, Ns_h] int64,
    ``u_zz`` / ``u_acc`` [T, Ns_h], movers in ascending walker order (Ns_0 = n0, Ns_1 = W - n0).  Also, for the tests of the
    construction itself, ``movers`` [T, Ns_h] and ``cw`` [nbranches, T, Ns_h]: the walkers that move and their complements."""
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    n0 = (W + 1) // 2
    ns = (n0, W - n0)
    labels = np.zeros((T, W), dtype=np.uint8)
    out = dict(labels=labels, rint=[np.zeros((nbranches, T, n), dtype=np.int64) for n in ns],
               u_zz=[np.zeros((T, n)) for n in ns], u_acc=[np.zeros((T, n)) for n in ns],
               movers=[np.zeros((T, n), dtype=np.int64) for n in ns], cw=[np.zeros((nbranches, T, n), dtype=np.int64) for n in ns])
    for t in range(T):
        rung = rung_begin + t
        order = split_order(seed, it, rung, W)
        labels[t, order[n0:]] = 1
        halves = (order[:n0], order[n0:])
        for h in range(2):
            movers = np.sort(halves[h])                                   # ascending walker order (red_blue.py:150-154)
            other, other_sorted = halves[1 - h], np.sort(halves[1 - h])
            wid = rung * W + movers
            out["movers"][h][t] = movers
            for b in range(nbranches):
                d = philox4x32_10(it & 0xFFFFFFFF, it >> 32, wid, PURPOSE_RJ_STRETCH | (h << 8) | (b << 16), lo, hi)
                cw = other[rj_pick(d[0], len(other))] if len(other) else np.zeros(0, dtype=np.int64)
                out["cw"][h][b, t] = cw
                out["rint"][h][b, t] = np.searchsorted(other_sorted, cw)  # index into the other set's ascending list
                if b == 0:
                    out["u_zz"][h][t] = u01(d[1], d[2])
            d = philox4x32_10(it & 0xFFFFFFFF, it >> 32, wid, PURPOSE_RJ_ACC | (RJ_MODE_STRETCH << 8) | (h << 16), lo, hi)
            out["u_acc"][h][t] = u01(d[0], d[1])
    return out
