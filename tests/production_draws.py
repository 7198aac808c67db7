"""NumPy specification of the PRODUCTION random draws of ``hens_step`` (test infrastructure).

Not a restatement of the reference (that is ``oracle/``): the reference draws from NumPy's global Mersenne Twister,
which a device cannot reproduce in parallel.  Production stepping draws from Philox4x32-10 (Salmon et al. 2011), a
pure function of (seed, iteration, purpose, global rung, walker), and builds its permutations from a keyed Feistel
network.  This file states that construction independently of the HIP code (eryn_amd/csrc/hens_kernels.h:
philox4x32_10, u01, stretch_draw, prp_key, pmix, prp, place_column, k_plan, k_plan_draws, stretch_draws_at, pt_slot,
pt_uniform; for the Gaussian / MH move mh_uniform, mh_normal_key, mh_normal_quad, mh_normal_pair, mh_pair_rows,
mh_normal_from32, k_mh_draw, and the host's move_uniform / iteration_is_mh in eryn_amd/csrc/hens.hip) so that

* the generator can be pinned on CPU against the published known-answer vectors of Random123 (test_host_logic), and
* ``hens_debug_draws`` - hence the draws the timed path consumes - can be compared with it bit for bit on the GPU.

Distributional equivalence with the reference's draws (balanced random halves, uniform complement, uniform matchings,
uniform accept numbers) is what tests/test_hip_rng.py measures; tests/replay_utils.py turns these draws into the
reference's own variables and replays them through the oracle.

The Gaussian move's normals are the one draw that is NOT bit-exact by construction: the device takes logarithm, square
root, sine and cosine on its single-precision units.  mh_normal_ideal states the function they approximate in float64,
MH_NORMAL_E how far the device may be from it (measured, see there), and normal_stream_stats what "standard normal and
independent" means for a stream of them - for the specification's values and the device's alike.
"""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
PURPOSE_STRETCH, PURPOSE_STRETCH_ACC, PURPOSE_SPLIT, PURPOSE_PTPERM, PURPOSE_PTU = 0, 2, 8, 9, 10
PURPOSE_MH_ACC, PURPOSE_MH_NORMAL, PURPOSE_MOVE = 11, 12, 13


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over the counter words (arrays or scalars of any broadcastable shape); returns four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & MASK, p1 & MASK,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def u01(hi, lo):
    """53-bit uniform in [0, 1) from two words."""
    v = (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)
    return (v >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & MASK
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & MASK
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & MASK
    h ^= h >> np.uint64(16)
    return h


def prp_key(seed, it, purpose, rung):
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    a = philox4x32_10(it & 0xFFFFFFFF, it >> 32, rung, purpose, lo, hi)
    b = philox4x32_10(it & 0xFFFFFFFF, it >> 32, rung, purpose ^ 0x100, lo, hi)
    return [int(v) for v in a + b]


def idx_bits_of(W):
    b, n = 0, 1
    while n < W:
        n <<= 1
        b += 1
    return b


def pmix(x, k):
    """Round function of the Feistel network: two 24-bit multiplies with a shift-xor between them (hens_kernels.h: pmix)."""
    m24 = np.uint64(0xFFFFFF)
    h = (((np.asarray(x, dtype=np.uint64) ^ np.uint64(k)) & m24) * np.uint64(0x9E3779)) & MASK
    h ^= h >> np.uint64(15)
    h = ((h & m24) * np.uint64(0x85EBCB)) & MASK
    return h >> np.uint64(11)


def _feistel(x, key, bits, inverse):
    lb = bits >> 1
    rb = bits - lb
    lm, rm = np.uint64((1 << lb) - 1), np.uint64((1 << rb) - 1)
    L, R = x >> np.uint64(rb), x & rm
    rounds = range(6, -1, -2) if inverse else range(0, 8, 2)
    for r in rounds:
        if inverse:
            R = R ^ (pmix(L, key[r + 1]) & rm)
            L = L ^ (pmix(R, key[r]) & lm)
        else:
            L = L ^ (pmix(R, key[r]) & lm)
            R = R ^ (pmix(L, key[r + 1]) & rm)
    return (L << np.uint64(rb)) | R


def prp(x, key, bits, W, inverse=False):
    """Keyed permutation of [0, W): 8-round alternating Feistel network on ``bits`` bits (round function pmix),
    cycle-walked into range."""
    x = np.array(x, dtype=np.uint64, copy=True)
    out = _feistel(x, key, bits, inverse)
    while True:
        bad = out >= np.uint64(W)
        if not bad.any():
            return out.astype(np.int64)
        out[bad] = _feistel(out[bad], key, bits, inverse)


def place_column(h, p, cb):
    """Column that meets the walker at place p of half h: block * cb + h * cb/2 + member (hens_kernels.h: place_column)."""
    hb = cb // 2
    return (p // hb) * cb + h * hb + (p % hb)


def label_cb(T, W, tempered=True):
    """Columns per block of the block-balanced labelling, or 0 (hens_create)."""
    if tempered and 2 <= T <= 64:
        cb = 1
        while cb * 2 * T <= 128:          # the largest power of two with cb T <= 128 (= 128 / T where T divides 128)
            cb *= 2
        if cb >= 2 and W % cb == 0:
            return cb
    return 0


def stretch_draw(seed, it, wid):
    """(u_zz, u_acc, r22) of split position ``wid`` = rung * W + position: ONE Philox call (stretch_draw in
    hens_kernels.h) - two 53-bit uniforms and, from the 2 x 11 low bits they do not use, a 22-bit number that indexes the
    complement half."""
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    d = philox4x32_10(it & 0xFFFFFFFF, it >> 32, wid, PURPOSE_STRETCH, lo, hi)
    r22 = ((d[1].astype(np.uint64) & np.uint64(0x7FF)) << np.uint64(11)) | (d[3].astype(np.uint64) & np.uint64(0x7FF))
    return u01(d[0], d[1]), u01(d[2], d[3]), r22


def plan(seed, it, T, W, cb):
    """own, cw, u_zz, u_acc of iteration ``it`` for the whole ladder, [T][W] by split position (k_plan; with block-balanced
    labels k_plan_draws / stretch_draws_at).  Without block labels both halves are listed in ascending walker order; with
    them the walker at place p of half h is the one the column place_column(h, p) meets."""
    bits, N0 = idx_bits_of(W), (W + 1) // 2
    own = np.empty((T, W), dtype=np.int64)
    cw = np.empty((T, W), dtype=np.int64)
    uz = np.empty((T, W))
    ua = np.empty((T, W))
    w = np.arange(W)
    s0 = w < N0
    for t in range(T):
        key = prp_key(seed, it, PURPOSE_PTPERM if cb else PURPOSE_SPLIT, t)
        if cb:
            order = prp(place_column((~s0).astype(np.int64), np.where(s0, w, w - N0), cb), key, bits, W)
        else:
            lab = (prp(w, key, bits, W) >= N0).astype(np.int64)
            order = np.concatenate([w[lab == 0], w[lab == 1]])                   # both halves ascending
            assert (lab == 0).sum() == N0
        own[t] = order
        uz[t], ua[t], r22 = stretch_draw(seed, it, t * W + w)
        Nc = np.where(s0, W - N0, N0).astype(np.uint64)
        r = ((r22 * Nc) >> np.uint64(22)).astype(np.int64)                       # uniform index into the other half
        cw[t] = order[np.where(s0, N0, 0) + r]
    return dict(own=own, cw=cw, u_zz=uz, u_acc=ua)


def pt_draws(seed, it, T, W):
    """pt_slot [T][W] (column c meets slot pt_slot[t, c]) and u_swap [T-1][W] (row j: pair T-1-j)."""
    bits = idx_bits_of(W)
    c = np.arange(W)
    slot = np.empty((T, W), dtype=np.int64)
    for t in range(T):
        slot[t] = prp(c, prp_key(seed, it, PURPOSE_PTPERM, t), bits, W)
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    u = np.empty((T - 1, W))
    for j in range(T - 1):
        d = philox4x32_10(it & 0xFFFFFFFF, it >> 32, j * W + c, PURPOSE_PTU, lo, hi)
        u[j] = u01(d[0], d[1])
    return slot, u


# ---------------------------------------------------------------------------------------------------------------------
# The Gaussian / Metropolis-Hastings move (hens_set_mh_proposal): which iterations propose it, the accept uniforms, the
# proposal's standard normals.
# ---------------------------------------------------------------------------------------------------------------------
def _call(seed, it, c2, c3):
    """The Philox call every draw of iteration ``it`` makes: counter (it lo, it hi, c2, c3), key (seed lo, seed hi)."""
    return philox4x32_10(it & 0xFFFFFFFF, (it >> 32) & 0xFFFFFFFF, c2, c3, seed & 0xFFFFFFFF, seed >> 32)


def move_uniform(seed, it):
    """The uniform behind the weighted move choice of iteration ``it``: one per iteration, on the host."""
    d = _call(seed, it, 0, PURPOSE_MOVE)
    return float(u01(d[0], d[1]))


def is_mh(seed, it, weight):
    """Whether iteration ``it`` is a Gaussian-move iteration when the move has probability ``weight``."""
    if weight <= 0.0:
        return False
    return weight >= 1.0 or move_uniform(seed, it) < weight


def mh_uniform(seed, it, rung, W):
    """Accept uniforms [W] of global rung ``rung``."""
    d = _call(seed, it, rung * W + np.arange(W), PURPOSE_MH_ACC)
    return u01(d[0], d[1])


def mh_pair_rows(RW):
    """g: walkers w and w + g (w's bit g clear) of a rung share a Philox call at device row width RW; 0: nobody shares."""
    return {128: 8, 64: 16, 32: 32, 16: 32}.get(RW, 0)


def mh_normal_address(rung, W, RW):
    """Where the Box-Muller pair of (walker, coordinate pair) comes from: counter word 2, counter word 3 and which half of
    the call's four words (0: words 0, 1; 1: words 2, 3), each [W, ceil(RW/2)]."""
    g = mh_pair_rows(RW)
    w = np.arange(W, dtype=np.int64)[:, None]
    pr = np.arange((RW + 1) // 2, dtype=np.int64)[None, :]
    c2, c3, half = np.broadcast_arrays(rung * W + (w & ~g), PURPOSE_MH_NORMAL | (pr << 8), ((w & g) != 0).astype(np.int64))
    return c2, c3, half


def mh_normal_words(seed, it, rung, W, RW):
    """(a, b), [W, ceil(RW/2)] uint32 each: the word behind the radius and the word behind the angle of the Box-Muller
    pair that gives coordinates (2 pr, 2 pr + 1) of walker w."""
    c2, c3, half = mh_normal_address(rung, W, RW)
    d = _call(seed, it, c2, c3)
    return np.where(half == 1, d[2], d[0]), np.where(half == 1, d[3], d[1])


def mh_normal_ideal(a, b):
    """The two standard normals of words (a, b), float64.  The uniforms are formed in single precision - u1 in (0, 1],
    the angle in revolutions in [0, 1] - exactly as the device forms them: a conversion, an addition and a multiplication
    by a power of two, correctly rounded operations with one possible result.  Everything after that is the function
    the device approximates: Box-Muller."""
    two_m32 = np.float32(2.0 ** -32)
    u1 = (np.asarray(a, dtype=np.uint32).astype(np.float32) + np.float32(1.0)) * two_m32
    ang = np.asarray(b, dtype=np.uint32).astype(np.float32) * two_m32
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)) + 0.0)              # (+ 0.0: u1 = 1 gives radius +0, not -0)
    t = 2.0 * np.pi * ang.astype(np.float64)
    return r * np.cos(t), r * np.sin(t)


# How far the device's normals (mh_normal_from32: v_log_f32, v_sqrt_f32, v_sin_f32, v_cos_f32 and float32 products) may
# be from mh_normal_ideal, absolute, per value.  MH_NORMAL_OBSERVED is the largest deviation measured on an MI355X over
# every draw of tests/test_production_draws_mh.py::test_device_mh_draws_equal_the_specification (all row-width classes,
# W = 100 and 200, iterations 0, 1 and the counter edges); the bar is four times that - the deviation is a property of
# the units, not of the sample, and the factor covers the inputs not drawn.  It may not exceed 1e-4: an error of the
# mapping (a wrong word, walker or coordinate) is of order 1, and 1e-4 is far below what the distribution bars resolve.
# Measured: 5.593e-07 (at row width 128, W = 200; 3.6e-07 .. 5.4e-07 in the other classes) - about one float32 ulp of a
# value in [4, 8), 4.8e-07: the units and the two float32 products cost no more than the format itself.
MH_NORMAL_OBSERVED = 5.593e-07
MH_NORMAL_E = 4.0 * MH_NORMAL_OBSERVED                                    # 2.237e-06


def mh_steps(seed, it, T, W, RW, kind, scale, rung_begin=0, weight=1.0):
    """What ``hens_debug_draws`` exports of the Gaussian move for T resident rungs from global rung ``rung_begin``:
    z [T, W, RW] the standard normals (float64 ideal), mh_step the proposal's steps (kind "iso": scale z, "diag":
    scale[d] z, "full": L z with L = scale the lower Cholesky factor [RW, RW]), mh_u [T, W], is_mh."""
    z = np.empty((T, W, RW))
    u = np.empty((T, W))
    for t in range(T):
        zx, zy = mh_normal_ideal(*mh_normal_words(seed, it, rung_begin + t, W, RW))
        z[t, :, 0::2] = zx
        z[t, :, 1::2] = zy[:, :RW // 2]                                  # (odd RW: the last pair's second normal is dropped)
        u[t] = mh_uniform(seed, it, rung_begin + t, W)
    if kind == "full":
        step = z @ np.asarray(scale, dtype=np.float64).reshape(RW, RW).T
    else:
        step = z * (float(scale) if kind == "iso" else np.asarray(scale, dtype=np.float64).reshape(RW))
    return dict(z=z, mh_step=step, mh_u=u, is_mh=is_mh(seed, it, weight))


def _corr_z(x, y):
    """Sample correlation of x and y times sqrt(n): standard normal for independent samples."""
    x = np.ravel(x) - np.mean(x)
    y = np.ravel(y) - np.mean(y)
    return float(np.dot(x, y) / math.sqrt(np.dot(x, x) * np.dot(y, y)) * math.sqrt(x.size))


def _ks_normal(v):
    """Kolmogorov-Smirnov distance of the sample from N(0, 1) and its asymptotic p-value (Stephens' finite-n argument)."""
    v = np.sort(np.ravel(v))
    n = v.size
    cdf = 0.5 * np.frompyfunc(math.erfc, 1, 1)(-v / math.sqrt(2.0)).astype(np.float64)
    i = np.arange(n)
    dist = float(max(np.max((i + 1) / n - cdf), np.max(cdf - i / n)))
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * dist
    p = 2.0 * sum((-1) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam) for k in range(1, 101))
    return dist, min(max(p, 0.0), 1.0)


def normal_stream_stats(z, g):
    """What a stream of standard normals z [iterations, rungs, W, RW] (RW even) has to look like, as numbers that are
    standard-normal z-scores when it does.  g = mh_pair_rows(RW): walkers w and w + g share a Philox call (g = 0: nobody
    does - the neighbours w, w + 1 are compared instead)."""
    z = np.asarray(z, dtype=np.float64)
    n_it, _, W, RW = z.shape
    n = z.size
    s = dict(n=n)
    s["ks_d"], s["ks_p"] = _ks_normal(z)
    z2 = z * z
    s["z_mean"] = float(np.mean(z) * math.sqrt(n))
    s["z_var"] = float((np.mean(z2) - 1.0) / math.sqrt(2.0 / n))
    s["z_m3"] = float(np.mean(z2 * z) / math.sqrt(15.0 / n))
    s["z_m4"] = float((np.mean(z2 * z2) - 3.0) / math.sqrt(96.0 / n))
    x, y = z[..., 0::2], z[..., 1::2]
    s["z_pair"] = _corr_z(x, y)                                          # the two outputs of one Box-Muller pair
    s["z_adjacent"] = _corr_z(z[..., :-2], z[..., 2:])                   # pairs pr and pr + 1, like output with like
    d = g or 1
    lo = np.array([w for w in range(W) if not (w & d) and w + d < W])
    s["z_partner"] = _corr_z(z[:, :, lo], z[:, :, lo + d])
    s["z_partner_sq"] = _corr_z(z2[:, :, lo], z2[:, :, lo + d])
    s["equal_fraction"] = float(np.mean(z[:, :, lo] == z[:, :, lo + d]))
    s["z_iterations"] = _corr_z(z[:-1], z[1:])
    for name, cut in (("gt3", 3.0), ("gt4", 4.0)):                       # tail counts against the normal's, Poisson
        lam = n * math.erfc(cut / math.sqrt(2.0))
        cnt = int(np.count_nonzero(np.abs(z) > cut))
        s["n_" + name], s["exp_" + name], s["z_" + name] = cnt, lam, (cnt - lam) / math.sqrt(lam)
    for name, v in (("x", x), ("y", y)):                                 # sign symmetry of each output
        pos, neg = int(np.count_nonzero(v > 0)), int(np.count_nonzero(v < 0))
        s["z_sign_" + name] = (pos - neg) / math.sqrt(pos + neg)
    return s


def normal_stream_violations(s):
    """The bars on normal_stream_stats: |z| < 5 for every z-score, KS p > 1e-6, no equal values between partners.
    Returns the names of the statistics that miss theirs."""
    bad = [k for k, v in s.items() if k.startswith("z_") and not abs(v) < 5.0]
    if not s["ks_p"] > 1e-6:
        bad.append("ks_p")
    if s["equal_fraction"] != 0.0:
        bad.append("equal_fraction")
    return bad
