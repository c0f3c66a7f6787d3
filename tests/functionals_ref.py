"""numpy restatement of ev_functionals (include/emojivoice.h): the eGeMAPS functionals of a contour.  It runs in float64
and, with ``dtype=np.longdouble``, in extended precision; both take the values as the float64 numbers they are.

For a contour v of F frames, n = len (F without lengths; n < 0 or n > F: zeros everywhere), mask m (None: ones), fractions q:
    valid       f < n, m[f] != 0 and v[f] finite;  dropped: f < n, m[f] != 0 and v[f] not finite (counted, invalid for everything else)
    u, g        the valid values in ascending frame order and their frames;  pair i = (u_i, u_{i+1}) is adjacent when g_{i+1} = g_i + 1
    moments     mean = sum u / k;  sd = sqrt(sum (u - mean)^2 / k)
    order       s = u sorted ascending;  min = s_0, max = s_{k-1};  p = q (k - 1) (ONE rounded product), j = floor(p), t = p - j,
                s_j + t (s_{min(j+1, k-1)} - s_j)
    parts       class of pair i: +1 adjacent and u_{i+1} > u_i, -1 adjacent and u_{i+1} < u_i, else 0;  a rising (falling) part is a maximal run of
                consecutive pairs of class +1 (-1), from index a to index e of u, with the slope (u_e - u_a) / (e - a);  mean and population sd
                of the slopes over the parts, two passes
    peaks       both pairs of i adjacent, u_i > u_{i-1} and u_i >= u_{i+1}
    runs, gaps  maximal stretches of valid / not valid frames inside [0, n), leading and trailing gaps included;  N stretches, S1 = sum l,
                S2 = sum l^2:  mean = S1 / N,  sd = sqrt(N S2 - S1 S1) / N  (integers under the root)
    stat        0 mean 1 sd 2 min 3 max 4 rise_mean 5 rise_sd 6 fall_mean 7 fall_sd 8 run_mean 9 run_sd 10 gap_mean 11 gap_sd 12 + r percentile r
    count       0 k 1 dropped 2 rising parts 3 falling parts 4 peaks 5 runs 6 gaps 7 adjacent pairs;  a statistic over no terms is 0
    sums        ``slot_sum``: term i belongs to slot i mod 256, a slot adds its terms in ascending i from +0.0, the slots are reduced by an xor tree
                (offsets 32 .. 1) inside each group of 64, the four group sums are added in ascending order.  A part's slope (or its squared
                deviation) sits at the index of the part's LAST pair, +0.0 elsewhere.

Besides the outputs every contour reports what the comparison on the device needs to know: the percentile indices j and whether t == 0 (such a
percentile is one of the values and is compared as a value).
"""
from itertools import groupby

import numpy as np

TOL = 1e-9                               # the project's float64 margin: |device - restatement| <= TOL max(|restatement|, 1)
STAT = ("mean", "sd", "min", "max", "rise_mean", "rise_sd", "fall_mean", "fall_sd", "run_mean", "run_sd", "gap_mean", "gap_sd")
COUNT = ("valid", "dropped", "rising_parts", "falling_parts", "peaks", "runs", "gaps", "adjacent_pairs")
MUTANTS = ("percentile_nearest", "slope_per_pair", "adjacency_ignored", "peak_strict", "sample_sd", "gaps_inner_only", "dropped_is_valid_for_runs")
GARBAGE = float("nan")                   # what lies behind a row's length, under a mask of ones: reading it would count a dropped frame
Q3 = (0.2, 0.5, 0.8)
Q16 = (0.0, 1.0, 0.5, 0.2, 0.8, 0.05, 0.95, 0.25, 0.75, 1.0 / 3.0, 0.999, 0.001, 0.1, 0.9, 0.6, 0.4)
HAND = (1.0, 2.0, 3.0, 3.0, 2.0, 5.0, 1.0, 1.0, 4.0)


def err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0))) if got.size else 0.0


def slot_sum(terms, dtype=np.float64):
    """The device's order over the terms of one sum (the module docstring's ``sums``)."""
    terms = np.asarray(terms, dtype=dtype)
    n = len(terms)
    R = max(-(-n // 256), 1)
    buf = np.zeros(R * 256, dtype=dtype)
    buf[:n] = terms
    acc = np.zeros(256, dtype=dtype)
    for r in range(R):
        acc = acc + buf[r * 256: (r + 1) * 256]
    acc = acc.reshape(4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return ((acc[0, 0] + acc[1, 0]) + acc[2, 0]) + acc[3, 0]


def stretches(flags):
    """(lengths of the runs of True, lengths of the runs of False, is the first stretch a gap, is the last one) of a 1-D bool array."""
    runs, gaps = [], []
    for val, grp in groupby(bool(f) for f in flags):
        (runs if val else gaps).append(sum(1 for _ in grp))
    return runs, gaps, bool(len(flags)) and not flags[0], bool(len(flags)) and not flags[-1]


def _length_stats(lengths, dtype):
    N, S1, S2 = len(lengths), sum(lengths), sum(l * l for l in lengths)
    if not N:
        return dtype(0), dtype(0)
    return dtype(S1) / dtype(N), np.sqrt(dtype(N * S2 - S1 * S1)) / dtype(N)


def parts(u, adj, per_pair=False):
    """[(class, a, e)] of the rising and falling parts of u under the pairs' adjacency, in ascending order; the part's last pair is e - 1."""
    k = len(u)
    cls = np.where(adj, (u[1:] > u[:-1]).astype(int) - (u[1:] < u[:-1]).astype(int), 0) if k > 1 else np.zeros(0, int)
    out, i = [], 0
    while i < k - 1:
        c = int(cls[i])
        if c == 0:
            i += 1
            continue
        a = i
        while not per_pair and i + 1 < k - 1 and cls[i + 1] == c:
            i += 1
        out.append((c, a, i + 1))
        i += 1
    return out


def contour(v, mask, n, q, dtype=np.float64, mutant=None):
    """One contour -> (stat (12 + NQ,) in ``dtype``, count (8,) int32, j (NQ,) int64: the percentile indices, -1 without a valid frame, t0 (NQ,)
    bool: t == 0)."""
    v = np.asarray(v, dtype=np.float64)
    F, NQ = len(v), len(q)
    stat, count = np.zeros(12 + NQ, dtype=dtype), np.zeros(8, np.int32)
    js, t0 = np.full(NQ, -1, np.int64), np.zeros(NQ, bool)
    n = int(n)
    if n < 0 or n > F:
        return stat, count, js, t0
    vv = v[:n]
    on = np.ones(n, bool) if mask is None else np.asarray(mask)[:n] != 0
    fin = np.isfinite(vv)
    valid, dropped = on & fin, on & ~fin
    g = np.nonzero(valid)[0]
    u = vv[g].astype(dtype)
    k = len(u)
    count[0], count[1] = k, int(dropped.sum())
    # ---- runs and gaps, from the frames' flags
    runs, gaps, lead, trail = stretches(valid | dropped if mutant == "dropped_is_valid_for_runs" else valid)
    if mutant == "gaps_inner_only":
        gaps = gaps[1:] if lead else gaps
        gaps = gaps[:-1] if trail and gaps else gaps
    count[5], count[6] = len(runs), len(gaps)
    stat[8], stat[9] = _length_stats(runs, dtype)
    stat[10], stat[11] = _length_stats(gaps, dtype)
    if not k:
        return stat, count, js, t0
    # ---- moments
    mean = slot_sum(u, dtype) / dtype(k)
    d = u - mean
    stat[0] = mean
    stat[1] = np.sqrt(slot_sum(d * d, dtype) / dtype(max(k - 1, 1) if mutant == "sample_sd" else k))
    # ---- order statistics
    s = np.sort(u)
    stat[2], stat[3] = s[0], s[k - 1]
    for r, qr in enumerate(q):
        p = dtype(qr) * dtype(k - 1)
        j = int(np.floor(p))
        t = p - dtype(j)
        js[r], t0[r] = j, t == 0
        if mutant == "percentile_nearest":
            stat[12 + r] = s[min(int(np.floor(p + dtype(0.5))), k - 1)]
        else:
            sj = s[j]
            stat[12 + r] = sj + t * (s[min(j + 1, k - 1)] - sj)
    # ---- parts and peaks
    adj = g[1:] == g[:-1] + 1
    if mutant == "adjacency_ignored":
        adj = np.ones(k - 1, bool)
    count[7] = int(adj.sum())
    ps = parts(u, adj, per_pair=mutant == "slope_per_pair")
    for sign, at in ((1, 4), (-1, 6)):
        mine = [(a, e) for c, a, e in ps if c == sign]
        count[2 if sign > 0 else 3] = len(mine)
        if mine:
            terms = np.zeros(k - 1, dtype=dtype)
            for a, e in mine:
                terms[e - 1] = (u[e] - u[a]) / dtype(e - a)
            m = slot_sum(terms, dtype) / dtype(len(mine))
            dev = np.zeros(k - 1, dtype=dtype)
            for a, e in mine:
                x = terms[e - 1] - m
                dev[e - 1] = x * x
            stat[at], stat[at + 1] = m, np.sqrt(slot_sum(dev, dtype) / dtype(len(mine)))
    peaks = 0
    for i in range(1, k - 1):
        after = u[i] > u[i + 1] if mutant == "peak_strict" else u[i] >= u[i + 1]
        peaks += bool(adj[i - 1] and adj[i] and u[i] > u[i - 1] and after)
    count[4] = peaks
    return stat, count, js, t0


def slopes(v, mask=None, n=None):
    """(rising slopes, falling slopes) of one contour, in ascending order of the parts: what the hand case states."""
    v = np.asarray(v, dtype=np.float64)
    n = len(v) if n is None else n
    valid = (np.ones(n, bool) if mask is None else np.asarray(mask)[:n] != 0) & np.isfinite(v[:n])
    g = np.nonzero(valid)[0]
    u = v[:n][g]
    ps = parts(u, g[1:] == g[:-1] + 1)
    return [float((u[e] - u[a]) / (e - a)) for c, a, e in ps if c > 0], [float((u[e] - u[a]) / (e - a)) for c, a, e in ps if c < 0]


def batch(v, mask, lens, q, dtype=np.float64, mutant=None):
    """v (B, K, F) float64, mask (B, K, F) or None, lens (B,) or None, q fractions -> {"stat" (B, K, 12 + NQ) in ``dtype``, "count" (B, K, 8)
    int32, "j" (B, K, NQ) int64, "t0" (B, K, NQ) bool}."""
    v = np.asarray(v, dtype=np.float64)
    B, K, F = v.shape
    NQ = len(q)
    out = {"stat": np.zeros((B, K, 12 + NQ), dtype=dtype), "count": np.zeros((B, K, 8), np.int32), "j": np.full((B, K, NQ), -1, np.int64),
           "t0": np.zeros((B, K, NQ), bool)}
    for b in range(B):
        n = F if lens is None else int(lens[b])
        for k in range(K):
            out["stat"][b, k], out["count"][b, k], out["j"][b, k], out["t0"][b, k] = contour(v[b, k], None if mask is None else mask[b, k], n, q,
                                                                                             dtype, mutant)
    return out


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
CONTOURS = ("walk", "integers", "constant", "zeros", "ramp")
MASKS = ("ones", "runs", "alternating", "zeros")


def make_contour(kind, F, g):
    if kind == "walk":
        return 100.0 + np.cumsum(g.standard_normal(F))
    if kind == "integers":                                               # ties and plateaus
        return np.repeat(g.integers(-3, 4, size=F).astype(np.float64), g.integers(1, 4, size=F))[:F]
    if kind == "constant":
        return np.full(F, 0.1)
    if kind == "zeros":                                                  # +0.0 and -0.0 mixed: equal values, no part, no peak
        return np.where(g.integers(0, 2, size=F) > 0, 0.0, -0.0)
    return -np.cumsum(g.uniform(0.5, 1.5, size=F))                       # a monotone ramp with uneven steps: ONE falling part


def make_mask(kind, F, g):
    if kind == "ones":
        return np.ones(F, np.uint8)
    if kind == "zeros":
        return np.zeros(F, np.uint8)
    if kind == "alternating":
        return (np.arange(F) % 2 == 0).astype(np.uint8)
    out, f, val = np.zeros(F, np.uint8), 0, int(g.integers(0, 2))
    while f < F:                                                         # random runs; a non-zero byte is any of 1 .. 255
        l = int(g.integers(1, 12 if val else 5))
        out[f: f + l] = int(g.integers(1, 256)) if val else 0
        f, val = f + l, 1 - val
    return out


def make(B, K, F, seed, lens=None, masked=True, shift=0):
    """(v (B, K, F), mask or None): contour kinds and mask kinds cycle over (b, k) with coprime periods 5 and 4; GARBAGE behind each length."""
    g = np.random.default_rng(seed)
    v = np.zeros((B, K, F))
    mask = np.zeros((B, K, F), np.uint8) if masked else None
    for b in range(B):
        for k in range(K):
            i = b * K + k + shift
            v[b, k] = make_contour(CONTOURS[i % 5], F, g)
            if masked:
                mask[b, k] = make_mask(MASKS[(i // 5 + i) % 4], F, g)
        if lens is not None and 0 <= lens[b] <= F:
            v[b, :, lens[b]:] = GARBAGE
            if masked:
                mask[b, :, lens[b]:] = 1
    return v, mask


SHAPES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)


def cases():
    """name -> (v (B, K, F), mask or None, lens or None, q): every case of the device test that needs no device to state."""
    out = {}
    for i, F in enumerate(SHAPES):
        lens = [F, max(F - 1, 1), (F + 1) // 2]
        v, m = make(3, 4, F, seed=100 + i, lens=lens, shift=i)
        out[f"F{F}"] = (v, m, lens, Q3)
    g = np.random.default_rng(7)
    out["ramp4096"] = (make_contour("ramp", 4096, g)[None, None], np.ones((1, 1, 4096), np.uint8), None, Q16)
    lens = [516, 400, 77]
    v, m = make(3, 20, 516, seed=11, lens=lens)
    out["batch516"] = (v, m, lens, Q3)
    lens = [0, 1, 65, 66, -1]
    v, m = make(5, 2, 65, seed=12, lens=lens)
    m[:, 0] = 1
    out["lengths"] = (v, m, lens, Q3)
    v, _ = make(2, 2, 257, seed=13, masked=False)
    out["null-mask-null-lengths-nq0"] = (v, None, None, ())
    v, m = make(2, 3, 255, seed=14, shift=1)
    out["nq1"] = (v, m, None, (0.5,))
    v, m = make(2, 3, 257, seed=15, shift=2)
    out["nq16"] = (v, m, [257, 130], Q16)
    # non-finite values under a non-zero mask are dropped and counted: they break adjacency and split a run; under a zero mask they are nothing
    F = 130
    v, m = make(2, 2, F, seed=16)
    m[:] = 1
    v[0, 0] = 50.0 + np.cumsum(g.standard_normal(F))
    for f, x in ((5, np.nan), (40, np.inf), (41, -np.inf), (64, np.nan), (129, np.inf), (90, np.nan)):
        v[0, 0, f] = x
    m[0, 0, 90] = 0
    v[1, 1, :] = np.nan                                                  # every frame dropped: k = 0, one gap
    out["nonfinite"] = (v, m, None, Q3)
    hand = np.array(HAND)
    out["hand"] = (hand[None, None], np.ones((1, 1, 9), np.uint8), None, Q3)
    gv = np.array([7.0, 1.0, 2.0, 9.0, 3.0, 4.0, 0.5])
    out["gapped"] = (gv[None, None], np.array([0, 1, 1, 0, 1, 1, 0], np.uint8)[None, None], None, Q3)
    return out


# mutant -> (case, contour (b, k), the output it changes: a name of COUNT or STAT, or "p<r>")
MUTANT_SHOWS = {
    "percentile_nearest": ("hand", (0, 0), "p2"),
    "slope_per_pair": ("hand", (0, 0), "rising_parts"),
    "adjacency_ignored": ("gapped", (0, 0), "rising_parts"),
    "peak_strict": ("hand", (0, 0), "peaks"),
    "sample_sd": ("hand", (0, 0), "sd"),
    "gaps_inner_only": ("gapped", (0, 0), "gaps"),
    "dropped_is_valid_for_runs": ("nonfinite", (0, 0), "runs"),
}


def output(res, bk, name):
    """One named output of a ``batch`` result at contour (b, k)."""
    b, k = bk
    if name in COUNT:
        return res["count"][b, k, COUNT.index(name)]
    return res["stat"][b, k, 12 + int(name[1:]) if name[0] == "p" and name[1:].isdigit() else STAT.index(name)]
