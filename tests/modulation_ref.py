"""numpy restatement of ev_modulation (include/emojivoice.h): the modulation spectrum of a contour, pooled over its runs of
valid frames, and the peak of every band.  It runs in float64, adding in the device's order, and, with ``dtype=np.longdouble``, in extended
precision; both take the values as the float64 numbers they are.

For a contour v of F frames, n = len (F without lengths; n < 0 or n > F: zeros everywhere), mask m (None: ones):
    valid       f < n, m[f] != 0 and v[f] finite;  dropped: f < n, m[f] != 0 and v[f] not finite (counted, invalid for everything else)
    runs        maximal stretches of valid frames inside [0, n);  a run of l >= min_run frames is analysed;  nothing crosses a gap
    grid        nu_j = nu0 + j dnu, one rounded product and one rounded sum IN FLOAT64 under either dtype (the grid is an input of the arithmetic)
    one run     tc = t - (l - 1) / 2;  m = sum u / l;  b = sum(tc u) / ((l (l l - 1)) / 12);  r = (u - m) - b tc;
                w = 0.5 - 0.5 cospi((2 t + 1) / l);  sw = sum w;  ph = nu_j t, ONE float64 product, reduced modulo 1 exactly (ph - floor(ph) is
                exact) before the trigonometric call;  xr = sum w r cospi(2 ph), xi = sum w r sinpi(2 ph);  P = 2 (xr^2 + xi^2) / (sw sw);
                resolved: nu_j l >= min_cycles, one float64 product under either dtype
    pooling     W_j = sum l over the runs resolving j;  Pm_j = (sum l P_j) / W_j or 0;  stat 0 = sum sum r^2 / frames analysed;
                stat 1 = sum l b / frames analysed
    peak        per band [j_lo, j_hi): candidates 1 <= j <= NM - 2 with W_{j-1}, W_j, W_{j+1} > 0, Pm_{j-1}, Pm_{j+1} > 0, Pm_j > Pm_{j-1},
                Pm_j >= Pm_{j+1};  the largest, the lowest j among equals;  a, c, e = log Pm;  den = (a - 2 c) + e;  off = den < 0 ?
                (0.5 (a - e)) / den : 0;  pw = exp(c - (0.25 (a - e)) off);  {nu0 + (j + off) dnu, sqrt(2 pw), band mean over W_j > 0, pw / mean}
    count       0 valid 1 dropped 2 analysed runs 3 analysed frames 4 + band the peak index, -1 without a candidate
    sums        per run ``wave_sum``: term t in slot t mod 64, ascending from +0.0, xor tree 32 .. 1.  xr, xi ``chain_sum``: four chains t mod 4
                ascending from +0.0, a rounded product added by a rounded sum (the device uses no fused multiply-add), ((s0 + s1) + s2) + s3.
                Over the runs: from +0.0 in ascending order.
"""
from itertools import groupby

import numpy as np

TOL = 1e-9                               # the project's float64 margin: |device - restatement| <= TOL max(|restatement|, 1)
MARGIN = 1e-6                            # the least relative gap a peak choice or a local-peak comparison of a GPU case may rest on
COUNT = ("valid", "dropped", "runs", "frames")
MUTANTS = ("no_detrend", "asymmetric_window", "pooling_weight", "linear_parabola", "resolution_off_by_one_run", "peak_without_local_maximum")
GARBAGE = float("nan")                   # what lies behind a row's length, under a mask of ones: reading it would count a dropped frame


def err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0))) if got.size else 0.0


def wave_sum(terms, dtype=np.float64):
    """One wave's order over the terms of one sum (the module docstring's ``sums``)."""
    terms = np.asarray(terms, dtype=dtype)
    n = len(terms)
    R = max(-(-n // 64), 1)
    buf = np.zeros(R * 64, dtype=dtype)
    buf[:n] = terms
    acc = np.zeros(64, dtype=dtype)
    for r in range(R):
        acc = acc + buf[r * 64: (r + 1) * 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return acc[0]


def chain_sum(terms, dtype=np.float64):
    """terms (l, NM) -> (NM,): four chains t mod 4 in ascending t, joined as ((s0 + s1) + s2) + s3."""
    l, NM = terms.shape
    R = -(-l // 4)
    buf = np.zeros((R * 4, NM), dtype=dtype)
    buf[:l] = terms
    acc = np.zeros((4, NM), dtype=dtype)
    for r in range(R):
        acc = acc + buf[4 * r: 4 * r + 4]
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def grid(nu0, dnu, NM):
    return np.float64(nu0) + np.arange(NM, dtype=np.float64) * np.float64(dnu)


_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def _pi(dtype):
    return dtype(np.pi) if dtype is np.float64 else _PI_LD


def analyse_run(u, nu, dtype=np.float64, mutant=None):
    """One run u (l,) float64 -> (P (NM,), b, sum r^2, and the pieces a brute-force check reads: r, w)."""
    l = len(u)
    u = np.asarray(u, dtype=np.float64).astype(dtype)
    t = np.arange(l)
    tc = (t.astype(np.float64) - np.float64(l - 1) / 2.0).astype(dtype)
    m = wave_sum(u, dtype) / dtype(l)
    b = wave_sum(tc * u, dtype) / (dtype(l * (l * l - 1)) / dtype(12.0))
    if mutant == "no_detrend":
        b = dtype(0.0)
    r = (u - m) - b * tc
    wx = ((2 * t).astype(np.float64) if mutant == "asymmetric_window" else (2 * t + 1).astype(np.float64)).astype(dtype) / dtype(l)
    w = dtype(0.5) - dtype(0.5) * np.cos(_pi(dtype) * wx)
    sw = wave_sum(w, dtype)
    s2 = wave_sum(r * r, dtype)
    x = w * r
    ph = nu[None, :] * t.astype(np.float64)[:, None]                     # (l, NM): one float64 product
    fr = (ph - np.floor(ph)).astype(dtype)                               # exact
    ang = dtype(2.0) * _pi(dtype) * fr
    xr = chain_sum(x[:, None] * np.cos(ang), dtype)
    xi = chain_sum(x[:, None] * np.sin(ang), dtype)
    P = dtype(2.0) * (xr * xr + xi * xi) / (sw * sw)
    return P, b, s2, r, w


def runs_of(valid):
    """[(start, length)] of the maximal stretches of True."""
    out, f = [], 0
    for val, grp in groupby(bool(x) for x in valid):
        l = sum(1 for _ in grp)
        if val:
            out.append((f, l))
        f += l
    return out


def contour(v, mask, n, nu0, dnu, NM, min_run, min_cycles, bands=(), dtype=np.float64, mutant=None):
    """One contour -> {"spec" (NM,) in ``dtype``, "weight" (NM,) int32, "peak" (NBAND, 4) in ``dtype``, "stat" (2,), "count" (4 + NBAND,) int32}."""
    v = np.asarray(v, dtype=np.float64)
    F, NB = len(v), len(bands)
    out = {"spec": np.zeros(NM, dtype=dtype), "weight": np.zeros(NM, np.int32), "peak": np.zeros((NB, 4), dtype=dtype), "stat": np.zeros(2, dtype=dtype),
           "count": np.zeros(4 + NB, np.int32)}
    n = int(n)
    if n < 0 or n > F:
        return out
    vv = v[:n]
    on = np.ones(n, bool) if mask is None else np.asarray(mask)[:n] != 0
    fin = np.isfinite(vv)
    valid, dropped = on & fin, on & ~fin
    nu = grid(nu0, dnu, NM)
    runs = [(s, l) for s, l in runs_of(valid) if l >= min_run]
    lens = [l for _, l in runs]
    acc, W = np.zeros(NM, dtype=dtype), np.zeros(NM, np.int64)
    q, lb, frames = dtype(0.0), dtype(0.0), 0
    for i, (s, l) in enumerate(runs):
        P, b, s2, _, _ = analyse_run(vv[s: s + l], nu, dtype, mutant)
        lr = lens[i - 1] if mutant == "resolution_off_by_one_run" else l
        res = nu * np.float64(lr) >= np.float64(min_cycles)              # one float64 product
        wt = 1 if mutant == "pooling_weight" else l
        acc = np.where(res, acc + dtype(wt) * P, acc)
        W = W + np.where(res, wt, 0)
        q, lb, frames = q + s2, lb + dtype(l) * b, frames + l
    Pm = np.where(W > 0, acc / np.maximum(W, 1).astype(dtype), dtype(0.0))
    out["spec"], out["weight"] = Pm, W.astype(np.int32)
    if frames:
        out["stat"][0], out["stat"][1] = q / dtype(frames), lb / dtype(frames)
    out["count"][:4] = int(valid.sum()), int(dropped.sum()), len(runs), frames
    for k, (jlo, jhi) in enumerate(bands):
        best = -1
        for j in range(jlo, jhi):
            if mutant == "peak_without_local_maximum":
                ok = 1 <= j <= NM - 2 and W[j - 1] > 0 and W[j] > 0 and W[j + 1] > 0 and Pm[j - 1] > 0 and Pm[j + 1] > 0 and Pm[j] > 0
            else:
                ok = candidate(Pm, W, j)
            if ok and (best < 0 or Pm[j] > Pm[best]):
                best = j
        out["count"][4 + k] = best
        if best < 0:
            continue
        inb = [j for j in range(jlo, jhi) if W[j] > 0]
        bs = dtype(0.0)
        for j in inb:
            bs = bs + Pm[j]
        bm = bs / dtype(len(inb))
        j = best
        if mutant == "linear_parabola":
            a, c, e = Pm[j - 1], Pm[j], Pm[j + 1]
        else:
            a, c, e = np.log(Pm[j - 1]), np.log(Pm[j]), np.log(Pm[j + 1])
        den = (a - dtype(2.0) * c) + e
        off = (dtype(0.5) * (a - e)) / den if den < 0 else dtype(0.0)
        pw = c - (dtype(0.25) * (a - e)) * off
        if mutant != "linear_parabola":
            pw = np.exp(pw)
        out["peak"][k] = (dtype(np.float64(nu0)) + (dtype(j) + off) * dtype(np.float64(dnu)), np.sqrt(dtype(2.0) * pw), bm, pw / bm)
    return out


def candidate(Pm, W, j):
    NM = len(Pm)
    return bool(1 <= j <= NM - 2 and W[j - 1] > 0 and W[j] > 0 and W[j + 1] > 0 and Pm[j - 1] > 0 and Pm[j + 1] > 0 and Pm[j] > Pm[j - 1]
                and Pm[j] >= Pm[j + 1])


def batch(v, mask, lens, nu0, dnu, NM, min_run, min_cycles, bands=(), dtype=np.float64, mutant=None):
    """v (B, K, F) float64, mask (B, K, F) or None, lens (B,) or None -> {"spec" (B, K, NM), "weight", "peak" (B, K, NBAND, 4), "stat" (B, K, 2),
    "count" (B, K, 4 + NBAND)}."""
    v = np.asarray(v, dtype=np.float64)
    B, K, F = v.shape
    rows = [[contour(v[b, k], None if mask is None else mask[b, k], F if lens is None else int(lens[b]), nu0, dnu, NM, min_run, min_cycles, bands,
                     dtype, mutant) for k in range(K)] for b in range(B)]
    return {key: np.stack([np.stack([c[key] for c in row]) for row in rows]) for key in ("spec", "weight", "peak", "stat", "count")}


def decision_margin(case, res=None):
    """The least relative gap |x - y| / max(x, y) that any decision of the case's peaks rests on, in the float64 restatement: every evaluated
    comparison Pm_j > Pm_{j-1} and Pm_j >= Pm_{j+1} of a j inside a band whose other conditions hold, and for every band the gap between the
    largest candidate and the next.  A spectrum value that is positive and under 1e-250 (a zero that rounding lifted) counts as a gap of 0.
    inf where nothing is decided."""
    v, mask, lens, kw = case
    res = batch(v, mask, lens, **kw) if res is None else res
    worst = np.inf
    NM = kw["NM"]
    for b in range(res["spec"].shape[0]):
        for k in range(res["spec"].shape[1]):
            Pm, W = res["spec"][b, k].astype(np.float64), res["weight"][b, k]
            if ((Pm > 0) & (Pm < 1e-250)).any():
                return 0.0
            for jlo, jhi in kw["bands"]:
                cands = []
                for j in range(max(jlo, 1), min(jhi, NM - 1)):
                    if not (W[j - 1] > 0 and W[j] > 0 and W[j + 1] > 0 and Pm[j - 1] > 0 and Pm[j + 1] > 0):
                        continue
                    for o in (Pm[j - 1], Pm[j + 1]):
                        worst = min(worst, abs(Pm[j] - o) / max(Pm[j], o)) if max(Pm[j], o) > 0 else worst
                    if candidate(Pm, W, j):
                        cands.append(Pm[j])
                cands.sort(reverse=True)
                if len(cands) > 1:
                    worst = min(worst, (cands[0] - cands[1]) / cands[0])
    return float(worst)


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
CONTOURS = ("sinusoid", "two_sinusoids", "walk", "constant", "integers", "zeros")
MASKS = ("ones", "runs", "alternating", "zeros", "exact", "short")
GRID = dict(nu0=1.0 / 64.0, dnu=1.0 / 256.0)                            # exact in binary: nu_j l lands on integers (the resolution boundary)
GRID128 = dict(nu0=1.0 / 128.0, dnu=0.00387)                           # 128 frequencies up to 0.4993 cycles per frame, under the limit of 0.5
NMS = (1, 3, 64, 65, 128)
AUDIO_RATE = 22050.0 / 256.0                                            # audio.modulation's default frame rate; its default grid is 1 .. 16 Hz by 0.125
AUDIO_KW = dict(nu0=1.0 / AUDIO_RATE, dnu=0.125 / AUDIO_RATE, NM=121, min_run=18, min_cycles=2.0, bands=((24, 89), (8, 57)))


def grid_for(NM):
    return GRID128 if NM > 65 else GRID


def make_contour(kind, F, g):
    t = np.arange(F, dtype=np.float64)
    if kind == "sinusoid":                                               # on a line, with a little noise: the floor of the spectrum is not rounding
        return 40.0 + 0.03 * t + 0.5 * np.sin(2 * np.pi * (g.uniform(0.03, 0.2) * t + g.uniform())) + 1e-3 * g.standard_normal(F)
    if kind == "two_sinusoids":
        return (0.5 * np.sin(2 * np.pi * (0.0625 * t + g.uniform())) + 0.3 * np.sin(2 * np.pi * (0.171 * t + g.uniform())) + 1e-3 * g.standard_normal(F))
    if kind == "walk":
        return 100.0 + np.cumsum(g.standard_normal(F))
    if kind == "constant":                                               # 0.5: every sum is exact, r and the spectrum are exactly 0
        return np.full(F, 0.5)
    if kind == "integers":                                               # ties and plateaus
        return np.repeat(g.integers(-3, 4, size=F).astype(np.float64), g.integers(1, 4, size=F))[:F]
    return np.where(g.integers(0, 2, size=F) > 0, 0.0, -0.0)             # +0.0 and -0.0 mixed


def make_mask(kind, F, g, min_run):
    if kind == "ones":
        return np.ones(F, np.uint8)
    if kind == "zeros":
        return np.zeros(F, np.uint8)
    if kind == "alternating":
        return (np.arange(F) % 2 == 0).astype(np.uint8)
    if kind in ("exact", "short"):                                       # one run of exactly min_run (min_run - 1) frames, and a long one behind it
        out = np.zeros(F, np.uint8)
        l = min_run if kind == "exact" else min_run - 1
        out[2: 2 + l] = 1
        out[2 + l + 3:] = 255
        return out
    out, f, val = np.zeros(F, np.uint8), 0, int(g.integers(0, 2))
    while f < F:                                                         # random runs; a non-zero byte is any of 1 .. 255
        l = int(g.integers(1, 48 if val else 5))
        out[f: f + l] = int(g.integers(1, 256)) if val else 0
        f, val = f + l, 1 - val
    return out


def make(B, K, F, seed, min_run, lens=None, masked=True, shift=0):
    """(v (B, K, F), mask or None): contour kinds and mask kinds cycle over (b, k) with periods 6 and 6 (the mask advances once more per cycle of
    the contours, so every pair comes up); GARBAGE behind each length."""
    g = np.random.default_rng(seed)
    v = np.zeros((B, K, F))
    mask = np.zeros((B, K, F), np.uint8) if masked else None
    for b in range(B):
        for k in range(K):
            i = b * K + k + shift
            v[b, k] = make_contour(CONTOURS[i % 6], F, g)
            if masked:
                mask[b, k] = make_mask(MASKS[(i // 6 + i) % 6], F, g, min_run)
        if lens is not None and 0 <= lens[b] <= F:
            v[b, :, lens[b]:] = GARBAGE
            if masked:
                mask[b, :, lens[b]:] = 1
    return v, mask


SHAPES = (3, 63, 64, 65, 255, 256, 257, 1023)


def bands_for(NM, NB):
    if NB == 0:
        return ()
    if NB == 1:
        return ((0, NM),)
    return ((0, 1), (0, NM), (NM // 4, NM // 2 + 1), (NM - 1, NM))      # the first and the last can hold no candidate


def cases():
    """name -> (v (B, K, F), mask or None, lens or None, kw of ``batch``): every case of the device test that needs no device to state."""
    out = {}
    for i, F in enumerate(SHAPES):
        lens = [F, max(F - 1, 1), (F + 1) // 2]
        mr = 3 if F == 3 else 4
        NM = NMS[i % 5]
        v, m = make(3, 4, F, seed=300 + i, min_run=mr, lens=lens, shift=i)
        out[f"F{F}"] = (v, m, lens, dict(grid_for(NM), NM=NM, min_run=mr, min_cycles=1.5, bands=bands_for(NM, (0, 1, 4)[i % 3])))
    g = np.random.default_rng(7)
    out["run4096"] = (make_contour("sinusoid", 4096, g)[None, None], None, None, dict(GRID128, NM=128, min_run=4096, min_cycles=2.0, bands=bands_for(128, 4)))
    # a run of 32 frames: nu_j l = 32 / 64 + j / 8 is exactly min_cycles = 2 at j = 12, resolved from there on; the run of 40 resolves from j = 9 on
    v = np.stack([make_contour(k, 80, g) for k in ("walk", "two_sinusoids")])[None]
    m = np.zeros((1, 2, 80), np.uint8)
    m[:, :, 3: 35] = 1
    m[:, :, 38: 78] = 7
    out["boundary"] = (v, m, None, dict(GRID, NM=64, min_run=8, min_cycles=2.0, bands=bands_for(64, 4)))
    # non-finite values under a non-zero mask are dropped and counted and split a run; under a zero mask they are nothing
    F = 200
    v, m = make(2, 2, F, seed=16, min_run=4)
    m[:] = 1
    v[0, 0] = make_contour("walk", F, g)
    for f, x in ((5, np.nan), (70, np.inf), (71, -np.inf), (128, np.nan), (199, np.inf), (150, np.nan)):
        v[0, 0, f] = x
    m[0, 0, 150] = 0
    v[1, 1, :] = np.nan                                                  # every frame dropped
    out["nonfinite"] = (v, m, None, dict(GRID, NM=65, min_run=4, min_cycles=1.5, bands=bands_for(65, 1)))
    lens = [0, 1, 65, 66, -1]
    v, m = make(5, 2, 65, seed=12, min_run=4, lens=lens)
    m[:, 0] = 1
    out["lengths"] = (v, m, lens, dict(GRID, NM=64, min_run=4, min_cycles=1.5, bands=bands_for(64, 4)))
    v, _ = make(2, 2, 257, seed=13, min_run=4, masked=False)
    out["null-mask-null-lengths"] = (v, None, None, dict(GRID, NM=3, min_run=4, min_cycles=0.0, bands=bands_for(3, 1)))
    # the sinusoid sits on the grid at j = 20 (nu = 1 / 64 + 20 / 256 = 0.09375): a band of that j alone has both neighbours outside it
    t = np.arange(300, dtype=np.float64)
    v = (12.0 + 0.01 * t + 0.4 * np.sin(2 * np.pi * (0.09375 * t + 0.1)) + 1e-3 * g.standard_normal(300))[None, None]
    out["neighbours-outside"] = (v, None, None, dict(GRID, NM=64, min_run=4, min_cycles=2.0, bands=((20, 21), (0, 1), (63, 64), (19, 22))))
    # three runs of unequal length: what the pooling mutants and the resolution mutant move
    v = np.stack([make_contour("two_sinusoids", 160, g), make_contour("walk", 160, g)])[None]
    m = np.zeros((1, 2, 160), np.uint8)
    m[:, :, 0: 20] = 1
    m[:, :, 25: 65] = 1
    m[:, :, 70: 160] = 1
    out["three-runs"] = (v, m, None, dict(GRID, NM=64, min_run=4, min_cycles=2.0, bands=((0, 64),)))
    # the contour of the identities: alone, inside a batch, at another k, as a prefix
    g = np.random.default_rng(21)
    c, cm = make_contour("walk", 257, g), make_mask("runs", 257, g, 4)
    out["identity"] = (c[None, None], cm[None, None], None, dict(GRID, NM=65, min_run=4, min_cycles=1.5, bands=((0, 65), (10, 30))))
    # what audio.modulation is handed: float32 contours, one mask per row, ragged lengths, the default grid and the tremor and rhythm bands
    g = np.random.default_rng(31)
    F, lens = 300, [300, 120, 7]
    v = np.stack([np.stack([make_contour(kind, F, g) for kind in ("sinusoid", "walk")]) for _ in range(3)]).astype(np.float32)
    m = np.stack([make_mask(kind, F, g, 18) for kind in ("runs", "ones", "zeros")])[:, None, :]
    v, m = v.astype(np.float64), np.ascontiguousarray(np.broadcast_to(m, v.shape))
    for b, n in enumerate(lens):
        v[b, :, n:], m[b, :, n:] = GARBAGE, 1
    out["audio"] = (v, m, lens, dict(AUDIO_KW))
    return out


# mutant -> (case, contour (b, k), the output it moves past TOL)
MUTANT_SHOWS = {
    "no_detrend": ("neighbours-outside", (0, 0), "stat"),
    "asymmetric_window": ("identity", (0, 0), "spec"),
    "pooling_weight": ("three-runs", (0, 0), "spec"),
    "linear_parabola": ("identity", (0, 0), "peak"),
    "resolution_off_by_one_run": ("three-runs", (0, 0), "weight"),
    "peak_without_local_maximum": ("three-runs", (0, 1), "count"),
}
