"""numpy float64 restatement of ev_speech_rate (include/emojivoice.h): the power contour in the header's order (64 slots, the xor tree), the exact
rank selection on the bit patterns, the two steps of the segmentation, candidates, dips and nuclei.  ``speech_rate`` is the restatement (array
operations), ``speech_rate(..., plain=True)`` the plain form of the same definition (np.sum, np.sort, Python loops over runs and candidates),
``mutant=`` one wrong reading of the definition each, ``margin`` the least relative distance between the two sides of any comparison a decision
rests on, ``bursts`` the signal generator with its ground truth.  A plain module: imported by the host tests, the GPU tests and the bench tool.
"""
import numpy as np

MUTANTS = ("dip_before", "peak_ge_left", "no_fill", "b_before_a", "rank_plus", "no_mean", "last_never")
PAR = dict(power_floor=1e-12, rank_fraction=0.01, silence_db=25.0, dip_db=2.0, min_pause=8, min_sound=3)
FLOAT_OUTPUTS = ("power", "stat")
SND, RAW, CAND, NUC = 1, 2, 4, 8


def ratios(par):
    """(silence_ratio, dip_ratio) as the host forms them."""
    return 10.0 ** (-par["silence_db"] / 10.0), 10.0 ** (par["dip_db"] / 10.0)


def frames_of(n, L, H):
    return 0 if n < 1 or n > L else -(-n // H)


def window_sum(win):
    sw = 0.0
    for v in np.asarray(win, dtype=np.float64):
        sw = sw + float(v)
    return sw


def frame_matrix(x, n, W, H):
    """(nf, W) float64: s_f[j] = x[f H + H/2 - W/2 + j], zero outside [0, n).  Reads x[:n] only."""
    nf = -(-n // H)
    lo = W // 2 - H // 2
    pad = np.zeros(max(lo, 0) + nf * H + W, dtype=np.float64)
    pad[max(lo, 0): max(lo, 0) + n] = np.asarray(x[:n], dtype=np.float32).astype(np.float64)
    start = np.arange(nf) * H + (max(lo, 0) - lo)
    return pad[start[:, None] + np.arange(W)[None, :]]


def slot_sum(T):
    """Rows of T (nf, W) summed by the 64-slot rule: slot j mod 64 adds its terms in ascending j from +0.0, then the xor tree 32 .. 1."""
    nf, W = T.shape
    G = -(-W // 64)
    Tp = np.zeros((nf, G * 64), dtype=np.float64)
    Tp[:, :W] = T                                                        # (adding +0.0 to a slot changes no bit: a slot is never -0.0)
    Tp = Tp.reshape(nf, G, 64)
    acc = np.zeros((nf, 64), dtype=np.float64)
    for g in range(G):
        acc = acc + Tp[:, g, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def power(x, n, win, H, mutant=None, plain=False):
    """P (nf,) of one row of n samples."""
    w = np.asarray(win, dtype=np.float64)
    S = frame_matrix(x, n, len(w), H)
    if plain:
        sw = np.sum(w)
        m = np.sum(w[None] * S, axis=1) / sw
        return np.sum(w[None] * (S - m[:, None]) ** 2, axis=1) / sw
    sw = window_sum(w)
    m = slot_sum(w[None] * S) / sw
    if mutant == "no_mean":
        m = np.zeros_like(m)
    d = S - m[:, None]
    return slot_sum(w[None] * (d * d)) / sw


def runs_of(flag):
    """[(start, end inclusive, value)] of the maximal runs of equal entries."""
    flag = np.asarray(flag, dtype=bool)
    if len(flag) == 0:
        return []
    cut = np.flatnonzero(np.diff(flag.astype(np.int8))) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut - 1, [len(flag) - 1]])
    return [(int(s), int(e), bool(flag[s])) for s, e in zip(starts, ends)]


def step_a(flag, min_pause):
    out = flag.copy()
    for s, e, v in runs_of(flag):
        if not v and s > 0 and e < len(flag) - 1 and e - s + 1 < min_pause:
            out[s: e + 1] = True
    return out


def step_b(flag, min_sound):
    out = flag.copy()
    for s, e, v in runs_of(flag):
        if v and e - s + 1 < min_sound:
            out[s: e + 1] = False
    return out


def select(P, k, plain):
    """The (k + 1)-th largest of P: on the bit patterns (the restatement) or by np.sort of the values (the plain form)."""
    if plain:
        return float(np.sort(P)[::-1][k])
    bits = np.ascontiguousarray(P).view(np.uint64)
    pre, kk = 0, k
    for bit in range(63, -1, -1):
        c = int(np.count_nonzero((bits >> np.uint64(bit)) == np.uint64(pre >> bit | 1)))
        if c > kk:
            pre |= 1 << bit
        else:
            kk -= c
    return float(np.array([pre], dtype=np.uint64).view(np.float64)[0])


def decide(P, par, voiced=None, mutant=None, plain=False):
    """Everything behind the power of one row -> {"mark" (nf,) uint8, "count" (8,) int32, "stat" (4,) float64, "cand", "dips"}."""
    nf = len(P)
    sil, dipr = ratios(par)
    k = int(np.floor(par["rank_fraction"] * float(nf - 1)))
    if mutant == "rank_plus":
        k = min(k + 1, nf - 1)
    ref = select(P, k, plain)
    thr = ref * sil
    raw = (P > thr) & (P > par["power_floor"])
    if mutant == "no_fill":
        snd = step_b(raw, par["min_sound"])
    elif mutant == "b_before_a":
        snd = step_a(step_b(raw, par["min_sound"]), par["min_pause"])
    else:
        snd = step_b(step_a(raw, par["min_pause"]), par["min_sound"])
    cand = np.zeros(nf, dtype=bool)
    if nf >= 3:
        mid = P[1:-1]
        left = mid >= P[:-2] if mutant == "peak_ge_left" else mid > P[:-2]
        cand[1:-1] = left & (mid >= P[2:]) & (mid > thr) & snd[1:-1]
    cs = [int(c) for c in np.flatnonzero(cand)]
    nuc = np.zeros(nf, dtype=bool)
    dips = []
    for i, c in enumerate(cs):
        if mutant == "dip_before":
            lo, hi = (cs[i - 1] + 1 if i > 0 else 0), c
        else:
            lo, hi = c + 1, (cs[i + 1] if i + 1 < len(cs) else nf)
            if mutant == "last_never" and i + 1 == len(cs):
                hi = lo
        if hi <= lo:
            continue
        d = float(np.min(P[lo:hi]))
        dips.append((c, d))
        if d * dipr <= P[c] and (voiced is None or voiced[c] != 0):
            nuc[c] = True
    pauses, lead, trail = [], 0, 0
    for s, e, v in runs_of(snd):
        if v:
            continue
        if s == 0:
            lead = e - s + 1
        elif e == nf - 1:
            trail = e - s + 1
        else:
            pauses.append(e - s + 1)
    n, S1, S2 = len(pauses), sum(pauses), sum(l * l for l in pauses)
    stat = np.array([ref, thr, S1 / n if n else 0.0, np.sqrt(float(n * S2 - S1 * S1)) / n if n else 0.0], dtype=np.float64)
    count = np.array([nf, int(snd.sum()), n, S1, len(cs), int(nuc.sum()), lead, trail], dtype=np.int32)
    mark = (snd * SND + raw * RAW + cand * CAND + nuc * NUC).astype(np.uint8)
    return {"mark": mark, "count": count, "stat": stat, "cand": cs, "dips": dips}


def rel(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else 0.0


def row_margin(P, par, res):
    """The least relative distance between the two sides of a comparison whose sides are not bit-equal: raw (against thr and the floor), the
    peak rule at every sounding frame above thr, every dip, and ref against its neighbours in rank."""
    nf = len(P)
    _, dipr = ratios(par)
    ref, thr = float(res["stat"][0]), float(res["stat"][1])
    ds = []
    for f in range(nf):
        ds += [rel(P[f], thr), rel(P[f], par["power_floor"])]
        if 1 <= f <= nf - 2 and res["mark"][f] & SND and P[f] > thr:
            ds += [rel(P[f], P[f - 1]), rel(P[f], P[f + 1])]
    for c, d in res["dips"]:
        ds.append(rel(d * dipr, P[c]))
    ds += [rel(ref, v) for v in P]
    ds = [d for d in ds if d > 0.0]
    return min(ds) if ds else 1.0


def speech_rate(x, lens, win, H, par=PAR, voiced=None, mutant=None, plain=False):
    """The outputs of ev_speech_rate for x (B, L) float32 and lens (B,) or None -> {"power" (B, NF), "mark" (B, NF) uint8, "count" (B, 8) int32,
    "stat" (B, 4), "margin" (B,)}."""
    x = np.asarray(x, dtype=np.float32)
    B, L = x.shape
    NF = -(-L // H)
    out = {"power": np.zeros((B, NF)), "mark": np.zeros((B, NF), np.uint8), "count": np.zeros((B, 8), np.int32), "stat": np.zeros((B, 4)),
           "margin": np.ones(B)}
    for b in range(B):
        n = L if lens is None else int(lens[b])
        nf = frames_of(n, L, H)
        if nf == 0:
            continue
        P = power(x[b], n, win, H, mutant, plain)
        res = decide(P, par, None if voiced is None else np.asarray(voiced)[b], mutant, plain)
        out["power"][b, :nf], out["mark"][b, :nf], out["count"][b], out["stat"][b] = P, res["mark"], res["count"], res["stat"]
        out["margin"][b] = row_margin(P, par, res)
    return out


def rel_err(dev, ref):
    """test_gpu_loudness.py's rule: relative to max(|ref|, 1e-9 x the row's largest |ref|), the worst entry."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    r = ref.reshape(ref.shape[0], -1)
    scale = np.maximum(np.abs(r), 1e-9 * np.abs(r).max(axis=1, keepdims=True))
    scale[scale == 0] = 1.0
    return float((np.abs(dev.reshape(r.shape) - r) / scale).max())


# ---- signals ---------------------------------------------------------------------------------------------------------------------------------
def bursts(H, groups=(4, 3, 4, 3), seed=0, lead=6, trail=7, noise=1e-4, sr=8000.0):
    """Harmonic bursts under raised-cosine envelopes, in groups separated by silences -> (x float32, bursts, interior gaps).  A burst lasts 9-13
    frames, a gap 12-19, the bursts of a group touch; a noise floor lies under everything."""
    rng = np.random.default_rng(seed)
    parts, nb = [np.zeros(lead * H)], 0
    for gi, g in enumerate(groups):
        if gi:
            parts.append(np.zeros(int(rng.integers(12, 20)) * H))
        for _ in range(g):
            n = int(rng.integers(9, 14)) * H
            f0 = float(rng.uniform(90.0, 220.0))
            t = np.arange(n) / sr
            tone = sum(np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 6))
            env = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(n) + 0.5) / n)
            parts.append(float(rng.uniform(0.15, 0.3)) * env * tone)
            nb += 1
    parts.append(np.zeros(trail * H))
    y = np.concatenate(parts)
    y = y + noise * rng.standard_normal(len(y))
    return y.astype(np.float32), nb, len(groups) - 1


def periodic(H, levels, seed=0):
    """A signal of period H scaled by a power of two per frame span: ``levels`` = [(frames, scale)].  Frames whose window lies inside one span hold
    identical samples, so their power is bit-equal on any arithmetic."""
    g = np.random.default_rng(seed).uniform(-0.5, 0.5, H).astype(np.float32)
    return np.concatenate([np.tile(g, n) * np.float32(s) for n, s in levels]).astype(np.float32)


def padded(rows, L=None, fill=np.nan):
    """(x (B, L) float32 with ``fill`` behind every row's length, lens)."""
    lens = [len(r) for r in rows]
    L = max(lens) if L is None else L
    x = np.full((len(rows), L), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, lens


# ---- the named cases of the host and GPU tests: name -> (x (B, L) float32, lens or None, W, par); H = 64 throughout ----------------------------
H0 = 64
CASES = ("b1-w128", "b3-w192", "b5-w256", "lengths", "last-only", "one-frame-dip", "pause-edges", "sound-edges", "blip", "silent-and-sounding",
         "rank-0", "rank-half", "plateau", "dc")


def one_frame_dip_row():
    """A single burst cut two frames behind its peak: the only candidate is frame nf - 2 and its dip interval holds exactly one frame.  (An EMPTY
    interval cannot occur: the frame behind a candidate is never one, by the peak rule.)"""
    x, _, _ = bursts(H0, groups=(1,), seed=5)
    full = speech_rate(x[None], None, np.kaiser(128, 20.24), H0)
    c = int(np.flatnonzero(full["mark"][0] & CAND)[-1])
    return x[: (c + 2) * H0]


def case(name):
    par = dict(PAR)
    if name in ("b1-w128", "b3-w192", "b5-w256"):
        B, W = {"b1-w128": (1, 128), "b3-w192": (3, 192), "b5-w256": (5, 256)}[name]
        rows = [bursts(H0, seed=s)[0] for s in range(B)]
        rows = [r[: len(r) - 17 * b] for b, r in enumerate(rows)]        # (odd lengths: the last frame is a partial one)
        return (*padded(rows), W, par)
    if name == "lengths":
        W, L = 256, 20 * H0 + 5
        y = bursts(H0, groups=(2,), seed=9, lead=1, trail=1)[0][:L + 1]
        lens = [0, 1, 63, 64, 65, W // 2, W, 3 * H0, L, L + 1]
        x = np.full((len(lens), L), np.nan, dtype=np.float32)
        for b, n in enumerate(lens):
            x[b, :min(n, L)] = y[:min(n, L)]
        return x, lens, W, par
    if name == "last-only":
        return (*padded([bursts(H0, groups=(1,), seed=5)[0]]), 128, par)
    if name == "one-frame-dip":
        return (*padded([one_frame_dip_row()]), 128, par)
    if name == "pause-edges":                                            # raw silent runs of 7 = min_pause - 1 (filled) and 8 = min_pause (a pause)
        return (*padded([periodic(H0, [(10, 1), (9, 0), (10, 1)]), periodic(H0, [(10, 1), (10, 0), (10, 1)])]), 128, par)
    if name == "sound-edges":                                            # raw sounding runs of 3 = min_sound - 1 (dropped) and 4 = min_sound (kept)
        par["min_sound"] = 4
        return (*padded([periodic(H0, [(12, 0), (1, 1), (12, 0)]), periodic(H0, [(12, 0), (2, 1), (12, 0)])]), 128, par)
    if name == "blip":                                                   # a sounding run under min_sound between two silent runs under min_pause
        par["min_sound"] = 5
        return (*padded([periodic(H0, [(10, 1), (5, 0), (2, 1), (5, 0), (10, 1)])]), 128, par)
    if name == "silent-and-sounding":
        return (*padded([np.zeros(30 * H0, np.float32), periodic(H0, [(30, 1.0)])]), 128, par)
    if name in ("rank-0", "rank-half"):
        par["rank_fraction"] = 0.0 if name == "rank-0" else 0.5
        return (*padded([bursts(H0, seed=s)[0] for s in (4, 5)]), 192, par)
    if name == "plateau":                                                # exact ties: frames of identical samples
        return (*padded([periodic(H0, [(8, 0.25), (8, 1.0), (8, 0.25)])]), 128, par)
    if name == "dc":
        return (*padded([bursts(H0, seed=0)[0] + np.float32(0.25)]), 128, par)
    raise KeyError(name)


def case_ref(name, mutant=None, plain=False):
    x, lens, W, par = case(name)
    return speech_rate(x, lens, np.kaiser(W, 20.24), H0, par, mutant=mutant, plain=plain)


MUTANT_CASE = {"dip_before": "b1-w128", "peak_ge_left": "plateau", "no_fill": "b1-w128", "b_before_a": "blip", "rank_plus": "b1-w128",
               "no_mean": "dc", "last_never": "last-only"}


def mutant_distance(res, wrong):
    """(the largest relative distance of a float output, whether mark or count differ)."""
    far = max(rel_err(res[k], wrong[k]) for k in FLOAT_OUTPUTS)
    return far, not (np.array_equal(res["mark"], wrong["mark"]) and np.array_equal(res["count"], wrong["count"]))
