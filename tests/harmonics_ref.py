"""numpy restatement of ev_harmonics (include/emojivoice.h): per frame the levels of the harmonics of the frame's period in the float64 log-power
spectrum of ev_voice_quality, and from them H1-H2, H1-A3 and the level of the harmonic at F1, F2, F3 over H1 (Hanson 1997; eGeMAPS, Eyben et al.
2016), in float64 and, from the same float64 tables, in np.longdouble.  The device runs one fixed order of its own in the DFT sums, so it differs
from the float64 restatement by float64 rounding; the longdouble evaluation measures how much rounding the INPUT admits, and the margins reported
beside the figures say how far every decision (an argmax, a floor, a ceil, a threshold) lies from turning over.

    frames(n)  = ceil(n / H)
    s_f[j]     = x[f H + H / 2 - W / 2 + j], ZERO outside [0, len)                                    (no reflection)
    re, sm     = s_f @ {c, s}                                                                           (ev_stft_dist's basis)
    raw        = sm^2 + re^2,  p = max(raw, floor),  Ldb = (10 / ln 10) log(p)
    T          = (double)period[f];  UNVOICED: not T > 0;  SILENT: no raw > floor;  UNRESOLVED: v = nfft / T < min_spacing
    c, r       = h v, max(1, search v);  lo, hi = ceil(c - r), floor(c + r);  measured while hi <= NB - 2 and h <= n_harm
    k*         = argmax Ldb over lo .. hi (the lowest k of a tie);  a, b, c' = Ldb[k* - 1], Ldb[k*], Ldb[k* + 1];  den = (a - 2 b) + c'
    shift      = 0.5 (a - c') / den when den < 0 and |shift| <= 1, else 0;  A_h = b - 0.25 (a - c') shift;  f_h = (k* + shift)(sr / nfft)
    u          = sr / T;  g = F_i / u;  h_i = floor(g + 0.5), valid when 1 <= h_i <= n_h;  rel_i = A_{h_i} - A_1
    A3         = max A_h over max(1, ceil(g - w)) .. min(n_h, floor(g + w)),  g = F_3 / u,  w = max(0.5, a3_range g)   (the lowest h of a tie)
    frame      = {A_1 - A_2, A_1 - A3, rel_1, rel_2, rel_3, A_1, f_1, v};  count = {n_h, flags}
"""
from collections import namedtuple

import numpy as np

from stft_dist_ref import basis, hann, twiddle  # noqa: F401  (the windowed DFT basis is ev_stft_dist's, entry for entry)
from stoi_ref import GARBAGE, speech_like  # noqa: F401
from voice_quality_ref import err, frame_matrix, frames, ragged_lens  # noqa: F401  (the framing is ev_voice_quality's)

TOL = 1e-9                       # device against the float64 restatement, every entry: |got - ref| <= TOL max(|ref|, 1)
INPUT_TOL = 1e-11                # float64 against longdouble restatement, the same form: the condition on the input
MIN_PEAK_MARGIN = 1e-6           # dB between the two largest Ldb of a searched range, every measured harmonic
MIN_ROUND_MARGIN = 1e-9          # every argument of a floor / ceil / threshold from its boundary
POWER_FLOOR = 1e-7
FS = 22050
# the restatement against the closed form on harmonic complexes (tests/test_harmonics_host.py measures and says how): twice the measured figure,
# never looser than 1 dB
CLOSED_GATE_H1H2 = 0.39          # dB: twice the measured 0.191
CLOSED_GATE_REL = 1.0            # dB: twice the measured 0.545 is 1.09
FIGURES = ("h1_h2_db", "h1_a3_db", "f1_rel_db", "f2_rel_db", "f3_rel_db", "h1_db", "h1_hz", "spacing_bins")
MUTANTS = ("half_spacing", "no_parabola", "tie_high", "a3_nearest", "floor_g", "power_vertex")

Geometry = namedtuple("Geometry", "nfft H W sr n_harm search min_spacing a3_range", defaults=(0.25, 4.0, 0.1))

# n_harm = 64 at 1024: lanes with four harmonics (h = j + 49); 32 at 2048 / 256: what fits 160 KiB of LDS beside the log-spectrum
GEOMETRIES = (
    Geometry(64, 10, 24, 2000, 8),
    Geometry(64, 64, 64, 2000, 8),
    Geometry(512, 128, 400, FS, 48),
    Geometry(1024, 256, 1024, FS, 64),
    Geometry(2048, 256, 2048, FS, 32),
)
EDGE_GEOMETRIES = (Geometry(16, 3, 12, 2000, 4), Geometry(16, 7, 16, 2000, 4))     # voice_quality_ref's: NB = 9, at most one harmonic
IDS = [f"{g.nfft}-{g.H}-{g.W}" for g in GEOMETRIES + EDGE_GEOMETRIES]

_TABLES = {}


def tables(g):
    """The host tables of a load, made once per (nfft, W) and never modified: window, twiddle and the basis (c, s)."""
    key = (g.nfft, g.W)
    if key not in _TABLES:
        t = {"window": hann(g.W), "twiddle": twiddle(g.nfft)}
        t["c"], t["s"] = basis(g.nfft, g.W, t["window"], t["twiddle"])
        for v in t.values():
            v.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


def spectrum(x, g, dtype=np.float64):
    """(nf, NB) raw powers sm^2 + re^2 of one row."""
    t = tables(g)
    fm = frame_matrix(np.asarray(x, dtype=np.float64), g).astype(dtype)
    re, sm = fm @ t["c"].astype(dtype), fm @ t["s"].astype(dtype)
    return sm * sm + re * re


def _near(a):
    """distance of every entry to the nearest integer, float64"""
    a = np.asarray(a)
    return np.abs(a - np.rint(a)).astype(np.float64)


def _vertex(a, b, c, dtype):
    den = (a - dtype(2) * b) + c
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den < 0, dtype(0.5) * (a - c) / np.where(den < 0, den, dtype(1)), dtype(0))
    s = np.where(np.abs(s) <= 1, s, dtype(0))
    return b - dtype(0.25) * (a - c) * s, s


def row(x, period, g, formant=None, fcount=None, dtype=np.float64, floor=POWER_FLOOR, mutant=None):
    """One row of len(x) samples, ``period`` (>= nf,) float32, ``formant`` (>= nf, n_formants, 2) float64 and ``fcount`` (>= nf,) int32 or both
    None -> dict: frame (nf, 8), count (nf, 2) int32, harm (nf, n_harm, 2), kstar (nf, n_harm) int64 (-1: not measured), shift (nf, n_harm), hidx (nf, 3) int64
    (h_i, 0: not valid), a3 (nf, 2) int64 (the range, 0 0: not valid), margin (nf, n_harm): the gap in dB between the two largest Ldb of
    the searched range (inf: not measured), rounding (nf,): the least distance of an argument of a floor, ceil or threshold of the frame from
    its boundary (inf: none)."""
    assert mutant is None or mutant in MUTANTS
    raw = spectrum(x, g, dtype)
    nf, NB = raw.shape
    NH = g.n_harm
    p = np.maximum(raw, dtype(floor))
    db = dtype(10) / np.log(dtype(10))
    L = db * np.log(p)
    T = np.asarray(period[:nf], dtype=np.float32).astype(np.float64).astype(dtype)
    voiced = T > 0
    live = (raw > dtype(floor)).any(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(voiced & live, dtype(g.nfft) / np.where(voiced, T, dtype(1)), dtype(0))
    comb = voiced & live & ~(v < dtype(g.min_spacing))
    rounding = np.where(voiced & live, np.abs(v - dtype(g.min_spacing)).astype(np.float64), np.inf)
    r = np.maximum(dtype(1), dtype(0.5 if mutant == "half_spacing" else g.search) * v)
    c = np.arange(1, NH + 1).astype(dtype)[None, :] * v[:, None]
    lo_a, hi_a = c - r[:, None], c + r[:, None]
    with np.errstate(invalid="ignore"):
        lo, hi = np.ceil(lo_a), np.floor(hi_a)
        meas = comb[:, None] & (hi <= NB - 2)
    edge = np.minimum(_near(lo_a), _near(hi_a))
    rounding = np.minimum(rounding, np.where(comb[:, None], np.where(np.isfinite(edge), edge, np.inf), np.inf).min(axis=1, initial=np.inf))
    loi = np.where(meas, lo, 1).astype(np.int64)
    hii = np.where(meas, hi, 1).astype(np.int64)
    assert (loi >= 1).all() and (loi <= hii).all()
    maxw = int((hii - loi).max(initial=0)) + 1
    k = loi[:, :, None] + np.arange(maxw)[None, None, :]
    inside = k <= hii[:, :, None]
    fi = np.arange(nf)[:, None, None]
    Lg = np.where(inside, L[fi, np.minimum(k, NB - 1)], -np.inf)
    if mutant == "tie_high":
        kidx = maxw - 1 - np.argmax(Lg[:, :, ::-1], axis=2)
    else:
        kidx = np.argmax(Lg, axis=2)
    ks = loi + kidx
    top = np.sort(Lg, axis=2)
    with np.errstate(invalid="ignore"):
        margin = np.where(meas, (top[:, :, -1] - top[:, :, -2]).astype(np.float64), np.inf) if maxw > 1 else np.full((nf, NH), np.inf)
    f2 = np.arange(nf)[:, None]
    src = p if mutant == "power_vertex" else L
    a, b, cc = src[f2, ks - 1], src[f2, ks], src[f2, np.minimum(ks + 1, NB - 1)]
    A, s = _vertex(a, b, cc, dtype)
    if mutant == "power_vertex":
        A = db * np.log(np.maximum(A, dtype(floor)))
    if mutant == "no_parabola":
        A, s = L[f2, ks], np.zeros_like(s)
    fh = (ks.astype(dtype) + s) * dtype(float(g.sr) / float(g.nfft))
    A, fh = np.where(meas, A, dtype(0)), np.where(meas, fh, dtype(0))
    nh = meas.sum(axis=1)
    frame = np.zeros((nf, 8), dtype)
    flags = np.zeros(nf, np.int64)
    frame[:, 7] = v
    one, two = nh >= 1, nh >= 2
    frame[:, 5], frame[:, 6] = np.where(one, A[:, 0], 0), np.where(one, fh[:, 0], 0)
    if NH >= 2:
        frame[:, 0] = np.where(two, A[:, 0] - A[:, 1], 0)
    flags |= two.astype(np.int64)
    hidx, a3 = np.zeros((nf, 3), np.int64), np.zeros((nf, 2), np.int64)
    if formant is not None:
        formant, fcount = np.asarray(formant, dtype=np.float64), np.asarray(fcount)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = dtype(float(g.sr)) / np.where(voiced, T, dtype(1))
        for i in range(min(3, formant.shape[1])):
            F = formant[:nf, i, 0].astype(dtype)
            okF = comb & (fcount[:nf] >= i + 1) & (F > 0)
            gq = np.where(okF, F, dtype(1)) / u
            arg = gq if mutant == "floor_g" else gq + dtype(0.5)
            hd = np.floor(arg)
            rounding = np.minimum(rounding, np.where(okF, _near(arg), np.inf))
            ok = okF & (hd >= 1) & (hd <= nh)
            hi_ = np.where(ok, hd, 1).astype(np.int64)
            frame[:, 2 + i] = np.where(ok, A[np.arange(nf), hi_ - 1] - A[:, 0], 0)
            flags |= ok.astype(np.int64) << (i + 1)
            hidx[:, i] = np.where(ok, hi_, 0)
            if i == 2:
                if mutant == "a3_nearest":
                    ok3, l3, h3 = ok, hi_, hi_
                else:
                    w = np.maximum(dtype(0.5), dtype(g.a3_range) * gq)
                    rounding = np.minimum(rounding, np.where(okF, np.minimum(_near(gq - w), _near(gq + w)), np.inf))
                    l3f, h3f = np.maximum(dtype(1), np.ceil(gq - w)), np.minimum(nh.astype(dtype), np.floor(gq + w))
                    ok3 = okF & (l3f <= h3f)
                    l3, h3 = np.where(ok3, l3f, 1).astype(np.int64), np.where(ok3, h3f, 1).astype(np.int64)
                hh = np.arange(1, NH + 1)[None, :]
                Am = np.where((hh >= l3[:, None]) & (hh <= h3[:, None]), A, -np.inf)
                best = np.argmax(Am, axis=1)
                frame[:, 1] = np.where(ok3, A[:, 0] - A[np.arange(nf), best], 0)
                flags |= ok3.astype(np.int64) << 4
                a3[:, 0], a3[:, 1] = np.where(ok3, l3, 0), np.where(ok3, h3, 0)
    harm = np.stack([fh, A], axis=2)
    count = np.stack([nh, flags], axis=1).astype(np.int32)
    return {"frame": frame, "count": count, "harm": harm, "kstar": np.where(meas, ks, -1), "shift": np.where(meas, s, dtype(0)), "hidx": hidx, "a3": a3, "margin": margin,
            "rounding": rounding}


def batch(x, lens, period, g, formant=None, fcount=None, dtype=np.float64, floor=POWER_FLOOR, mutant=None):
    """ev_harmonics's shapes: x (B, L), lens (B,) or None, period (B, NF), formant (B, NF, n, 2) and fcount (B, NF) or None -> the dict of
    ``row`` with a leading batch axis; a row with len < 1 or len > L is a row of zeros; nothing at or behind a row's length is looked at."""
    x = np.atleast_2d(np.asarray(x))
    B, L = x.shape
    lens = [L] * B if lens is None else [int(v) for v in lens]
    NF, NH = frames(L, g.H), g.n_harm
    out = {"frame": np.zeros((B, NF, 8), dtype), "count": np.zeros((B, NF, 2), np.int32), "harm": np.zeros((B, NF, NH, 2), dtype),
           "kstar": np.full((B, NF, NH), -1, np.int64), "shift": np.zeros((B, NF, NH), dtype), "hidx": np.zeros((B, NF, 3), np.int64), "a3": np.zeros((B, NF, 2), np.int64),
           "margin": np.full((B, NF, NH), np.inf), "rounding": np.full((B, NF), np.inf)}
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        r = row(x[b, :n], period[b], g, None if formant is None else formant[b], None if fcount is None else fcount[b], dtype, floor, mutant)
        nf = r["frame"].shape[0]
        for k2, v in r.items():
            out[k2][b, :nf] = v
    return out


# ---- the rows of the tests ---------------------------------------------------------------------------------------------------------------------

def tone_row(n, T, sr, seed=0, amp=0.1, noise=1e-3, top=0.45, tilt_db=0.0, silence=None):
    """A harmonic complex of period ``T`` samples (f0 = sr / T), float32: partials h f0 below ``top`` sr at amplitude amp 10^(-tilt_db (h - 1) /
    20) / h, on white noise of ``noise`` rms (above the power floor in every geometry of the tests); ``silence`` = (first, end): exact zeros
    there."""
    g = np.random.default_rng(4000 + seed)
    t = np.arange(n, dtype=np.float64)
    s = np.zeros(n)
    h = 1
    while h / T < top:
        s += 10.0 ** (-tilt_db * (h - 1) / 20.0) / h * np.sin(2 * np.pi * h * t / T + 0.37 * h * h)
        h += 1
    y = amp * s + noise * g.standard_normal(n)
    if silence is not None:
        y[silence[0]:silence[1]] = 0.0
    return y.astype(np.float32)


def tie_row(g, n=5000):
    """(x float32, T float32): a band-limited tone (eight partials, 6.83 bins apart) WITHOUT noise: above its partials every bin lies on the power
    floor, so every searched range there is a tie of equal values, exact in any arithmetic."""
    t = np.arange(n, dtype=np.float64)
    T = g.nfft / 6.83
    return (0.1 * sum(np.sin(2 * np.pi * h * t / T + 0.37 * h * h) / h for h in range(1, 9))).astype(np.float32), np.float32(T)


def speech_periods(n, H, seed=0, fs=FS, f0=120.0):
    """The period in samples of ``speech_like(n, seed)`` at the centre of every frame of hop H, float32 (the glide of its f0 restated)."""
    t = (np.arange(frames(n, H)) * H + H // 2) / float(fs)
    return (fs / (f0 * (1.0 + 0.2 * np.sin(2 * np.pi * 0.7 * t + 0.3 * seed)))).astype(np.float32)


def case(g, seed=0, n_formants=4):
    """The three ragged rows of a geometry (15, 0 and 1 frames mod 16) with periods and formants of the test's own:
    x (3, L) float32 with GARBAGE behind every row's length, lens, period (3, NF) float32, formant (3, NF, n_formants, 2) float64, fcount
    (3, NF) int32.  At 22050 Hz rows 0 and 1 are speech_like rows at their gliding period, row 2 a tone; at 2000 Hz all are tones.  Every row
    holds frames of exact zeros (silent), frames with period 0 (unvoiced), frames with a period too long to resolve and voiced frames; the
    periods are no dyadic fractions of nfft, so no search range ends on an integer."""
    rng = np.random.default_rng(7000 + seed + 13 * g.nfft + g.H)
    lens = ragged_lens(g.H)
    NB = g.nfft // 2 + 1
    # periods (samples) whose spacing nfft / T is resolved: one cut by n_harm where the geometry admits it, one cut by the Nyquist bin
    v_choices = [4.37, 5.81, 10.17] if NB > 9 else [4.37, 5.3]
    rows, periods = [], []
    for i, n in enumerate(lens):
        nf = frames(n, g.H)
        z0 = (nf // 2) * g.H
        # the borders of the silence sit so that a frame's window holds no or at least two samples with a non-zero weight beside it: ONE sample
        # has a flat spectrum, every bin of a range a tie in exact arithmetic
        s0 = g.H // 2 - g.W // 2
        e0, e1 = z0 - g.W, z0 + g.W + 2 * g.H
        e0 += (3 - (e0 - s0)) % g.H
        e1 += (g.W - 3 - (e1 - s0)) % g.H
        silence = (e0, e1)
        if g.sr == FS and i < 2:
            y = speech_like(n, seed=seed + i, fs=FS).copy()
            y[silence[0]:silence[1]] = 0.0
            per = speech_periods(n, g.H, seed + i)
        else:
            T = g.nfft / v_choices[(i + seed) % len(v_choices)]
            y = tone_row(n, T, g.sr, seed=seed + i, silence=silence)
            per = np.full(nf, T, np.float32)
        per = per.copy()
        per[1::7] = 0.0                                                  # unvoiced
        per[3::11] = np.float32(g.nfft / 3.3)                            # unresolved: 3.3 bins between harmonics
        per[5::13] = np.float32(g.nfft / v_choices[(i + 1) % len(v_choices)])   # a comb of another spacing than the row's
        if nf > 6:
            per[6] = np.float32(g.nfft / 4.0003)                         # just resolved
        rows.append(y)
        periods.append(per)
    L = max(lens) + 29
    NF = frames(L, g.H)
    x = np.full((3, L), GARBAGE, np.float32)
    period = np.full((3, NF), 77.7, np.float32)                          # (garbage behind a row's frames: never read)
    for b, (y, per) in enumerate(zip(rows, periods)):
        x[b, :len(y)] = y
        period[b, :len(per)] = per
    ny = g.sr / 2.0
    formant = np.zeros((3, NF, n_formants, 2))
    lo_hi = ((0.03, 0.09), (0.1, 0.2), (0.22, 0.31), (0.33, 0.4))
    for i in range(n_formants):
        a, b2 = lo_hi[min(i, 3)]
        formant[:, :, i, 0] = ny * rng.uniform(a, b2, (3, NF))
        formant[:, :, i, 1] = rng.uniform(40.0, 900.0, (3, NF))
    fcount = rng.choice(np.array([-1, 0, 1, 2, 3, 4, 4, 4, 3, 3], np.int32), (3, NF)).astype(np.int32)
    fcount = np.minimum(fcount, n_formants).astype(np.int32)
    return x, lens, period, formant, fcount


def conditions(x, lens, period, g, formant, fcount, floor=POWER_FLOOR):
    """The conditions on the input, on the restatement alone: (float64 result, report).  report: input_err (float64 against longdouble over
    frame and harm), decisions_equal (k*, h_i, the A3 ranges, the counts), min_margin (dB), min_rounding, and the census of the frames."""
    r64 = batch(x, lens, period, g, formant, fcount, np.float64, floor)
    rld = batch(x, lens, period, g, formant, fcount, np.longdouble, floor)
    T = np.asarray(period, dtype=np.float64)
    nfr = np.array([frames(n, g.H) for n in lens])
    inside = np.arange(r64["count"].shape[1])[None, :] < nfr[:, None]
    nh = r64["count"][..., 0]
    v = r64["frame"][..., 7]
    lanes = np.zeros(5, np.int64)                                         # how many (frame, lane) pairs search 0, 1, 2, 3, 4 harmonics
    for cnt in nh[inside & (nh > 0)]:
        per_lane = np.array([len(range(j + 1, cnt + 1, 16)) for j in range(16)])
        lanes += np.bincount(per_lane, minlength=5)[:5]
    rep = {
        "input_err": max(err(r64["frame"], rld["frame"]), err(r64["harm"], rld["harm"])),
        "decisions_equal": all(np.array_equal(r64[k], rld[k]) for k in ("kstar", "hidx", "a3", "count")),
        "min_margin": float(r64["margin"].min()),
        "min_rounding": float(r64["rounding"].min()),
        "voiced": int((inside & (nh > 0)).sum()),
        "unvoiced": int((inside & ~(T[:, :inside.shape[1]] > 0)).sum()),
        "unresolved": int((inside & (nh == 0) & (v > 0) & (v < g.min_spacing)).sum()),
        "silent": int((inside & (T[:, :inside.shape[1]] > 0) & (v == 0)).sum()),
        "cut_by_n_harm": int((inside & (nh == g.n_harm)).sum()),
        "cut_by_nyquist": int((inside & (nh > 0) & (nh < g.n_harm)).sum()),
        "lanes": lanes.tolist(),
        "searched": int(np.isfinite(r64["margin"]).sum()),
    }
    return r64, rep
