"""numpy restatement of ev_voice_quality (include/emojivoice.h): per frame the spectral-balance descriptors of the eGeMAPS set (alpha ratio,
Hammarberg index, two spectral slopes; Eyben et al. 2016) and the cepstral peak prominence (Hillenbrand et al. 1994), as two matrix products
(frames x windowed DFT basis, dB spectrum x cosine basis), in float64 and, from the same float64 tables, in np.longdouble.  The device runs one
fixed order of its own, so it differs from the float64 restatement by float64 rounding; the longdouble evaluation measures how much rounding
the INPUT admits.

    frames(n)  = ceil(n / H)
    s_f[j]     = x[f H + H / 2 - W / 2 + j], ZERO outside [0, len)                                    (no reflection)
    re, sm     = s_f @ {c, s},  c[j][k] = w[j] cos_tab[((j + off) k) mod nfft], off = (nfft - W) / 2   (ev_stft_dist's basis)
    raw        = sm^2 + re^2,  p = max(raw, floor),  Ldb = (10 / ln 10) log(p)
    C[q]       = sum_k Ldb[k] cep[k][q],  cep[k][q] = g[k] cos_tab[(k q) mod nfft] / nfft,  g = 1 at k = 0 and k = nfft / 2, else 2
    q*         = argmax C over q_min .. q_max (the lowest q of a tie)
    base       = mean_{q_fit .. q_max} C + (sum_q fit_w[q - q_fit] C[q]) (q* - q_mean)
    frame      = {C[q*] - base, (10 / ln 10)(log sum_{alpha hi} p - log sum_{alpha lo} p), max_{ham lo} Ldb - max_{ham hi} Ldb,
                  slope_w[0] . Ldb, slope_w[1] . Ldb, sum p, C[q*], base}
    fit_w[i]   = (q_i - q_mean) / sum (q - q_mean)^2 over q_fit .. q_max;  slope_w[b][k] = (x_k - xbar) / sum (x - xbar)^2 over band b,
                 x_k = k sr / nfft / 1000 (dB per kHz), 0 outside the band: least-squares lines in their centred form
    A silent frame (no raw[k] > floor) keeps its power; its other seven entries, its peak and its cepstrum are zeros.

The cepstrum is the linear real cepstrum of the dB spectrum: comparable across this project's runs, not to the digit with Praat's or
Hillenbrand's CPP (cepstral magnitude in dB) or VoiceSauce's (pitch-synchronous windows).
"""
from collections import namedtuple

import numpy as np

from stft_dist_ref import basis, edge_signal, hann, twiddle  # noqa: F401  (the windowed DFT basis is ev_stft_dist's, entry for entry)
from stoi_ref import GARBAGE, padded, speech_like  # noqa: F401

TOL = 1e-9                       # device against the float64 restatement, every entry: |got - ref| <= TOL max(|ref|, 1)
INPUT_TOL = 1e-11                # float64 against longdouble restatement, the same form: the condition on the input
MIN_PEAK_MARGIN = 1e-6           # the gap between the two largest C of the search range, every non-silent frame
POWER_FLOOR = 1e-7
FS = 22050
FIGURES = ("cpp_db", "alpha_ratio_db", "hammarberg_db", "slope_0_500", "slope_500_1500", "power", "peak_value", "baseline")

Geometry = namedtuple("Geometry", "nfft H W q_fit q_min q_max bands sr")


def band_edges(sr, nfft):
    """The six bin ranges of audio.voice_quality_tables: ceil(hz nfft / sr) at alpha 50-1000 / 1000-5000 Hz, Hammarberg 0-2000 / 2000-5000 Hz,
    slopes 0-500 / 500-1500 Hz."""
    e = lambda hz: int(-(-(hz * nfft) // sr))
    return ((e(50), e(1000)), (e(1000), e(5000)), (e(0), e(2000)), (e(2000), e(5000)), (e(0), e(500)), (e(500), e(1500)))


SMALL_BANDS = ((1, 5), (5, 16), (0, 8), (8, 20), (0, 4), (4, 11))
GEOMETRIES = (
    Geometry(64, 10, 24, 2, 4, 30, SMALL_BANDS, 2000),
    Geometry(64, 64, 64, 2, 4, 32, SMALL_BANDS, 2000),
    Geometry(512, 128, 400, 22, 36, 250, band_edges(FS, 512), FS),
    Geometry(1024, 256, 1024, 22, 36, 340, band_edges(FS, 1024), FS),
)
IDS = [f"{g.nfft}-{g.H}-{g.W}" for g in GEOMETRIES]
# a hop under 4 (the skew walk pads inside a step), a skew of 3 at a hop that is not 2 mod 4, W / 4 = 3 (the first round's clamp) and W / 4 = 4 (one whole round);
# NB = 9: one bin tile (waves 1-3 hand over their identities), NBp = 12: three phase-2 steps, NQ = 8: half a quefrency tile
EDGE_BANDS = ((1, 3), (3, 7), (0, 4), (4, 9), (0, 3), (3, 6))
EDGE_GEOMETRIES = (Geometry(16, 3, 12, 1, 2, 8, EDGE_BANDS, 2000), Geometry(16, 7, 16, 1, 2, 8, EDGE_BANDS, 2000))
MUTANTS = ("ends2", "fit_from_qmin", "peak_over_fit", "natural_log", "reflect")


def frames(n, H):
    return -(-int(n) // int(H))


def fit_weights(q_lo, q_hi):
    """(fit_w (q_hi - q_lo + 1,), q_mean): the centred least-squares slope weights over the quefrencies q_lo .. q_hi."""
    q = np.arange(q_lo, q_hi + 1, dtype=np.float64)
    d = q - q.mean()
    return d / np.sum(d * d), float(q.mean())


def slope_weights(bands, nfft, sr):
    """(2, NB): row b the centred least-squares slope weights over slope band b in dB per kHz, zeros outside it."""
    NB = nfft // 2 + 1
    w = np.zeros((2, NB))
    for b, (lo, hi) in enumerate(bands[4:6]):
        x = np.arange(lo, hi, dtype=np.float64) * sr / nfft / 1000.0
        d = x - x.mean()
        w[b, lo:hi] = d / np.sum(d * d)
    return w


def cep_basis(g, ends=1.0):
    """(NB, NQ) float64: g[k] cos_tab[(k q) mod nfft] / nfft, each entry one rounding, the phase index in exact integers."""
    NB = g.nfft // 2 + 1
    k, q = np.arange(NB)[:, None], np.arange(g.q_fit, g.q_max + 1)[None, :]
    gk = np.full((NB, 1), 2.0)
    gk[0, 0] = gk[NB - 1, 0] = ends
    return gk * twiddle(g.nfft)[(k * q) % g.nfft, 0] / float(g.nfft)


_TABLES = {}


def tables(g):
    """The host tables of a load, made once per geometry and never modified: window, twiddle, bands (12,) int32, slope_w, fit_w, q_mean."""
    if g not in _TABLES:
        fit_w, q_mean = fit_weights(g.q_fit, g.q_max)
        t = {"window": hann(g.W), "twiddle": twiddle(g.nfft), "bands": np.asarray(g.bands, dtype=np.int32).reshape(-1),
             "slope_w": slope_weights(g.bands, g.nfft, g.sr), "fit_w": fit_w, "q_mean": q_mean}
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _TABLES[g] = t
    return _TABLES[g]


def frame_matrix(x, g, reflect=False):
    """(nf, W): frame f holds x[f H + H / 2 - W / 2 + j], zeros outside the row (``reflect``: the mutant that mirrors at both ends as
    ev_stft_dist does)."""
    x = np.asarray(x)
    n = len(x)
    nf = frames(n, g.H)
    i = np.arange(nf)[:, None] * g.H + g.H // 2 - g.W // 2 + np.arange(g.W)[None, :]
    if reflect:
        i = np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    ok = (i >= 0) & (i < n)
    return np.where(ok, x[np.clip(i, 0, n - 1)], 0).reshape(nf, g.W)


def spectrum(x, g, dtype=np.float64, reflect=False):
    """(nf, NB) raw powers sm^2 + re^2 of one row."""
    t = tables(g)
    c, s = basis(g.nfft, g.W, t["window"], t["twiddle"])
    fm = frame_matrix(np.asarray(x, dtype=np.float64), g, reflect).astype(dtype)
    re, sm = fm @ c.astype(dtype), fm @ s.astype(dtype)
    return sm * sm + re * re


def row(x, g, dtype=np.float64, floor=POWER_FLOOR, mutant=None, guard=True):
    """One row -> (frame (nf, 8), peak (nf,) int32, cepstrum (nf, NQ), margin (nf,): the gap between the two largest C of the search range,
    inf on a silent frame).  ``guard=False`` leaves the silent-frame rule out (what the rule exists for)."""
    assert mutant is None or mutant in MUTANTS
    t = tables(g)
    raw = spectrum(x, g, dtype, reflect=mutant == "reflect")
    nf = raw.shape[0]
    p = np.maximum(raw, dtype(floor))
    db = dtype(1) if mutant == "natural_log" else dtype(10) / np.log(dtype(10))
    L = db * np.log(p)
    C = L @ cep_basis(g, 2.0 if mutant == "ends2" else 1.0).astype(dtype)
    lo = 0 if mutant == "peak_over_fit" else g.q_min - g.q_fit
    idx = np.argmax(C[:, lo:], axis=1) + lo
    qs = g.q_fit + idx
    cq = C[np.arange(nf), idx]
    if mutant == "fit_from_qmin":
        fw, qm = fit_weights(g.q_min, g.q_max)
        m = g.q_min - g.q_fit
        base = C[:, m:].mean(axis=1) + (C[:, m:] @ fw.astype(dtype)) * (qs - dtype(qm))
    else:
        base = C.mean(axis=1) + (C @ t["fit_w"].astype(dtype)) * (qs - dtype(t["q_mean"]))
    b = g.bands
    alpha = db * (np.log(p[:, b[1][0]:b[1][1]].sum(axis=1)) - np.log(p[:, b[0][0]:b[0][1]].sum(axis=1)))
    ham = L[:, b[2][0]:b[2][1]].max(axis=1) - L[:, b[3][0]:b[3][1]].max(axis=1)
    sl = L @ t["slope_w"].T.astype(dtype)
    fr = np.stack([cq - base, alpha, ham, sl[:, 0], sl[:, 1], p.sum(axis=1), cq, base], axis=1).reshape(nf, 8)
    top = np.sort(C[:, lo:], axis=1)
    margin = (top[:, -1] - top[:, -2]).astype(np.float64)
    peak = qs.astype(np.int32)
    if guard:
        silent = ~(raw > dtype(floor)).any(axis=1)
        keep = fr[:, 5].copy()
        fr[silent] = 0
        fr[:, 5] = keep
        peak[silent] = 0
        C = np.where(silent[:, None], dtype(0), C)
        margin[silent] = np.inf
    return fr, peak, C, margin


def batch(x, lens, g, dtype=np.float64, floor=POWER_FLOOR, mutant=None):
    """ev_voice_quality's shapes: x (B, L), lens (B,) or None -> frame (B, NF, 8), peak (B, NF) int32, cepstrum (B, NF, NQ), margin (B, NF); a
    row with len < 1 or len > L is a row of zeros; nothing at or behind a row's length is looked at."""
    x = np.atleast_2d(np.asarray(x))
    B, L = x.shape
    lens = [L] * B if lens is None else [int(v) for v in lens]
    NF, NQ = frames(L, g.H), g.q_max - g.q_fit + 1
    fr, pk, cp, mg = np.zeros((B, NF, 8), dtype), np.zeros((B, NF), np.int32), np.zeros((B, NF, NQ), dtype), np.full((B, NF), np.inf)
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        f, q, c, m = row(x[b, :n], g, dtype, floor, mutant)
        nf = f.shape[0]
        fr[b, :nf], pk[b, :nf], cp[b, :nf], mg[b, :nf] = f, q, c, m
    return fr, pk, cp, mg


def err(got, ref):
    """max over the entries of |got - ref| / max(|ref|, 1)."""
    got, ref = np.asarray(got).astype(np.longdouble), np.asarray(ref).astype(np.longdouble)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1)))


def ragged_lens(H):
    """Three lengths of at least 2500 samples whose frame counts ceil(len / H) are 15, 0 and 1 modulo 16."""
    m = -(-(-(-2500 // H)) // 16) * 16
    return [(m - 2) * H + min(3, H - 1), m * H, m * H + 1]


def rows_for(g, seed=0):
    """(x (3, L), lens): speech_like at 22050 Hz at the ragged lengths of the geometry's hop, 50.0 behind every row's length."""
    rows = [speech_like(n, seed=seed + i, fs=FS) for i, n in enumerate(ragged_lens(g.H))]
    x, _, lens = padded([(r, r) for r in rows], tail=29)
    return x, lens


def harmonic_tone(n, f0=147.0, harmonics=29, sr=FS, amp=0.02):
    """``harmonics`` equal-amplitude harmonics of f0 (29 x 147 Hz stays under 5 kHz), float32."""
    t = np.arange(n, dtype=np.float64) / sr
    return (amp * sum(np.sin(2 * np.pi * h * f0 * t + 0.37 * h * h) for h in range(1, harmonics + 1))).astype(np.float32)


def white_noise(n, rms, seed=0):
    return (rms * np.random.default_rng(900 + seed).standard_normal(n)).astype(np.float32)
