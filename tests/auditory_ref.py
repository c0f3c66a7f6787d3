"""numpy restatement of ev_auditory (include/emojivoice.h): per frame the loudness of an auditory spectrum, the spectral flux, the power and the
mel-frequency cepstral coefficients (the descriptors of timbre and dynamics of the eGeMAPS set; Eyben et al. 2016), as two matrix products (frames
x windowed DFT basis, power spectrum x mel table), in float64 and, from the same float64 tables, in np.longdouble.  The device runs one fixed order
of its own, so it differs from the float64 restatement by float64 rounding; the longdouble evaluation measures how much rounding the INPUT admits.

    frames(n)  = ceil(n / H)
    s_f[j]     = x[f H + H / 2 - W / 2 + j], ZERO outside [0, len)                                    (no reflection)
    re, sm     = s_f @ {c, s}                                                                         (ev_stft_dist's basis)
    raw        = sm^2 + re^2,  power = sum_k raw[k]
    E[m]       = sum_k raw[k] mel_w[k][m],  Ef = max(E, floor)
    loudness   = sum_m (eq[m] Ef[m])^compress
    mfcc[i]    = sum_m log(Ef[m]) dct[m][i]
    flux_f     = sqrt(sum_{k_lo <= k < k_hi} (sqrt(raw_f[k]) - sqrt(raw_{f-1}[k]))^2 / (k_hi - k_lo)) for f >= 1,  flux_0 = 0
    frame      = {loudness, flux, power, log(max(power, floor))},  flags = live | 2 (f >= 1),  live = some raw[k] > floor
    A silent frame (not live) keeps its power and its flux; loudness, log-energy, mfcc and bands are zeros.

The tables are the device's arguments: HTK mel triangles on the power spectrum, Hermansky's equal-loudness weights at the band centres, DCT-II
columns 1 .. n_ceps under the HTK lifter, restated here on their own (tests/test_auditory_host.py holds audio.auditory_tables to them).
"""
from collections import namedtuple

import numpy as np

from stft_dist_ref import basis, hann, twiddle  # noqa: F401  (the windowed DFT basis is ev_stft_dist's, entry for entry)
from stoi_ref import GARBAGE, padded, speech_like  # noqa: F401
from voice_quality_ref import EDGE_GEOMETRIES as VQ_EDGE_GEOMETRIES
from voice_quality_ref import GEOMETRIES as VQ_GEOMETRIES
from voice_quality_ref import err, frame_matrix, frames, harmonic_tone  # noqa: F401

TOL = 1e-9                       # device against the float64 restatement, every entry: |got - ref| <= TOL max(|ref|, 1)
INPUT_TOL = 1e-11                # float64 against longdouble restatement, the same form: the condition on the input
POWER_FLOOR = 1e-7
COMPRESS = 0.33
LIFTER = 22.0
FS = 22050
FIGURES = ("loudness", "spectral_flux", "power", "log_energy")
TILE = 15                        # the frames a workgroup of the device adds: its 16 matrix rows carry the frame before them

Geometry = namedtuple("Geometry", "nfft H W sr n_mel n_ceps fmin fmax")


def _of(v, n_mel, n_ceps, fmin, fmax):
    return Geometry(v.nfft, v.H, v.W, v.sr, n_mel, n_ceps, fmin, fmax)


# voice_quality_ref's four: 6 bands from 20-1000 Hz at the 2 kHz ones, 26 bands from 20-8000 Hz at 22050 Hz, 4 cepstra
GEOMETRIES = tuple(_of(v, 6, 4, 20.0, 1000.0) if v.sr == 2000 else _of(v, 26, 4, 20.0, 8000.0) for v in VQ_GEOMETRIES)
IDS = [f"{g.nfft}-{g.H}-{g.W}" for g in GEOMETRIES]
# a hop under 4, a skew of 3, W / 4 = 3 and 4, NB = 9: one bin tile, NBp = 12: three phase-2 steps; 3 bands from 100-1000 Hz and 2 cepstra
EDGE_GEOMETRIES = tuple(_of(v, 3, 2, 100.0, 1000.0) for v in VQ_EDGE_GEOMETRIES)
EDGE_IDS = [f"{g.nfft}-{g.H}-{g.W}" for g in EDGE_GEOMETRIES]
# each a plausible misreading of the definition: name -> the outputs it moves (the others stay equal)
MUTANTS = ("flux_on_power", "flux_from_frame_minus_one", "flux_unnormalised", "log10", "floor_after_log", "eq_after_compress", "reflect",
           "silent_keeps_loudness")
MUTANT_MOVES = {"flux_on_power": ("spectral_flux",), "flux_from_frame_minus_one": ("spectral_flux",), "flux_unnormalised": ("spectral_flux",),
                "log10": ("mfcc",), "floor_after_log": ("mfcc",), "eq_after_compress": ("loudness",),
                "reflect": ("loudness", "spectral_flux", "power", "log_energy", "mfcc", "bands"), "silent_keeps_loudness": ("loudness",)}
OUTPUTS = FIGURES + ("mfcc", "bands", "flags")


def htk_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def htk_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_table(sr, nfft, n_mel, fmin, fmax):
    """((NB, n_mel) triangles on the power spectrum, linear in HTK mel between n_mel + 2 equally spaced corners; the centres in Hz), by loops."""
    NB = nfft // 2 + 1
    corners = np.linspace(float(htk_mel(fmin)), float(htk_mel(fmax)), n_mel + 2)
    w = np.zeros((NB, n_mel))
    for k in range(NB):
        mk = float(htk_mel(k * sr / nfft))
        for m in range(n_mel):
            lo, c, hi = corners[m], corners[m + 1], corners[m + 2]
            if lo < mk <= c:
                w[k, m] = (mk - lo) / (c - lo)
            elif c < mk < hi:
                w[k, m] = (hi - mk) / (hi - c)
    return w, htk_hz(corners[1:-1])


def equal_loudness(f):
    """Hermansky 1990, eq. 4."""
    w2 = (2.0 * np.pi * np.asarray(f, dtype=np.float64)) ** 2
    return (w2 + 56.8e6) * w2 ** 2 / ((w2 + 6.3e6) ** 2 * (w2 + 0.38e9))


def dct_table(n_mel, n_ceps, lifter=LIFTER):
    """(n_mel, n_ceps): DCT-II columns 1 .. n_ceps, sqrt(2 / n_mel) cos(pi i (m + 1 / 2) / n_mel), times 1 + lifter / 2 sin(pi i / lifter)."""
    d = np.zeros((n_mel, n_ceps))
    for i in range(1, n_ceps + 1):
        lift = 1.0 + 0.5 * lifter * np.sin(np.pi * i / lifter) if lifter else 1.0
        for m in range(n_mel):
            d[m, i - 1] = np.sqrt(2.0 / n_mel) * np.cos(np.pi * i * (m + 0.5) / n_mel) * lift
    return d


_TABLES = {}


def tables(g, flux=None, zero_column=None):
    """The host tables of a load, made once per (geometry, flux range, zeroed band) and never modified: window, twiddle, mel_w (NB, n_mel), eq,
    dct (n_mel, n_ceps), k_lo, k_hi (``flux``: (k_lo, k_hi), None: every bin), compress.  ``zero_column``: a band whose filter is all zeros."""
    key = (g, flux, zero_column)
    if key not in _TABLES:
        NB = g.nfft // 2 + 1
        mel_w, centres = mel_table(g.sr, g.nfft, g.n_mel, g.fmin, g.fmax)
        if zero_column is not None:
            mel_w[:, zero_column] = 0.0
        k_lo, k_hi = (0, NB) if flux is None else flux
        t = {"window": hann(g.W), "twiddle": twiddle(g.nfft), "mel_w": mel_w, "eq": equal_loudness(centres), "dct": dct_table(g.n_mel, g.n_ceps),
             "k_lo": int(k_lo), "k_hi": int(k_hi), "compress": COMPRESS}
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


def spectrum(x, g, t, dtype=np.float64, reflect=False, first=0):
    """(nf, NB) raw powers sm^2 + re^2 of one row (``first`` = -1: with the frame before the row in front, nf + 1 rows)."""
    c, s = basis(g.nfft, g.W, t["window"], t["twiddle"])
    x = np.asarray(x, dtype=np.float64)
    fm = frame_matrix(x, g, reflect)
    if first == -1:
        i = -g.H + g.H // 2 - g.W // 2 + np.arange(g.W)
        ok = (i >= 0) & (i < len(x))
        fm = np.concatenate([np.where(ok, x[np.clip(i, 0, len(x) - 1)], 0.0)[None, :], fm], axis=0)
    fm = fm.astype(dtype)
    re, sm = fm @ c.astype(dtype), fm @ s.astype(dtype)
    return sm * sm + re * re


def row(x, g, t, dtype=np.float64, floor=POWER_FLOOR, mutant=None):
    """One row -> {"frame" (nf, 4), "mfcc" (nf, n_ceps), "bands" (nf, n_mel), "flags" (nf,) int32} in ``dtype``."""
    assert mutant is None or mutant in MUTANTS
    raw = spectrum(x, g, t, dtype, reflect=mutant == "reflect", first=-1)
    before, raw = raw[0], raw[1:]
    nf = raw.shape[0]
    fl = dtype(floor)
    power = raw.sum(axis=1)
    E = raw @ t["mel_w"].astype(dtype)
    Ef = np.maximum(E, fl)
    eq, c = t["eq"].astype(dtype)[None, :], dtype(t["compress"])
    loud = (eq * Ef ** c).sum(axis=1) if mutant == "eq_after_compress" else ((eq * Ef) ** c).sum(axis=1)
    if mutant == "log10":
        lg = np.log10(Ef)
    elif mutant == "floor_after_log":
        with np.errstate(divide="ignore"):
            lg = np.maximum(np.log(E), fl)
    else:
        lg = np.log(Ef)
    mfcc = lg @ t["dct"].astype(dtype)
    k_lo, k_hi = t["k_lo"], t["k_hi"]
    sp = raw if mutant == "flux_on_power" else np.sqrt(raw)
    prev = np.concatenate([(before if mutant == "flux_on_power" else np.sqrt(before))[None, :], sp[:-1]], axis=0)
    d = (sp - prev)[:, k_lo:k_hi]
    ss = (d * d).sum(axis=1)
    flux = np.sqrt(ss if mutant == "flux_unnormalised" else ss / dtype(k_hi - k_lo))
    if mutant != "flux_from_frame_minus_one":
        flux[0] = 0
    live = (raw > fl).any(axis=1)
    le = np.log(np.maximum(power, fl))
    silent = ~live
    if mutant != "silent_keeps_loudness":
        loud = np.where(silent, dtype(0), loud)
    le = np.where(silent, dtype(0), le)
    mfcc = np.where(silent[:, None], dtype(0), mfcc)
    bands = np.where(silent[:, None], dtype(0), E)
    flags = live.astype(np.int32) | (2 * (np.arange(nf) >= 1)).astype(np.int32)
    return {"frame": np.stack([loud, flux, power, le], axis=1).reshape(nf, 4), "mfcc": mfcc, "bands": bands, "flags": flags}


def batch(x, lens, g, t, dtype=np.float64, floor=POWER_FLOOR, mutant=None):
    """ev_auditory's shapes: x (B, L), lens (B,) or None -> {"frame" (B, NF, 4), "mfcc" (B, NF, n_ceps), "bands" (B, NF, n_mel), "flags" (B, NF)
    int32}; a row with len < 1 or len > L is a row of zeros; nothing at or behind a row's length is looked at."""
    x = np.atleast_2d(np.asarray(x))
    B, L = x.shape
    lens = [L] * B if lens is None else [int(v) for v in lens]
    NF = frames(L, g.H)
    out = {"frame": np.zeros((B, NF, 4), dtype), "mfcc": np.zeros((B, NF, g.n_ceps), dtype), "bands": np.zeros((B, NF, g.n_mel), dtype),
           "flags": np.zeros((B, NF), np.int32)}
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        r = row(x[b, :n], g, t, dtype, floor, mutant)
        for k, v in r.items():
            out[k][b, :v.shape[0]] = v
    return out


def named(out):
    """The outputs of row / batch by the names of OUTPUTS."""
    o = {k: out["frame"][..., i] for i, k in enumerate(FIGURES)}
    o.update(mfcc=out["mfcc"], bands=out["bands"], flags=out["flags"])
    return o


def ragged_lens(H):
    """Three lengths of at least 2500 samples whose frame counts ceil(len / H) are 14, 0 and 1 modulo 15, the last two over 30: a flux there
    crosses two tile seams."""
    m = max(-(-(-(-2500 // H)) // TILE) * TILE, 2 * TILE)
    return [(m - 2) * H + min(3, H - 1), m * H, m * H + 1]


_ROWS = {}


def rows_for(g, seed=0):
    """(x (3, L), lens): speech_like at 22050 Hz at the ragged lengths of the geometry's hop, 50.0 behind every row's length."""
    key = (g.H, seed)
    if key not in _ROWS:
        rows = [speech_like(n, seed=seed + i, fs=FS) for i, n in enumerate(ragged_lens(g.H))]
        x, _, lens = padded([(r, r) for r in rows], tail=29)
        x.setflags(write=False)
        _ROWS[key] = (x, lens)
    return _ROWS[key]


def going_silent(n, at, seed=0):
    """Noise of rms 0.05 up to sample ``at``, exact zeros from there on, float32."""
    x = (0.05 * np.random.default_rng(300 + seed).standard_normal(n)).astype(np.float32)
    x[at:] = 0.0
    return x
