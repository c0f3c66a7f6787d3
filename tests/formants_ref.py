"""numpy restatement of ev_formants (include/emojivoice.h): per frame Burg's linear prediction of the pre-emphasised, windowed samples, the roots
of the prediction polynomial by the Aberth-Ehrlich iteration, and the formants as the roots of the upper half plane inside the band, in
float64 and, from the same float64 window and starting points, in np.longdouble / np.clongdouble.  Vectorised over the frames of a row.  The
device runs one fixed order of its own, so it differs from the float64 restatement by float64 rounding; the longdouble evaluation measures how
much rounding the INPUT admits.

    frames(n)  = ceil(n / H)
    s_f[j]     = x[f H + H / 2 - W / 2 + j],  j = -1 .. W - 1,  ZERO outside [0, len)                  (no reflection)
    y[j]       = w[j] (s_f[j] - pre s_f[j - 1])
    E0         = sum y^2;  E0 <= power_floor: SILENT, every output zero
    Burg       f_0 = b_0 = y;  m = 1 .. p over n = m .. W - 1:  k_m = -2 sum f b' / sum (f^2 + b'^2) (0 where the denominator is 0), b' = b[n - 1];
               a_m[i] = a[i] + k_m a[m - i];  f <- f + k_m b',  b <- b' + k_m f;  gain = (E0 / W) prod (1 - k_m^2)
    roots      Aberth-Ehrlich from z_i = 0.9 exp(i (2 pi i / p + 0.4)); r = P / P' (Horner), s_i = sum_{j != i} 1 / (z_i - z_j), w = r / (1 - r s),
               z -= w; two more iterations after the first with max |w| <= 2^-30; over 64 iterations or a non-finite value: UNCONVERGED (-1)
    formants   roots with Im z > 0 and f_lo < f < sr / 2 - f_lo, f = atan2(Im z, Re z) (sr / (2 pi)), bw = -ln|z| (sr / pi); the n_formants of lowest f
"""
from collections import namedtuple

import numpy as np

from stft_dist_ref import edge_signal, hann  # noqa: F401
from stoi_ref import GARBAGE, padded, speech_like  # noqa: F401

TOL = 1e-9                       # device against the float64 restatement, every entry: |got - ref| <= TOL max(|ref|, 1)
INPUT_TOL = 1e-11                # float64 against longdouble restatement, the same form: the condition on the input
MIN_FREQ_MARGIN = 1e-3           # Hz: the distance of every root's |f| from f_lo and from sr / 2 - f_lo
MAX_REF_ITERS = 32               # both restatements converge within this many iterations on every frame of a device case
MAX_ITERS = 64                   # the definition's bound
STOP = 2.0 ** -30
POWER_FLOOR = 1e-10

Geometry = namedtuple("Geometry", "sr W H order pre f_lo nform")


def geometry(sr, W, H, order, nform=4, f_lo=50.0, pre=None):
    return Geometry(float(sr), int(W), int(H), int(order), float(np.exp(-2.0 * np.pi * 50.0 / sr)) if pre is None else float(pre), float(f_lo), int(nform))


GEOMETRIES = (geometry(2000, 24, 10, 4), geometry(2000, 64, 16, 6), geometry(11025, 512, 128, 10), geometry(11025, 1024, 256, 32))
# W = 8 < 64: most lanes hold no sample, order 2: one conjugate pair at most; W = 70: two samples in some lanes, one or none in the others
EDGE_GEOMETRIES = (geometry(2000, 8, 3, 2), geometry(2000, 70, 7, 5))
IDS = [f"{int(g.sr)}-{g.W}-{g.H}-{g.order}" for g in GEOMETRIES]
EDGE_IDS = [f"{int(g.sr)}-{g.W}-{g.H}-{g.order}" for g in EDGE_GEOMETRIES]
MUTANTS = ("no_pre_emphasis", "autocorrelation_method", "reflect", "ignore_f_lo", "sort_by_bandwidth", "hann_window")


def frames(n, H):
    return -(-int(n) // int(H))


def formant_window(W):
    """Praat's Gaussian window, float64: (exp(-48 ((j + 0.5) / W - 0.5)^2) - e^-12) / (1 - e^-12)."""
    j = np.arange(int(W), dtype=np.float64)
    e = np.exp(-12.0)
    return (np.exp(-48.0 * ((j + 0.5) / int(W) - 0.5) ** 2) - e) / (1.0 - e)


def start_points(p):
    """(p,) complex128: 0.9 exp(i (2 pi i / p + 0.4))."""
    ang = 2.0 * np.pi * np.arange(p, dtype=np.float64) / p + 0.4
    return 0.9 * np.cos(ang) + 1j * (0.9 * np.sin(ang))


def frame_matrix(x, g, reflect=False):
    """(nf, W + 1): frame f holds x[f H + H / 2 - W / 2 + j] for j = -1 .. W - 1, zeros outside the row (``reflect``: the mutant that mirrors)."""
    x = np.asarray(x)
    n = len(x)
    nf = frames(n, g.H)
    i = np.arange(nf)[:, None] * g.H + g.H // 2 - g.W // 2 + np.arange(-1, g.W)[None, :]
    if reflect:
        i = np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    ok = (i >= 0) & (i < n)
    return np.where(ok, x[np.clip(i, 0, n - 1)], 0).reshape(nf, g.W + 1)


def burg(y, p, dtype):
    """y (nf, W) -> (a (nf, p + 1) with a[:, 0] = 1, k (nf, p))."""
    nf, W = y.shape
    f, b = y.copy(), y.copy()
    a = np.zeros((nf, p + 1), dtype)
    a[:, 0] = 1
    ks = np.zeros((nf, p), dtype)
    for m in range(1, p + 1):
        fm, bm = f[:, m:], b[:, m - 1:W - 1]
        num = dtype(-2) * np.sum(fm * bm, axis=1)
        den = np.sum(fm * fm + bm * bm, axis=1)
        k = np.where(den > 0, num / np.where(den > 0, den, dtype(1)), dtype(0))
        ks[:, m - 1] = k
        prev = a.copy()
        for i in range(1, m + 1):
            a[:, i] = prev[:, i] + k * prev[:, m - i]
        fn = fm + k[:, None] * bm
        bn = bm + k[:, None] * fm
        f, b = f.copy(), b.copy()
        f[:, m:], b[:, m:] = fn, bn
    return a, ks


def levinson(y, p, dtype):
    """The autocorrelation method (the mutant): Levinson-Durbin on the biased autocorrelation of y."""
    nf, W = y.shape
    r = np.stack([np.sum(y[:, :W - k] * y[:, k:], axis=1) for k in range(p + 1)], axis=1)
    a = np.zeros((nf, p + 1), dtype)
    a[:, 0] = 1
    ks = np.zeros((nf, p), dtype)
    e = r[:, 0].copy()
    for m in range(1, p + 1):
        acc = sum(a[:, i] * r[:, m - i] for i in range(m))
        k = np.where(e > 0, -acc / np.where(e > 0, e, dtype(1)), dtype(0))
        ks[:, m - 1] = k
        prev = a.copy()
        for i in range(1, m + 1):
            a[:, i] = prev[:, i] + k * prev[:, m - i]
        e = e * (dtype(1) - k * k)
    return a, ks


def aberth(a, dtype):
    """a (nf, p + 1) real, monic -> (z (nf, p) complex, iters (nf,) int: the iterations run, -1 where unconverged)."""
    ctype = np.clongdouble if dtype is np.longdouble else np.complex128
    nf, p1 = a.shape
    p = p1 - 1
    z = np.tile(start_points(p).astype(ctype), (nf, 1))
    left = np.full(nf, -1)                   # iterations still to run after the stop rule fired (-1: it has not)
    iters = np.full(nf, -1)
    run = np.ones(nf, bool)
    eye = np.eye(p, dtype=bool)[None]
    with np.errstate(all="ignore"):
        for it in range(1, MAX_ITERS + 1):
            if not run.any():
                break
            zz, aa = z[run], a[run].astype(ctype)
            pv, dv = np.ones_like(zz), np.zeros_like(zz)
            for i in range(1, p + 1):
                dv = dv * zz + pv
                pv = pv * zz + aa[:, i:i + 1]
            r = pv / dv
            d = zz[:, :, None] - zz[:, None, :]
            s = np.where(eye, 0, 1 / np.where(eye, 1, d)).sum(axis=2)
            w = r / (1 - r * s)
            zz = zz - w
            z[run] = zz
            bad = ~(np.isfinite(zz.real) & np.isfinite(zz.imag)).all(axis=1)
            mx = np.abs(w).max(axis=1)
            idx = np.flatnonzero(run)
            lf = left[idx]
            fired = (lf < 0) & (mx <= STOP)
            lf = np.where(fired, 2, np.where(lf > 0, lf - 1, lf))
            done = (lf == 0) & ~bad
            left[idx] = lf
            iters[idx[done]] = it
            run[idx[done | bad]] = False
    return z, iters


def row(x, g, dtype=np.float64, floor=POWER_FLOOR, mutant=None):
    """One row -> (lpc (nf, p + 2): a_1 .. a_p, gain, E0; formant (nf, nform, 2): Hz, bandwidth Hz; count (nf,) int32; iters (nf,): the
    iterations of the root finder (0 on a silent frame, -1 unconverged); margin (nf,): the smallest distance in Hz of a root's |f| from the
    band's two edges (inf on silent and unconverged frames))."""
    assert mutant is None or mutant in MUTANTS
    p, W, nform = g.order, g.W, g.nform
    win = (hann(W) if mutant == "hann_window" else formant_window(W)).astype(dtype)
    s = frame_matrix(np.asarray(x, dtype=np.float64), g, reflect=mutant == "reflect").astype(dtype)
    nf = s.shape[0]
    pre = dtype(0) if mutant == "no_pre_emphasis" else dtype(g.pre)
    y = win[None, :] * (s[:, 1:] - pre * s[:, :-1])
    E0 = np.sum(y * y, axis=1)
    a, ks = (levinson if mutant == "autocorrelation_method" else burg)(y, p, dtype)
    gain = E0 / dtype(W)
    for m in range(p):
        gain = gain * (dtype(1) - ks[:, m] * ks[:, m])
    z, iters = aberth(a, dtype)
    silent = ~(E0 > dtype(floor))
    lpc = np.concatenate([a[:, 1:], gain[:, None], E0[:, None]], axis=1)
    lpc[silent] = 0
    iters = np.where(silent, 0, iters)
    ok = ~silent & (iters > 0)
    with np.errstate(all="ignore"):
        f = np.arctan2(z.imag, z.real) * (dtype(g.sr) / (dtype(2) * dtype(np.pi)))
        bw = -np.log(np.abs(z)) * (dtype(g.sr) / dtype(np.pi))
    lo, hi = (dtype(0), dtype(g.sr) / 2) if mutant == "ignore_f_lo" else (dtype(g.f_lo), dtype(g.sr) / 2 - dtype(g.f_lo))
    formant = np.zeros((nf, nform, 2), dtype)
    count = np.zeros(nf, np.int32)
    margin = np.full(nf, np.inf)
    for i in range(nf):
        if silent[i]:
            continue
        if not ok[i]:
            count[i] = -1
            continue
        cand = (z[i].imag > 0) & (f[i] > lo) & (f[i] < hi)
        key = bw[i] if mutant == "sort_by_bandwidth" else f[i]
        sel = np.flatnonzero(cand)
        sel = sel[np.argsort(key[sel], kind="stable")][:nform]
        count[i] = len(sel)
        formant[i, :len(sel), 0], formant[i, :len(sel), 1] = f[i][sel], bw[i][sel]
        af = np.abs(f[i]).astype(np.float64)
        margin[i] = float(min(np.abs(af - float(g.f_lo)).min(), np.abs(af - (float(g.sr) / 2 - float(g.f_lo))).min()))
    return lpc, formant, count, iters, margin


def batch(x, lens, g, dtype=np.float64, floor=POWER_FLOOR, mutant=None):
    """ev_formants' shapes: x (B, L), lens (B,) or None -> lpc (B, NF, p + 2), formant (B, NF, nform, 2), count (B, NF) int32, iters (B, NF),
    margin (B, NF); a row with len < 1 or len > L is a row of zeros; nothing at or behind a row's length is looked at."""
    x = np.atleast_2d(np.asarray(x))
    B, L = x.shape
    lens = [L] * B if lens is None else [int(v) for v in lens]
    NF = frames(L, g.H)
    lpc, fm = np.zeros((B, NF, g.order + 2), dtype), np.zeros((B, NF, g.nform, 2), dtype)
    ct, it, mg = np.zeros((B, NF), np.int32), np.zeros((B, NF), np.int64), np.full((B, NF), np.inf)
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        r = row(x[b, :n], g, dtype, floor, mutant)
        nf = r[0].shape[0]
        lpc[b, :nf], fm[b, :nf], ct[b, :nf], it[b, :nf], mg[b, :nf] = r
    return lpc, fm, ct, it, mg


def err(got, ref):
    """max over the entries of |got - ref| / max(|ref|, 1)."""
    got, ref = np.asarray(got).astype(np.longdouble), np.asarray(ref).astype(np.longdouble)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1)))


def ragged_lens(H):
    """Three lengths of at least 2500 samples whose frame counts ceil(len / H) are 3, 0 and 1 modulo 4 (four frames to a workgroup)."""
    m = -(-(-(-2500 // H) + 2) // 4) * 4
    return [(m - 2) * H + min(3, H - 1), m * H, m * H + 1]


def rows_for(g, seed=1):
    """(x (3, L), lens): speech_like at the geometry's rate, seeds 1 .. 3, at the ragged lengths of the geometry's hop, 50.0 behind every row's
    length."""
    rows = [speech_like(n, seed=seed + i, fs=g.sr) for i, n in enumerate(ragged_lens(g.H))]
    x, _, lens = padded([(r, r) for r in rows], tail=29)
    return x, lens


def pole_noise(n, sr, poles, seed=0):
    """White noise through the all-pole filter with the given (frequency Hz, bandwidth Hz) pole pairs, float32."""
    a = np.array([1.0])
    for fc, bw in poles:
        r = np.exp(-np.pi * bw / sr)
        a = np.convolve(a, [1.0, -2.0 * r * np.cos(2.0 * np.pi * fc / sr), r * r])
    e = np.random.default_rng(4000 + seed).standard_normal(n)
    y = np.zeros(n)
    for i in range(n):
        acc = e[i]
        for j in range(1, min(i, len(a) - 1) + 1):
            acc -= a[j] * y[i - j]
        y[i] = acc
    return (0.01 * y).astype(np.float32)


def tone(n, sr, f0=147.0, amp=0.1):
    return (amp * np.sin(2.0 * np.pi * f0 * np.arange(n, dtype=np.float64) / sr)).astype(np.float32)
