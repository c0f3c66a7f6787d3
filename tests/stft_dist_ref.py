"""numpy restatement of ev_stft_dist (include/emojivoice.h): the per-frame terms of the multi-resolution STFT distance (Yamamoto et al. 2020) and
of the log-spectral distance at ONE resolution (n_fft, hop, win), as frames x basis matrix products, in float64 and — the same definition,
the same float64 basis entries — in np.longdouble.  The device runs one fixed order of its own, so it differs from the float64 restatement
by float64 rounding; the longdouble evaluation measures how much rounding the INPUT admits (tests/test_gpu_stft_dist.py states the rule).

    frames(n) = n > nfft / 2 ? 1 + n / H : 0
    t_f[j]    = x[refl(f H - W / 2 + j)],  refl(i) = -i below 0, 2 (len - 1) - i from len on
    c[j][k]   = w[j] cos_tab[((j + off) k) mod nfft],  s[j][k] = w[j] sin_tab[...],  off = (nfft - W) / 2,  k < NB = nfft / 2 + 1
    p         = max(sm^2 + re^2, floor),  m = sqrt(p),  l = log(p)
    frame[f]  = {sum_k (my - mx)^2, sum_k mx^2, sum_k |ly - lx|, sum_k (ly - lx)^2}
    sums      = {sum_f [0], sum_f [1], sum_f [2], sum_f sqrt([3] / NB)}
"""
import numpy as np

from stoi_ref import GARBAGE, padded, processed, speech_like  # noqa: F401  (the generators of the STOI tests; padded puts 50 / -50 behind a row)

TOL = 1e-9                       # device against the float64 restatement, relative, every entry of d_frame and d_sums
INPUT_TOL = 1e-11                # float64 against longdouble restatement, relative, every entry: the condition on the input
POWER_FLOOR = 1e-7
FS = 22050
SNR_DB = 20.0
GEOMETRIES = ((64, 10, 24), (512, 50, 240), (1024, 120, 600), (2048, 240, 1200))      # (nfft, H, W)
# hops under 4 (the skew walk pads inside a step), a skew of 3 at a hop that is not 2 mod 4, W / 4 = 2 and 1 (the first round's clamp)
EDGE_GEOMETRIES = ((16, 1, 8), (16, 3, 4))
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))                   # audio.MSTFT_RESOLUTIONS: (n_fft, hop, win)


def hann(W):
    """The periodic Hann window, float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(W), dtype=np.float64) / int(W))


def twiddle(nfft):
    a = 2.0 * np.pi * np.arange(int(nfft), dtype=np.float64) / int(nfft)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def frames(n, nfft, H):
    return 1 + n // H if n > nfft // 2 else 0


def basis(nfft, W, window=None, tw=None):
    """(c, s), each (W, NB) float64: every entry one float64 product, the phase index in exact integers."""
    window = hann(W) if window is None else np.asarray(window, dtype=np.float64)
    tw = twiddle(nfft) if tw is None else np.asarray(tw, dtype=np.float64)
    off = (nfft - W) // 2
    idx = ((np.arange(W)[:, None] + off) * np.arange(nfft // 2 + 1)[None, :]) % nfft
    return window[:, None] * tw[idx, 0], window[:, None] * tw[idx, 1]


def frame_matrix(x, nfft, H, W, fold="reflect"):
    """(nf, W): frame f holds x[refl(f H - W / 2 + j)].  ``fold``: "reflect" is the definition; "edge" (repeat the border sample) and
    "reflect_even" (the half-sample mirror, -i - 1 and 2 len - 1 - i) are the wrong folds the reflection test must tell apart."""
    n = len(x)
    nf = frames(n, nfft, H)
    i = np.arange(nf)[:, None] * H - W // 2 + np.arange(W)[None, :]
    if fold == "reflect":
        i = np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    elif fold == "edge":
        i = np.clip(i, 0, n - 1)
    else:
        i = np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    return np.asarray(x)[i].reshape(nf, W)


def spectra(x, geom, dtype=np.float64, floor=POWER_FLOOR, fold="reflect", window=None):
    """(nf, NB) clamped powers of one row."""
    nfft, H, W = geom
    c, s = basis(nfft, W, window)
    t = frame_matrix(np.asarray(x, dtype=np.float64), nfft, H, W, fold).astype(dtype)
    re, sm = t @ c.astype(dtype), t @ s.astype(dtype)
    return np.maximum(sm * sm + re * re, dtype(floor))


def row(x, y, geom, dtype=np.float64, floor=POWER_FLOOR, fold="reflect"):
    """One row -> (frame (nf, 4), sums (4,), nf) in ``dtype``."""
    nfft = geom[0]
    NB = nfft // 2 + 1
    px, py = spectra(x, geom, dtype, floor, fold), spectra(y, geom, dtype, floor, fold)
    mx, my = np.sqrt(px), np.sqrt(py)
    dl = np.log(py) - np.log(px)
    fr = np.stack([((my - mx) ** 2).sum(1), (mx * mx).sum(1), np.abs(dl).sum(1), (dl * dl).sum(1)], axis=1).reshape(-1, 4)
    sums = np.array([fr[:, 0].sum(), fr[:, 1].sum(), fr[:, 2].sum(), np.sqrt(fr[:, 3] / dtype(NB)).sum()], dtype=dtype)
    return fr, sums, fr.shape[0]


def batch(x, y, lens, geom, dtype=np.float64, floor=POWER_FLOOR, fold="reflect"):
    """ev_stft_dist's shapes: x, y (B, L), lens (B,) or None -> frame (B, NF, 4), sums (B, 4), counts (B,) int32; a row with len < 1,
    len > L or len <= nfft / 2 is a row of zeros; nothing at or behind a row's length is looked at."""
    x, y = np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y))
    B, L = x.shape
    nfft, H, _ = geom
    lens = [L] * B if lens is None else [int(v) for v in lens]
    NF = frames(L, nfft, H)
    fr, sums, counts = np.zeros((B, NF, 4), dtype), np.zeros((B, 4), dtype), np.zeros(B, np.int32)
    for b, n in enumerate(lens):
        if n < 1 or n > L or n <= nfft // 2:
            continue
        f, s, nf = row(x[b, :n], y[b, :n], geom, dtype, floor, fold)
        fr[b, :nf], sums[b], counts[b] = f, s, nf
    return fr, sums, counts


def figures(sums, counts, nfft):
    """(sc, log_mag, lsd_db) of every row as the caller takes them from d_sums and d_counts; NaN for a row without a frame."""
    s, nf = np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where(nf > 0, np.sqrt(s[:, 0] / np.where(nf > 0, s[:, 1], 1.0)), np.nan)
        lm = np.where(nf > 0, 0.5 * s[:, 2] / (np.maximum(nf, 1) * (nfft // 2 + 1)), np.nan)
        lsd = np.where(nf > 0, (10.0 / np.log(10.0)) * s[:, 3] / np.maximum(nf, 1), np.nan)
    return sc, lm, lsd


def rel_err(got, ref):
    """max over the entries of |got - ref| / |ref|; where the reference is exactly 0 the other side must be 0 too."""
    got, ref = np.asarray(got), np.asarray(ref)
    zero = ref == 0
    assert not np.asarray(got)[zero].any(), "an entry that is exactly zero in the reference is not zero"
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got[~zero].astype(np.longdouble) - ref[~zero].astype(np.longdouble)) / np.abs(ref[~zero].astype(np.longdouble))))


def ragged_lens(H):
    """Three lengths between 2500 and 6000 samples whose frame counts 1 + len / H are 15, 0 and 1 modulo 16, none but the last a multiple of
    the hop."""
    m = -(-(2 + 2500 // H) // 16) * 16
    return [(m - 2) * H + min(3, H - 1), (m - 1) * H + H - 1, m * H]


def rows_for(geom, seed=0):
    """(x (3, L), y, lens): speech_like at 22050 Hz against processed(.., 20 dB) at the ragged lengths of the geometry's hop, 50.0 / -50.0
    behind every row's length."""
    pairs = []
    for i, n in enumerate(ragged_lens(geom[1])):
        c = speech_like(n, seed=seed + i, fs=FS)
        pairs.append((c, processed(c, SNR_DB, seed=seed + i)))
    return padded(pairs, tail=29)


def edge_signal(n, W, seed=0):
    """A row that is zero except inside its first and its last W / 2 samples (noise there): only the folds of the first and last frames see it."""
    g = np.random.default_rng(700 + seed)
    x = np.zeros(n, np.float32)
    h = W // 2
    x[:h] = 0.1 * g.standard_normal(h)
    x[n - h:] = 0.1 * g.standard_normal(h)
    return x
