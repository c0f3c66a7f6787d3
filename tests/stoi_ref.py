"""The yardstick of the STOI / ESTOI tests: a numpy float64 restatement of the published algorithm, and the rows the tests run.

STOI: Taal, Hendriks, Heusdens and Jensen, "An algorithm for intelligibility prediction of time-frequency weighted noisy speech", IEEE TASL
19(7), 2011.  ESTOI: Jensen and Taal, "An algorithm for predicting the intelligibility of speech masked by modulated noise maskers", IEEE/ACM
TASLP 24(11), 2016.  Written from the papers (and the conventions of the authors' published code where the papers leave a choice: the Hann
window without its zero end points, frames at range(0, len - W, H), silent frames chosen on the clean signal at 40 dB below its loudest
frame and the rest overlap-added, the clipping at -15 dB signal-to-distortion ratio).  The spectra come from ``np.fft.rfft``; nothing here
follows the device's order of operations.  One stated difference: ESTOI's normalisations add no random dither (the published code adds
EPS x Gaussian noise before each; the device could not reproduce a host's random stream and 2e-16 does not show at the gate used here).
A clean row of zeros keeps NO frame (the dB test of the model would keep all: every frame sits 0 dB under the maximum); the header of
ev_stoi states the same.

``stoi`` returns per row, besides the outputs of ev_stoi, two conditions on the INPUT that every device comparison asserts first:
  margin        min over frames of |max dB - 40 - frame dB|: how far the nearest frame is from the silence threshold.  A frame at the
                threshold could fall either way under rounding, and the whole silence-removed signal would shift;
  conditioning  min over (segment, band) of ||v - mean(v)|| / ||v|| for v = X and for the clipped Y': a nearly constant band would make the
                normalised vectors, and their correlation, rounding noise.
The gates of the device tests live here: TOL, MIN_MARGIN_DB, MIN_CONDITIONING.

Figures on the CPU for a speech_like row of 20000 samples at 10 kHz (printed and asserted in tests/test_stoi_host.py): nf 155, nk 115,
nseg 85; margin 12.9 dB, conditioning 0.09 to 0.10; STOI 0.950 / 0.615 / 0.308 and ESTOI 0.732 / 0.184 / 0.051 at +20 / 0 / -10 dB SNR;
identical signals give 1 - 1.3e-15 for both.
"""
import numpy as np

EPS = np.finfo(np.float64).eps                     # 2^-52
FS = 10000
DYN_RANGE_DB = 40.0
SILENCE_RATIO = 10.0 ** (-DYN_RANGE_DB / 10.0)     # the 40 dB in the power domain
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)                 # -15 dB signal-to-distortion ratio

TOL = 1e-9                                         # device against this restatement: d_tob relative, d_seg and d_score absolute
MIN_MARGIN_DB = 1e-3
MIN_CONDITIONING = 1e-3
GARBAGE = 50.0                                     # behind every row's length, in both signals

BANDS_15 = [[7, 9], [9, 11], [11, 14], [14, 17], [17, 22], [22, 27], [27, 34], [34, 43], [43, 55], [55, 69], [69, 87], [87, 109], [109, 138],
            [138, 174], [174, 219]]


class Geometry:
    def __init__(self, W, H, nfft, bands, N):
        self.W, self.H, self.nfft, self.N = int(W), int(H), int(nfft), int(N)
        self.bands = np.asarray(bands, dtype=np.int32).reshape(-1, 2)
        self.window = np.hanning(self.W + 2)[1:-1]
        a = 2.0 * np.pi * np.arange(self.nfft, dtype=np.float64) / self.nfft
        self.twiddle = np.stack([np.cos(a), np.sin(a)], axis=1)

    def frames(self, n):
        return len(range(0, n - self.W, self.H)) if n > self.W else 0

    def sizes(self, L):
        NF = self.frames(L)
        NM = max(NF - 1, 0)
        return NF, NM, max(NM - self.N + 1, 0)


STANDARD = Geometry(256, 128, 512, BANDS_15, 30)
SMALL = Geometry(64, 32, 128, [[2, 4], [4, 7], [7, 12]], 4)

# the mutants of tests/test_stoi_host.py: each is a plausible misreading of the papers
VARIANTS = ("nonstrict_mask", "mask_from_processed", "no_clip", "clip_at_plus_15", "mean_before_clip", "n_plus_one", "keep_last_frame",
            "estoi_frames_only")


def _unit(v, axis):
    v = v - v.mean(axis=axis, keepdims=True)
    return v / (np.sqrt(np.sum(v * v, axis=axis, keepdims=True)) + EPS)


def stoi_row(x, y, g, variant=None, dyn_range_db=DYN_RANGE_DB):
    """One row: x clean, y processed, float arrays of one length.  -> dict(keep (nf,) bool, tob (2, n_bands, nm), seg (nseg, 2), score (2,),
    counts (nf, nk, nseg), margin, conditioning).  ``dyn_range_db``: the 40 dB of the silent-frame rule (the strictness test moves it to 0,
    where the loudest frame itself sits exactly on the threshold)."""
    assert variant is None or variant in VARIANTS
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    W, H, w = g.W, g.H, g.window
    N = g.N + 1 if variant == "n_plus_one" else g.N
    nb = len(g.bands)
    starts = list(range(0, len(x) - W, H)) if len(x) > W else []
    nf = len(starts)
    fx = np.array([w * x[s:s + W] for s in starts]).reshape(nf, W)
    fy = np.array([w * y[s:s + W] for s in starts]).reshape(nf, W)
    ref = fy if variant == "mask_from_processed" else fx
    energy = np.sum(ref * ref, axis=1)
    margin = np.inf
    keep = np.zeros(nf, dtype=bool)
    if nf and energy.max() > 0.0:
        db = 20.0 * np.log10(np.sqrt(energy) + EPS)
        d = db.max() - dyn_range_db - db
        keep = d <= 0 if variant == "nonstrict_mask" else d < 0
        margin = float(np.min(np.abs(d)))
    nk = int(keep.sum())

    def removed(frames):
        s = np.zeros((nk - 1) * H + W) if nk else np.zeros(0)
        for k, f in enumerate(frames[keep]):
            s[k * H:k * H + W] += f
        return s

    sx, sy = removed(fx), removed(fy)
    last = len(sx) - W + (1 if variant == "keep_last_frame" else 0)
    st = list(range(0, last, H)) if nk else []
    nm = len(st)
    tob = np.zeros((2, nb, nm))
    for which, s in enumerate((sx, sy)):
        for m, s0 in enumerate(st):
            p = np.abs(np.fft.rfft(w * s[s0:s0 + W], g.nfft)) ** 2
            tob[which, :, m] = [np.sqrt(np.sum(p[a:b])) for a, b in g.bands]
    nseg = max(nm - N + 1, 0)
    seg = np.zeros((nseg, 2))
    cond = np.inf
    clip = {"no_clip": np.inf, "clip_at_plus_15": 1.0 + 10.0 ** (-15.0 / 20.0)}.get(variant, CLIP)
    for q in range(nseg):
        X, Y = tob[0][:, q:q + N], tob[1][:, q:q + N]
        if variant == "mean_before_clip":
            Xc, Yc = X - X.mean(axis=1, keepdims=True), Y - Y.mean(axis=1, keepdims=True)
            a = np.linalg.norm(Xc, axis=1, keepdims=True) / (np.linalg.norm(Yc, axis=1, keepdims=True) + EPS)
            Yp = np.minimum(a * Yc, clip * Xc)
            Xu = Xc / (np.linalg.norm(Xc, axis=1, keepdims=True) + EPS)
            Yu = Yp / (np.linalg.norm(Yp, axis=1, keepdims=True) + EPS)
        else:
            a = np.linalg.norm(X, axis=1, keepdims=True) / (np.linalg.norm(Y, axis=1, keepdims=True) + EPS)
            Yp = np.minimum(a * Y, clip * X)
            for v in (X, Yp):
                nv = np.linalg.norm(v, axis=1)
                cv = np.linalg.norm(v - v.mean(axis=1, keepdims=True), axis=1)
                cond = min(cond, float(np.min(cv / np.maximum(nv, 1e-300))))
            Xu, Yu = _unit(X, 1), _unit(Yp, 1)
        seg[q, 0] = np.sum(Xu * Yu) / nb
        Xe, Ye = _unit(X, 1), _unit(Y, 1)
        if variant != "estoi_frames_only":
            Xe, Ye = _unit(Xe, 0), _unit(Ye, 0)
        seg[q, 1] = np.sum(Xe * Ye) / N
    score = seg.mean(axis=0) if nseg else np.zeros(2)
    return {"keep": keep, "tob": tob, "seg": seg, "score": score, "counts": (nf, nk, nseg), "margin": margin, "conditioning": cond}


def stoi(x, y, lens, g, variant=None):
    """The batch form with ev_stoi's shapes: x, y (B, L) or 1-D, lens (B,) or None -> keep (B, NF) uint8, tob (B, 2, n_bands, NM), seg (B, NSEG, 2),
    score (B, 2), counts (B, 3) int32, margin (B,), conditioning (B,); a row with len < 1 or len > L is a row of zeros; nothing at or behind a
    row's length is looked at."""
    x, y = np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y))
    B, L = x.shape
    lens = [L] * B if lens is None else [int(v) for v in lens]
    NF, NM, NSEG = g.sizes(L)
    nb = len(g.bands)
    out = {"keep": np.zeros((B, NF), np.uint8), "tob": np.zeros((B, 2, nb, NM)), "seg": np.zeros((B, NSEG, 2)), "score": np.zeros((B, 2)),
           "counts": np.zeros((B, 3), np.int32), "margin": np.full(B, np.inf), "conditioning": np.full(B, np.inf)}
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        r = stoi_row(x[b, :n], y[b, :n], g, variant)
        nf, nk, nseg = r["counts"]
        out["keep"][b, :nf] = r["keep"]
        out["tob"][b, :, :, :r["tob"].shape[2]] = r["tob"]
        out["seg"][b, :nseg] = r["seg"]
        out["score"][b] = r["score"]
        out["counts"][b] = r["counts"]
        out["margin"][b], out["conditioning"][b] = r["margin"], r["conditioning"]
    return out


# ---- the rows -------------------------------------------------------------------------------------------------------------------------------
SNRS_DB = (20.0, 0.0, -10.0)


def speech_like(n, seed=0, fs=FS, f0=120.0):
    """A speech-like row of n samples, float32: 24 harmonics (amplitude 1 / h) of an f0 that glides +-20 % at 0.7 Hz, under a syllabic
    envelope (a raised 4 Hz sine between 0.15 and 1), hard-gated: sound for 0.62 s in every 0.9 s, silence for the rest (so that a third of the
    frames are silent frames and kept frames that become neighbours lie far apart in the input), on a noise floor of 1e-4."""
    g = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    inst = f0 * (1.0 + 0.2 * np.sin(2 * np.pi * 0.7 * t + 0.3 * seed))
    phase = 2 * np.pi * np.cumsum(inst) / fs
    s = sum(np.sin(h * phase + 0.37 * h * h) / h for h in range(1, 25))
    env = 0.575 + 0.425 * np.sin(2 * np.pi * 4.0 * t + 1.1)
    gate = ((t + 0.05 * seed) % 0.9) < 0.62
    return (0.12 * s * env * gate + 1e-4 * g.standard_normal(n)).astype(np.float32)


def processed(clean, snr_db, seed=1):
    """clean + white Gaussian noise at snr_db (over the whole row), float32."""
    g = np.random.default_rng(1000 + seed)
    c = np.asarray(clean, dtype=np.float64)
    noise = g.standard_normal(len(c))
    noise *= np.sqrt(np.mean(c * c) / np.mean(noise * noise)) * 10.0 ** (-snr_db / 20.0)
    return (c + noise).astype(np.float32)


def padded(pairs, L=None, tail=0):
    """Rows of different lengths as (x (B, L), y (B, L), lengths): GARBAGE behind every row's length in both signals."""
    lens = [len(a) for a, _ in pairs]
    L = (max(lens) + tail) if L is None else L
    x = np.full((len(pairs), L), GARBAGE, np.float32)
    y = np.full((len(pairs), L), -GARBAGE, np.float32)
    for b, (a, d) in enumerate(pairs):
        x[b, :len(a)], y[b, :len(d)] = a, d
    return x, y, lens


STANDARD_LENS = (20000, 13337, 9000)


def standard_rows():
    """(x (3, 20000), y, lengths 20000 / 13337 / 9000): speech-like rows against themselves at +20, 0 and -10 dB SNR."""
    pairs = []
    for i, (n, snr) in enumerate(zip(STANDARD_LENS, SNRS_DB)):
        c = speech_like(n, seed=i)
        pairs.append((c, processed(c, snr, seed=i)))
    return padded(pairs)


def small_clean(n, seed=0):
    """The small geometry's row (W 64, H 32 at a nominal 10 kHz): speech_like with a fast gate, so that 3000 samples hold several runs."""
    g = np.random.default_rng(100 + seed)
    t = np.arange(n, dtype=np.float64) / FS
    s = sum(np.sin(2 * np.pi * 310.0 * h * t * (1.0 + 0.05 * np.sin(2 * np.pi * 9.0 * t)) + 0.37 * h * h) / h for h in range(1, 13))
    env = 0.575 + 0.425 * np.sin(2 * np.pi * 31.0 * t + 0.4)
    gate = ((t + 0.003 * seed) % 0.09) >= 0.045
    return (0.12 * s * env * gate + 1e-4 * g.standard_normal(n)).astype(np.float32)


def dense_row(n_frames_kept, seed=0):
    """A pair of the small geometry in which EVERY frame is kept and the number of frames is chosen: modulated stationary noise of
    W + (k - 1) H + 1 samples, k frames, against itself at 5 dB SNR."""
    n = SMALL.W + (n_frames_kept - 1) * SMALL.H + 1
    g = np.random.default_rng(300 + seed)
    c = (0.1 * g.standard_normal(n) * (1.0 + 0.5 * np.sin(2 * np.pi * np.arange(n) / 173.0))).astype(np.float32)
    return c, processed(c, 5.0, seed=seed)


def small_lens():
    """Lengths of the small geometry's edge rows: the whole row, nf = 0 (len = W and len = 1), nf = 1 (W + 1: nm = 0), exact multiples
    W + k H (k frames, not k + 1) and one sample more."""
    W, H = SMALL.W, SMALL.H
    return [3000, W, 1, W + 1, W + H, W + H + 1, W + 20 * H, W + 20 * H + 1]


SMALL_COUNTS = [[92, 46, 42], [0, 0, 0], [0, 0, 0], [1, 1, 0], [1, 1, 0], [2, 2, 0], [20, 13, 9], [21, 15, 11], [4, 4, 0], [5, 5, 1]]


def small_rows():
    """(x, y, lengths) at L = 3000: rows of small_clean against 5 dB SNR at the lengths of small_lens(), then two rows that keep every
    frame: N kept frames (nm = N - 1: no segment, score 0) and N + 1 (nm = N: exactly one segment).  SMALL_COUNTS are their (nf, nk, nseg)."""
    pairs = []
    for i, n in enumerate(small_lens()):
        c = small_clean(n, seed=i)
        pairs.append((c, processed(c, 5.0, seed=i)))
    pairs += [dense_row(SMALL.N, seed=1), dense_row(SMALL.N + 1, seed=2)]
    return padded(pairs, L=3000)


SCAN_L = 22400
SCAN_SHAPES = ("first_dropped", "last_dropped", "run_over_64", "run_over_256", "all_kept")


def scan_row(shape, seed=0):
    """A clean / processed pair of SCAN_L samples in the small geometry (698 frames: wider than one workgroup of the device's scan) whose
    mask has the named shape; silence is the 1e-5 floor, 80 dB under the rest."""
    assert shape in SCAN_SHAPES
    g = np.random.default_rng(500 + SCAN_SHAPES.index(shape) + 17 * seed)
    n, W, H = SCAN_L, SMALL.W, SMALL.H
    loud = np.ones(n)
    if shape == "first_dropped":
        loud[:W + H // 2] = 0.0                      # frame 0 lies in silence, frame 1 reaches into the signal
    elif shape == "last_dropped":
        loud[n - W - 3 * H:] = 0.0
    elif shape == "run_over_64":
        loud[100 * H:100 * H + 70 * H + W] = 0.0     # at least 70 whole frames of silence
        loud[400 * H:400 * H + 3 * H + W] = 0.0
    elif shape == "run_over_256":
        loud[150 * H:150 * H + 300 * H + W] = 0.0    # a dropped run that spans more than one round of 256 frames
    t = np.arange(n)
    c = (0.1 * g.standard_normal(n) * (1.0 + 0.5 * np.sin(2 * np.pi * t / 1931.0)) * loud + 1e-5 * g.standard_normal(n)).astype(np.float32)
    return c, processed(c, 3.0, seed=seed + 40)
