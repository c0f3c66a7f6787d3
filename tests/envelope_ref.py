"""The numpy float64 restatement of ev_envelope (include/emojivoice.h, steps 1 to 7): CheapTrick's envelope on given periods and its warped
cepstrum.  A plain module, imported by tests/test_envelope_host.py and tests/test_gpu_envelope.py; it is the definition the device is held to, not
pyworld or pysptk (neither is a dependency).  Sums are numpy's (pairwise): the device's orders differ in the last bits, far under the 1e-9 gate.

``envelope(..., mutant=)`` restates the definition with one deliberate error each (MUTANTS), to show that the gate sees it.
"""
import numpy as np

FLOOR = 1e-7
Q1 = -0.15
MUTANTS = ("no-mean-removal", "dc-on-corrected", "cell-offset-half", "no-compensation", "c0-not-halved")


def frames_of(n, L, H):
    n = n if 1 <= n <= L else 0
    return -(-n // H)


def t_max(nfft):
    return (nfft - 3) / 3.0


def period_of(p32, nfft, default_period):
    """(T, class) of one float32 period: class 0 keeps it, class 1 takes the default period."""
    T = float(np.float32(p32))
    ok = T > 0.0 and 2.0 <= T <= t_max(nfft)
    return (T, 0) if ok else (float(default_period), 1)


def window_frame(x, n, c, T, mutant=None):
    """Step 1: (s[-half .. half], half) of the frame centred at c of the row x[:n]."""
    half = int(np.floor(1.5 * T + 0.5))
    j = np.arange(-half, half + 1)
    w = 0.5 * np.cos(np.pi * j / (1.5 * T)) + 0.5
    idx = c + j
    ok = (idx >= 0) & (idx < n)
    xv = np.where(ok, x[np.clip(idx, 0, max(n - 1, 0))].astype(np.float64), 0.0)
    xw = xv * w
    ratio = 0.0 if mutant == "no-mean-removal" else xw.sum() / w.sum()
    return (xw - w * ratio) / np.sqrt((w * w).sum()), half


def power_spectrum(s, half, nfft):
    buf = np.zeros(nfft)
    buf[np.arange(-half, half + 1) % nfft] = s
    X = np.fft.rfft(buf)
    return X.real * X.real + X.imag * X.imag


def dc_correct(P, T, nfft, mutant=None):
    """Step 3 -> (P', kd)."""
    NB = nfft // 2 + 1
    rn = nfft / T
    kd = int(np.floor(rn))
    out = P.copy()
    src = out if mutant == "dc-on-corrected" else P                      # (the mutant reads what it has already corrected)
    for k in range(kd + 1):
        u = rn - k
        i = int(np.floor(u))
        fu = u - i
        out[k] = P[k] + (src[i] * (1.0 - fu) + src[min(i + 1, NB - 1)] * fu)
    return out, kd


def mirrored(Pc, nfft, pad):
    """ext[i + pad] = P'[the index i mirrored at 0 and at nfft / 2] for -pad <= i <= nfft / 2 + pad."""
    i = np.arange(-pad, nfft // 2 + pad + 1)
    i = np.where(i < 0, -i, i)
    return Pc[np.where(i > nfft // 2, nfft - i, i)]


def smooth_direct(Pc, T, nfft, mutant=None):
    """Step 4, the direct sum."""
    NB = nfft // 2 + 1
    wd = (2.0 * nfft) / (3.0 * T)
    hw = 0.5 * wd
    pad = nfft // 6 + 3
    ext = mirrored(Pc, nfft, pad)
    off = 0.0 if mutant == "cell-offset-half" else 0.5                   # (the mutant's cell i covers [i, i + 1))
    S = np.empty(NB)
    for k in range(NB):
        lo, hi = k - hw, k + hw
        ilo, ihi = int(np.floor(lo + off)), int(np.floor(hi + off))
        if ilo == ihi:
            acc = ext[ilo + pad] * (hi - lo)
        else:
            acc = ext[ilo + pad] * ((ilo + 1.0 - off) - lo) + ext[ilo + 1 + pad: ihi + pad].sum() + ext[ihi + pad] * (hi - (ihi - off))
        S[k] = acc / wd
    return S


def smooth_cumulative(Pc, T, nfft):
    """Step 4 the way WORLD takes it: the integral of the piecewise-constant P' as a difference of its cumulative sum, linearly interpolated."""
    NB = nfft // 2 + 1
    wd = (2.0 * nfft) / (3.0 * T)
    pad = nfft // 6 + 3
    ext = mirrored(Pc, nfft, pad)
    edges = np.arange(-pad, nfft // 2 + pad + 2) - 0.5                   # cell i covers [edges[i + pad], edges[i + pad + 1])
    cum = np.concatenate([[0.0], np.cumsum(ext)])
    k = np.arange(NB)
    return (np.interp(k + 0.5 * wd, edges, cum) - np.interp(k - 0.5 * wd, edges, cum)) / wd


def cos_table(nfft):
    """(NB, NB) g[k] cos(2 pi k q / nfft) with the phase reduced in integers."""
    NB = nfft // 2 + 1
    k = np.arange(NB)
    g = np.where((k == 0) | (k == nfft // 2), 1.0, 2.0)
    return g[:, None] * np.cos(2.0 * np.pi * ((k[:, None] * k[None, :]) % nfft) / nfft)


def lifter(T, nfft, q1=Q1, mutant=None):
    q = np.arange(nfft // 2 + 1)
    x = q / T
    sinc = np.where(q == 0, 1.0, np.sin(np.pi * x) / np.where(q == 0, 1.0, np.pi * x))
    comp = 1.0 if mutant == "no-compensation" else (1.0 - 2.0 * q1) + (2.0 * q1) * np.cos(2.0 * np.pi * x)
    return sinc * comp


def frame_envelope(x, n, c, T, nfft, A, tab, q1=Q1, floor=FLOOR, mutant=None):
    """One frame -> (Le (NB) or None when silent, mc (n_mcep), half, kd, the liftered cepstrum)."""
    s, half = window_frame(x, n, c, T, mutant)
    P = power_spectrum(s, half, nfft)
    Pc, kd = dc_correct(P, T, nfft, mutant)
    if not (P > floor).any():
        return None, None, half, kd, None
    Lg = np.log(np.maximum(smooth_direct(Pc, T, nfft, mutant), floor))
    cl = (Lg @ tab) / nfft * lifter(T, nfft, q1, mutant)                 # tab[k][q] = g[k] cos: c^[q] = (1 / nfft) sum_k g[k] Lg[k] cos
    Le = tab.T @ cl                                                      # Le[k] = sum_q g[q] c'[q] cos
    c1 = cl.copy()
    if mutant != "c0-not-halved":
        c1[0] = 0.5 * c1[0]
    return Le, A @ c1, half, kd, cl


def envelope(x, lens, period, H, nfft, A, default_period, q1=Q1, floor=FLOOR, mutant=None):
    """ev_envelope on the host: x (B, L) float32, lens (B,) or None, period (B, NF) float32 -> {"env" (B, NF, NB), "mcep" (B, NF, n_mcep),
    "class" (B, NF, 3) int32}."""
    x = np.asarray(x, dtype=np.float32)
    B, L = x.shape
    NF, NB = -(-L // H), nfft // 2 + 1
    A = np.asarray(A, dtype=np.float64)
    env, mcep, cls = np.zeros((B, NF, NB)), np.zeros((B, NF, A.shape[0])), np.zeros((B, NF, 3), np.int32)
    cls[:, :, 0] = 3
    tab = cos_table(nfft)
    for b in range(B):
        n = L if lens is None else int(lens[b])
        n = n if 1 <= n <= L else 0
        for f in range(frames_of(n, L, H)):
            T, k = period_of(period[b, f], nfft, default_period)
            Le, mc, half, kd, _ = frame_envelope(x[b], n, f * H + H // 2, T, nfft, A, tab, q1, floor, mutant)
            cls[b, f] = (2 if Le is None else k, half, kd)
            if Le is not None:
                env[b, f], mcep[b, f] = Le, mc
    return {"env": env, "mcep": mcep, "class": cls}


# ---- signals ------------------------------------------------------------------------------------------------------------------------------------
def harmonic_row(n, T, seed, noise_db=-60.0, amp=0.3):
    """n samples of a harmonic sum at the period T (harmonic h at 1 / h, below the Nyquist frequency) plus seeded white noise ``noise_db`` under
    the sum's rms: the range of P inside a frame is bounded, so the restatement's own rounding stays far under the gate."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    y = np.zeros(n)
    for h in range(1, int(T / 2.0 - 1e-9) + 1):
        y += np.cos(2.0 * np.pi * h * t / T + rng.uniform(0, 2 * np.pi)) / h
    y *= amp / np.sqrt(np.mean(y * y))
    y += rng.standard_normal(n) * amp * 10.0 ** (noise_db / 20.0)
    return y.astype(np.float32)


def pulse_train(n, T, f_hi_norm):
    """A band-limited pulse train at the period T: equal-amplitude cosine harmonics up to f_hi_norm (cycles per sample), all in phase."""
    t = np.arange(n, dtype=np.float64)
    y = np.zeros(n)
    for h in range(1, int(f_hi_norm * T) + 1):
        y += np.cos(2.0 * np.pi * h * t / T)
    return y


def padded(rows, L=None, fill=np.nan):
    """Rows of different lengths as (B, L) float32 with ``fill`` behind each row's length, and the lengths."""
    L = max(len(r) for r in rows) if L is None else L
    x = np.full((len(rows), L), fill, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, [len(r) for r in rows]
