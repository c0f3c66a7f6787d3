"""The numpy restatement of ev_phase_vocoder (include/emojivoice.h: analysis, time steps, propagation, synthesis), generic in the dtype: float64,
the arithmetic of the device, and longdouble, the yardstick of the input condition.  librosa is not installed and is not the yardstick; the header's
text is the definition and this module says it again.  The DFTs are matrix products on the bases the header names (w_j cos, w_j sin from the
float64 tables the device receives); the time steps s_t = (double)t * rate are ALWAYS float64, in either dtype: they are part of the definition
(t * 1.7 floors differently in long double and would select another frame).

Also here: the geometries, rates and input classes of tests/test_gpu_phase_vocoder.py and tests/test_phase_vocoder_host.py, the project's float64
margin TOL and the input condition INPUT_TOL, and the mutants of the definition the host tests hold the restatement against.

Inputs are broadband on purpose: a bin at rounding-noise level has an arbitrary angle, the accumulated phase carries that angle into every later
frame, and such an input is ill-conditioned, not a device error.  So the speech-like class is harmonics with a gliding f0 under an amplitude
envelope PLUS white noise 20 dB below; the condition (float64 and longdouble agree within INPUT_TOL) is asserted per case where it is used.
"""
import numpy as np

TOL = 1e-9                               # the project's float64 margin, relative to the row's largest |Y| / the row's peak
INPUT_TOL = 1e-11                        # float64 against longdouble: the input is well-conditioned
TWO_PI = 6.283185307179586
FLT_MIN = 1.1754943508222875e-38
RATE_MIN, RATE_MAX = 0.125, 8.0
NFFTS = (16, 64, 256, 1024, 2048)
RATES_64 = (1.0, 0.8, 1.25, 0.5, 1.7, 3.7, 0.125, 8.0)
SYNTH_OWNED = 13                         # hop segments a workgroup of pv_synthesis_kernel owns (16 frames - 3)
MUTANTS = ("a_swapped", "round_for_floor", "phasor_after_update", "advance_from_previous", "c_two_at_edges", "wss_without_squares", "out_len_by_floor")


def window(nfft):
    """The periodic Hann window (scipy.signal.get_window("hann", nfft, fftbins=True)), float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(nfft), dtype=np.float64) / int(nfft))


def twiddle(nfft):
    """(nfft, 2) float64 {cos, sin}(2 pi n / nfft)."""
    a = 2.0 * np.pi * np.arange(int(nfft), dtype=np.float64) / int(nfft)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def frames_of(n, nfft):
    return 1 + int(n) // (int(nfft) // 4) if n >= 1 else 0


def steps_of(nf, rate):
    return int(np.ceil(np.float64(nf) / np.float64(rate))) if nf > 0 else 0


def out_len_of(n, rate):
    return int(np.rint(np.float64(n) / np.float64(rate))) if n >= 1 else 0


def out_shape(L, rate, nfft):
    """(L_out, NF, NO) of a batch of rows of L samples."""
    NF = 1 + int(L) // (int(nfft) // 4)
    return int(np.rint(np.float64(L) / np.float64(rate))), NF, steps_of(NF, rate)


def time_steps(n_out, rate, mutant=None):
    """(i_t, a_t) for t < n_out: float64 whatever the dtype of the rest."""
    s = np.arange(n_out, dtype=np.float64) * np.float64(rate)
    i = np.floor(s)
    a = s - i
    if mutant == "round_for_floor":
        i = np.floor(s + 0.5)
    return i.astype(np.int64), a


_BASES = {}


def bases(nfft, dtype, w=None, tw=None):
    """(C, S) (nfft, NB): w_j cos(2 pi j k / nfft), w_j sin(2 pi j k / nfft) from the float64 tables, the phase index in exact integers; and the
    plain (cos, sin) pair for the synthesis.  (Those of the default tables are kept, read-only.)"""
    if w is None and tw is None:
        key = (int(nfft), np.dtype(dtype).name)
        if key not in _BASES:
            _BASES[key] = bases(nfft, dtype, window(nfft), twiddle(nfft))
            for a in _BASES[key]:
                a.setflags(write=False)
        return _BASES[key]
    w = window(nfft) if w is None else np.asarray(w, np.float64)
    tw = twiddle(nfft) if tw is None else np.asarray(tw, np.float64)
    NB = nfft // 2 + 1
    ph = (np.arange(nfft)[:, None] * np.arange(NB)[None, :]) % nfft
    c, s = tw[ph, 0].astype(dtype), tw[ph, 1].astype(dtype)
    wd = w.astype(dtype)[:, None]
    return wd * c, wd * s, c, s


def analysis(x, n, nfft, dtype=np.float64, w=None, tw=None):
    """(mag, ang) (nf + 2, NB) of the first n samples of x: the two all-zero frames behind frame nf - 1 included.  Also (re, im) (nf, NB)."""
    H, NB = nfft // 4, nfft // 2 + 1
    nf = frames_of(n, nfft)
    C, S, _, _ = bases(nfft, dtype, w, tw)
    pad = np.zeros(n + 2 * nfft, dtype)
    pad[nfft // 2: nfft // 2 + n] = np.asarray(x[:n], np.float32).astype(dtype)
    T = np.stack([pad[f * H: f * H + nfft] for f in range(nf)])
    re, im = T @ C, -(T @ S)
    mag = np.zeros((nf + 2, NB), dtype)
    ang = np.zeros((nf + 2, NB), dtype)
    mag[:nf] = np.sqrt(im * im + re * re)
    ang[:nf] = np.arctan2(im, re)
    return mag, ang, re, im


def propagate(mag, ang, nf, rate, nfft, dtype=np.float64, mutant=None):
    """Y (n_out, NB) as (re, im): per bin, ascending t, sequentially (vectorised over the bins only)."""
    H, NB = nfft // 4, nfft // 2 + 1
    n_out = steps_of(nf, rate)
    it, at = time_steps(n_out, rate, mutant)
    two_pi = dtype(TWO_PI)
    omega = (two_pi * (H * np.arange(NB)).astype(dtype)) / dtype(nfft)
    yr, yi = np.zeros((n_out, NB), dtype), np.zeros((n_out, NB), dtype)
    phi = ang[0].copy()
    z = np.zeros(NB, dtype)
    for t in range(n_out):
        i, a = int(it[t]), dtype(at[t])
        m0, m1, a0, a1 = mag[i], mag[i + 1], ang[i], ang[i + 1]
        if mutant == "advance_from_previous":
            a0, a1 = (ang[i - 1] if i >= 1 else z), ang[i]
        m = ((dtype(1) - a) * m1 + a * m0) if mutant == "a_swapped" else ((dtype(1) - a) * m0 + a * m1)
        d = a1 - a0 - omega
        d = d - two_pi * np.rint(d / two_pi)
        nxt = phi + (omega + d)
        if mutant == "phasor_after_update":
            phi = nxt
        yr[t], yi[t] = m * np.cos(phi), m * np.sin(phi)
        phi = nxt
    return yr, yi


def synthesis(yr, yi, n, rate, nfft, size, dtype=np.float64, mutant=None, w=None, tw=None):
    """y (size,) in dtype, NOT yet rounded to float32: the windowed inverse DFT of every frame, the overlap-add in ascending t, the division by
    the window's sum of squares, zeros from min(out_len, H (n_out - 1) + nfft / 2) on."""
    H, NB = nfft // 4, nfft // 2 + 1
    n_out = yr.shape[0]
    w64 = window(nfft) if w is None else np.asarray(w, np.float64)
    wd = w64.astype(dtype)
    _, _, c, s = bases(nfft, dtype, w, tw)
    ck = np.full(NB, 2, dtype)
    if mutant != "c_two_at_edges":
        ck[0] = ck[-1] = 1
    s = s.copy()
    s[:, 0] = 0
    s[:, -1] = 0                                                         # irfft: the imaginary parts of DC and Nyquist are ignored
    g = (wd / dtype(nfft))[None, :] * ((yr * ck) @ c.T + (-(yi * ck)) @ s.T)
    total = H * (n_out - 1) + nfft if n_out > 0 else 0
    num, wss = np.zeros(total, dtype), np.zeros(total, dtype)
    wsq = wd if mutant == "wss_without_squares" else wd * wd
    for t in range(n_out):
        num[t * H: t * H + nfft] = num[t * H: t * H + nfft] + g[t]
        wss[t * H: t * H + nfft] = wss[t * H: t * H + nfft] + wsq
    big = wss > FLT_MIN
    y = np.where(big, num / np.where(big, wss, 1), num)[nfft // 2:]
    out_len = out_len_of(n, rate)
    if mutant == "out_len_by_floor":
        out_len = int(np.floor(np.float64(n) / np.float64(rate)))
    lim = min(out_len, H * (n_out - 1) + nfft // 2, size) if n_out > 0 else 0
    out = np.zeros(size, dtype)
    out[:lim] = y[:lim]
    return out, out_len


def stretch_row(x, n, rate, nfft, size=None, dtype=np.float64, mutant=None):
    """One row -> {"nf", "n_out", "out_len", "Y" (n_out, NB, 2), "y" (size,)} in dtype; size defaults to out_len."""
    NB = nfft // 2 + 1
    if n < 1 or n > len(x):
        return {"nf": 0, "n_out": 0, "out_len": 0, "Y": np.zeros((0, NB, 2), dtype), "y": np.zeros(size or 0, dtype)}
    nf = frames_of(n, nfft)
    mag, ang, _, _ = analysis(x, n, nfft, dtype)
    yr, yi = propagate(mag, ang, nf, rate, nfft, dtype, mutant)
    y, out_len = synthesis(yr, yi, n, rate, nfft, out_len_of(n, rate) if size is None else size, dtype, mutant)
    return {"nf": nf, "n_out": yr.shape[0], "out_len": out_len, "Y": np.stack([yr, yi], axis=-1), "y": y}


def stretch(x, lens, rate, nfft, dtype=np.float64):
    """ev_phase_vocoder on the host: x (B, L) float32, lens (B,) or None -> {"y" (B, L_out) dtype (before the float32 rounding), "out_len" (B,)
    int32, "counts" (B, 2) int32, "stretch" (B, NO, NB, 2) dtype}."""
    x = np.asarray(x, np.float32)
    B, L = x.shape
    L_out, _, NO = out_shape(L, rate, nfft)
    NB = nfft // 2 + 1
    res = {"y": np.zeros((B, L_out), dtype), "out_len": np.zeros(B, np.int32), "counts": np.zeros((B, 2), np.int32),
           "stretch": np.zeros((B, NO, NB, 2), dtype)}
    for b in range(B):
        n = L if lens is None else int(lens[b])
        r = stretch_row(x[b], n, rate, nfft, L_out, dtype)
        res["y"][b], res["out_len"][b], res["counts"][b] = r["y"], r["out_len"], (r["nf"], r["n_out"])
        res["stretch"][b, : r["n_out"]] = r["Y"]
    return res


def rows_stub(x, lengths, rate, n_fft):
    """The ``rows=`` hook of audio.time_stretch on the host: torch in, torch out, through ``stretch``."""
    import torch

    r = stretch(x.cpu().numpy(), None if lengths is None else np.asarray(lengths.cpu()), float(rate), int(n_fft))
    return torch.from_numpy(r["y"].astype(np.float32)), torch.from_numpy(r["out_len"])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
def speech_like(n, seed):
    """Harmonics of a gliding f0 (0.02 -> 0.03 cycles per sample) under a slow amplitude envelope, plus white noise 20 dB below; float32, peak
    under 1."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f0 = 0.02 + 0.01 * t / max(n - 1, 1)
    ph = 2.0 * np.pi * np.cumsum(f0)
    h = np.zeros(n)
    for k in range(1, 16):
        h += np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k
    h *= 0.6 + 0.4 * np.sin(2.0 * np.pi * t / 311.0)
    h /= np.sqrt(np.mean(h * h)) if n > 1 else 1.0
    y = h + 0.1 * rng.standard_normal(n)
    return (0.5 * y / np.max(np.abs(y))).astype(np.float32)


def noise(n, seed):
    return (0.25 * np.random.default_rng(seed).standard_normal(n)).clip(-1, 1).astype(np.float32)


INPUTS = {"speech": speech_like, "noise": noise}


def batch(lens, L, kind="speech", seed=0, behind=50.0):
    """(B, L) float32: row b holds lens[b] samples of the class (seeded per row) and ``behind`` from there on (lens[b] outside 1 .. L: all of it)."""
    x = np.full((len(lens), L), behind, np.float32)
    for b, n in enumerate(lens):
        if 1 <= n <= L:
            x[b, :n] = INPUTS[kind](n, 1000 * seed + b)
    return x


def lens_for(nfft, base_frames, residues=(15, 0, 1), mod=16):
    """Three lengths whose frame counts nf = 1 + n / H are base_frames + the first values >= 0 with nf % mod in ``residues``, none a multiple of H."""
    H = nfft // 4
    out = []
    for k, r in enumerate(residues):
        nf = base_frames + (r - base_frames) % mod
        out.append((nf - 1) * H + (1 + 2 * k) % H if H > 1 else nf - 1)
    return out
