"""numpy float64 restatement of the pitch tracker's semantics (include/emojivoice.h): de Cheveigne and Kawahara's
YIN without its final "best local estimate" step.  librosa is not a dependency: the formula below IS the yardstick.

For a row x of len samples, W = frame_length, H = hop_length, n = tau_max + 1:
    frames      ceil(len / H);  frame f analyses s[j] = x[s_f + j], 0 <= j < W + n, s_f = f H + H // 2 - (W + tau_max) // 2, zeros outside [0, len)
    d(tau)      sum_{j < W} (s[j] - s[j + tau])^2,  1 <= tau <= n
    d'(tau)     d(tau) * tau / S(tau) where S(tau) = sum_{k <= tau} d(k) > 0, else 1
    tau0        the smallest tau in [tau_min, tau_max] with d'(tau) < threshold; while tau0 + 1 <= tau_max and d'(tau0 + 1) < d'(tau0): tau0 += 1
    period      tau0 + shift, shift = 0.5 (a - c) / (a - 2 b + c) over a, b, c = d'(tau0 - 1), d'(tau0), d'(tau0 + 1) when the denominator is
                > 0 and |shift| <= 1, else 0
    outputs     lag = tau0, period, cmnd = d'(tau0); an unvoiced frame (no tau0): lag 0, period 0, cmnd = min d' over [tau_min, tau_max]
Frames at or beyond ceil(len / H), and rows with len < 1 or len > L, are zeros.

Every frame also gets its DECISION MARGIN: the least distance of any comparison the decision made from flipping, i.e. the smallest of
|d'(tau) - threshold| over the tau the threshold search inspected (tau_min .. tau0's first value, or all of [tau_min, tau_max] for an
unvoiced frame), |d'(tau + 1) - d'(tau)| over the steps the walk-down compared (the one that stopped it included) and, for an unvoiced
frame, the gap between the two smallest d' of the range.  Where S(tau) = 0 (every d up to tau is an exact zero: a silent frame, or one
that is silent up to lag tau) d' is the constant 1 by definition, not by rounding: nothing can reorder there, so the last term is taken
over the lags with S(tau) > 0 only, and left out where fewer than two remain.  An implementation that sums in another order may differ
from this file only on frames whose margin is of the order of its rounding error.
"""
import numpy as np


def frame_count(length, hop_length):
    return -(-int(length) // int(hop_length))


def frame_span(x, f, frame_length, hop_length, tau_max):
    """The W + tau_max + 1 float64 samples frame f analyses; x holds the row's valid samples only."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    W, H = int(frame_length), int(hop_length)
    n_span = W + int(tau_max) + 1
    s0 = f * H + H // 2 - (W + int(tau_max)) // 2
    out = np.zeros(n_span)
    lo, hi = max(s0, 0), min(s0 + n_span, len(x))
    if hi > lo:
        out[lo - s0: hi - s0] = x[lo:hi]
    return out


def difference(span, frame_length, tau_max):
    """d(tau) for tau = 1 .. tau_max + 1 (index tau - 1)."""
    W, n = int(frame_length), int(tau_max) + 1
    win = np.lib.stride_tricks.sliding_window_view(span, W)[1: n + 1]        # row tau - 1 = s[tau : tau + W]
    diff = win - span[:W]
    return np.einsum("ij,ij->i", diff, diff)


def cmnd(d):
    """d'(tau) for tau = 1 .. len(d) (index tau - 1)."""
    S = np.cumsum(d)
    tau = np.arange(1, len(d) + 1, dtype=np.float64)
    out = np.ones(len(d))
    ok = S > 0
    out[ok] = d[ok] * tau[ok] / S[ok]
    return out


def decide(dp, tau_min, tau_max, threshold):
    """(lag, period, cmnd, margin) of one frame from d' (index tau - 1, length tau_max + 1); the unvoiced frames' gap term of the margin
    is yin_frame's."""
    at = lambda t: float(dp[t - 1])
    margin = np.inf
    tau0 = 0
    for t in range(tau_min, tau_max + 1):
        margin = min(margin, abs(at(t) - threshold))
        if at(t) < threshold:
            tau0 = t
            break
    if tau0 == 0:
        return 0, 0.0, float(np.min(dp[tau_min - 1: tau_max])), margin
    while tau0 + 1 <= tau_max:
        margin = min(margin, abs(at(tau0 + 1) - at(tau0)))
        if not at(tau0 + 1) < at(tau0):
            break
        tau0 += 1
    a, b, c = at(tau0 - 1), at(tau0), at(tau0 + 1)
    den = a - 2.0 * b + c
    shift = 0.0
    if den > 0:
        shift = 0.5 * (a - c) / den
        if not abs(shift) <= 1.0:
            shift = 0.0
    return tau0, tau0 + shift, b, margin


def yin_frame(span, frame_length, tau_min, tau_max, threshold):
    d = difference(span, frame_length, tau_max)
    dp = cmnd(d)
    lag, period, ap, margin = decide(dp, int(tau_min), int(tau_max), float(threshold))
    if lag == 0:
        computed = dp[tau_min - 1: tau_max][np.cumsum(d)[tau_min - 1: tau_max] > 0]
        if computed.size >= 2:
            two = np.partition(computed, 1)[:2]
            margin = min(margin, float(two[1] - two[0]))
    return lag, period, ap, margin


def pitch_yin(x, lengths=None, frame_length=1024, hop_length=256, tau_min=36, tau_max=340, threshold=0.1):
    """x (B, L) or (L,) -> {"lag" (B, F) int32, "period" (B, F) float64, "cmnd" (B, F) float64, "margin" (B, F) float64}, F = ceil(L / H).
    Frames past a row's own count and bad rows: zeros, margin inf."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    B, L = x.shape
    F = frame_count(L, hop_length)
    lens = [L] * B if lengths is None else [int(v) for v in lengths]
    out = {"lag": np.zeros((B, F), np.int32), "period": np.zeros((B, F)), "cmnd": np.zeros((B, F)), "margin": np.full((B, F), np.inf)}
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        for f in range(frame_count(n, hop_length)):
            span = frame_span(x[b, :n], f, frame_length, hop_length, tau_max)
            out["lag"][b, f], out["period"][b, f], out["cmnd"][b, f], out["margin"][b, f] = yin_frame(span, frame_length, tau_min, tau_max, threshold)
    return out


def f0_from_period(period, sr):
    period = np.asarray(period, dtype=np.float64)
    return np.where(period > 0, sr / np.where(period > 0, period, 1.0), 0.0)


# ---- the rows the tests share -----------------------------------------------------------------------------------------------------------
def harmonic_tone(f0, n, sr=22050, amps=(1.0, 0.5, 0.25), scale=0.3):
    t = np.arange(n) / sr
    y = sum(a * np.sin(2 * np.pi * f0 * (k + 1) * t + 0.3 * k) for k, a in enumerate(amps))
    return (scale * y).astype(np.float32)


def chirp(f_start, f_end, n, sr=22050, scale=0.5):
    t = np.arange(n) / sr
    phase = 2 * np.pi * (f_start * t + 0.5 * (f_end - f_start) * t * t / (n / sr))
    return (scale * np.sin(phase)).astype(np.float32)


def mixed_row(n, seed, sr=22050):
    """Thirds: Gaussian noise, silence, a 3-harmonic tone at 180 Hz."""
    g = np.random.default_rng(seed)
    a, b = n // 3, 2 * n // 3
    y = np.zeros(n, dtype=np.float32)
    y[:a] = (0.1 * g.standard_normal(a)).astype(np.float32)
    y[b:] = harmonic_tone(180.0, n - b, sr)
    return y


def interior_frames(n_frames, length, frame_length=1024, hop_length=256, tau_max=340):
    """Mask of the frames whose whole span lies inside [0, length): no zero padding enters them."""
    s0 = np.arange(n_frames) * hop_length + hop_length // 2 - (frame_length + tau_max) // 2
    return (s0 >= 0) & (s0 + frame_length + tau_max + 1 <= length)


# Relative error of the recovered f0 at 22050 Hz, W 1024, H 256, lags 36 .. 340, threshold 0.1, over 8192 samples of a pure sine and of a
# 3-harmonic tone at 110 / 220 / 440 Hz, MEASURED on this restatement (tests/test_pitch_host.py prints and asserts them):
#   interior frames (26 of 32):     sine 5.4e-6 / 4.7e-5 / 2.0e-4    3 harmonics 7.2e-6 / 5.3e-5 / 2.3e-4     worst 2.3e-4
#   every voiced frame (29 .. 32):  sine 5.0e-3 / 5.3e-3 / 1.5e-3    3 harmonics 6.0e-3 / 1.8e-3 / 8.4e-4     worst 6.0e-3
# (the frames at a row's ends see the tone through a half-empty span: the parabola's vertex moves).  The tolerances are 2 x the worst cases.
F0_TOL_INTERIOR = 4.6e-4
F0_TOL_ALL = 1.2e-2


# ---- the cases tests/test_gpu_pitch.py runs on the device (tests/test_pitch_host.py checks their margins on the CPU) --------------------------
STD = dict(frame_length=1024, hop_length=256, tau_min=36, tau_max=340, threshold=0.1)
GARBAGE = 50.0                           # what lies behind a row's length: loud, so that reading it would show


def parity_rows():
    """(x (4, 8192) float32 with garbage behind each row's length, lengths): a 3-harmonic tone at 110 Hz, a chirp from 100 to 300 Hz, a
    seeded mix of noise, silence and a tone, and silence."""
    L, lens = 8192, [8192, 8000, 5001, 8192]
    x = np.full((4, L), GARBAGE, np.float32)
    x[0] = harmonic_tone(110.0, L)
    x[1, :8000] = chirp(100.0, 300.0, 8000)
    x[2, :5001] = mixed_row(5001, seed=1)
    x[3] = 0.0
    return x, lens


GEOMETRIES = [
    # W, H, tau_min, tau_max, L, f0 of row 0
    (64, 64, 1, 1, 1000, 150.0),                 # the smallest of everything: two lags, one of them beyond tau_max; L no multiple of H
    (4096, 4096, 1, 2048, 8192, 150.0),          # the largest: 88 KiB of LDS, 33 lag chunks
    (1024, 64, 36, 340, 1024, 150.0),            # every frame reaches outside the row
    (1024, 256, 100, 100, 4096, 220.5),          # one lag to search: the period of row 0 is 100 samples
]
