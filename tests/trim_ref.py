"""numpy float64 restatement of the trimming semantics (include/emojivoice.h): librosa.effects.trim's frames and
bounds, and the peak gain of hifigan/meldataset.py:152.  librosa is not a dependency: the formula below IS the yardstick.

For a row x of len samples, frame_length F, hop_length H, top_db:
    n_frames = 1 + len // H;  frame f covers samples [f H - F/2, f H + F/2), zeros outside [0, len)      (center=True, constant padding)
    ms[f] = (1 / F) sum x^2
    f is non-silent  iff  max(ms[f], 1e-10) > max(max_f ms, 1e-10) * 10^(-top_db / 10)
    start = f_first H,  end = min(len, (f_last + 1) H);  no non-silent frame (top_db <= 0): (0, 0)
    peak = max |x| over the whole row
"""
import numpy as np


def frame_ms(x, frame_length=2048, hop_length=512, centred=True):
    """ms[f] for f < 1 + len // H.  ``centred=False`` is the MUTANT frame [f H, f H + F) (the tests hand it out as a wrong expectation)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    F, H = int(frame_length), int(hop_length)
    n_frames = 1 + len(x) // H
    left = F // 2 if centred else 0
    xp = np.concatenate([np.zeros(left), x, np.zeros(n_frames * H + F)])
    return np.array([np.sum(xp[f * H: f * H + F] ** 2) / F for f in range(n_frames)])


def non_silent(ms, top_db=60.0):
    ref = max(float(np.max(ms)), 1e-10)
    return np.maximum(ms, 1e-10) > ref * 10.0 ** (-float(top_db) / 10.0)


def margin_db(ms, top_db=60.0):
    """Least distance in dB of a frame's max(ms, 1e-10) from the threshold."""
    ref = max(float(np.max(ms)), 1e-10)
    return float(np.min(np.abs(10.0 * np.log10(np.maximum(ms, 1e-10) / ref) + float(top_db))))


def bounds(x, top_db=60.0, frame_length=2048, hop_length=512, centred=True, clip_end=True):
    """(start, end).  ``clip_end=False`` is the second MUTANT: end = (f_last + 1) H even past len."""
    n = len(np.asarray(x).reshape(-1))
    keep = np.flatnonzero(non_silent(frame_ms(x, frame_length, hop_length, centred), top_db))
    if keep.size == 0:
        return 0, 0
    end = (int(keep[-1]) + 1) * int(hop_length)
    return int(keep[0]) * int(hop_length), (min(n, end) if clip_end else end)


def peak(x):
    x = np.asarray(x).reshape(-1)
    return float(np.max(np.abs(x))) if x.size else 0.0


def apply(x, start, end, peak_value=None, target_peak=0.0, out_len=None):
    """(y float32 (out_len,), n): x[start:end] times the fp32 gain target / peak (1 without a peak, for target <= 0 or peak <= 0), one fp32
    multiply per sample, zeros right of n = min(end - start, out_len)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    g = np.float32(1.0)
    if peak_value is not None and target_peak > 0 and peak_value > 0:
        g = np.float32(target_peak) / np.float32(peak_value)
    L_out = len(x) if out_len is None else int(out_len)
    n = min(end - start, L_out) if 0 <= start <= end <= len(x) else 0
    y = np.zeros(L_out, dtype=np.float32)
    y[:n] = x[start:start + n] * g
    return y, n


LEVELS_DB = (-80.0, -50.0, 0.0, -50.0, -80.0)


def three_level_row(n, seed, burst_rms=0.25):
    """(float32 row of n samples, the five segment lengths): Gaussian noise at -80 dB, a segment at -50 dB, a burst at 0 dB (rms
    ``burst_rms``), then the mirror image.  With top_db = 60 the -50 dB parts lie 10 dB above the threshold and the -80 dB parts 20 dB
    below it.  From 4096 samples on, the two -80 / -50 boundaries sit on multiples of 512 samples, so that a frame of 4 hops holds
    0, 1/4, 2/4 ... of -50 dB material (a frame of 1 hop: 0 or 1/2) and never the ~1/10 that would put it AT the threshold; shorter rows
    are cut in the proportions 0.3 / 0.15 / 0.1 / 0.15 / 0.3 and every frame holds burst samples.  Rows under 5 samples are burst only."""
    g = np.random.default_rng(seed)
    if n < 5:
        lens = [0, 0, n, 0, 0]
    elif n < 4096:
        cuts = [int(round(n * c)) for c in (0.3, 0.45, 0.55, 0.7)] + [n]
        lens = np.diff([0] + cuts).tolist()
    else:
        k = n // 512
        c1, c4 = 512 * (k // 4), 512 * (k - k // 4)
        third = (c4 - c1) // 3
        lens = [c1, third, c4 - c1 - 2 * third, third, n - c4]
    parts = [g.standard_normal(m) * (burst_rms * 10.0 ** (db / 20.0)) for m, db in zip(lens, LEVELS_DB)]
    return np.concatenate(parts).astype(np.float32), lens
