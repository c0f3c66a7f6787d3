"""numpy / scipy float64 restatement of ev_loudness' semantics (include/emojivoice.h): ITU-R BS.1770-4 gated loudness of
mono rows.  For a row x of len samples, S samples per 100 ms, coef = {b0, b1, b2, a1, a2} of the shelf then of the high pass:
    y           scipy.signal.lfilter per stage over the WHOLE row, float64, zero initial state
    e[i]        sum of y^2 over [i S, (i + 1) S) for i < ns = len // S; the incomplete tail is discarded
    z[j]        ((e[j] + e[j+1]) + (e[j+2] + e[j+3])) / (4 S) for j < nb = max(ns - 3, 0)
    gates       absolute z > abs_gate; m_abs = mean of those z; relative, additionally, z > 0.1 m_abs (strict, power domain)
    gated       {mean of z over the blocks passing both, m_abs}, 0 where the set is empty;  counts {nb, n_abs, n_both}
Rows with len < 1 or len > L are zeros.  Outputs are padded with zeros to NS = L // S and NB = max(NS - 3, 0).

Every row also gets its GATE MARGIN in dB: the smallest |10 log10(z[j] / threshold)| over ALL its blocks and both thresholds (the relative one
exists once a block has passed the absolute one); inf for a row without blocks.  An implementation that filters or sums in another order may
differ from this file in the counts only on rows whose margin is of the order of its rounding error.

The file also holds the rows the loudness tests share.  The device cases pass the 22.05 kHz coefficients together with a SMALL S: the kernel
does not tie the two, and small cases need that (no filter is designed for a tiny rate: below ~3.4 kHz the shelf's f0 is beyond Nyquist).
"""
import numpy as np
from scipy.signal import lfilter

import pitch_ref as P

OFFSET = -0.691
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
GARBAGE = 50.0                           # what lies behind a row's length: loud, so that reading it would show
CHUNK = 1024                             # LOUD_CHUNK of ev_analysis_kernels.h: the edge cases sit around it

# the BS.1770-4 table: the two biquads at 48 kHz, in ev_loudness' layout
TABLE_48K = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                      1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])


def lufs(ms):
    ms = np.asarray(ms, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(ms > 0, OFFSET + 10.0 * np.log10(np.where(ms > 0, ms, 1.0)), -np.inf)


def k_filter(x, coef):
    """The K-weighted signal of one row: lfilter per stage over the whole row."""
    c = np.asarray(coef, dtype=np.float64)
    y = lfilter(c[0:3], [1.0, c[3], c[4]], np.asarray(x, dtype=np.float64))
    return lfilter(c[5:8], [1.0, c[8], c[9]], y)


def row_loudness(x, S, coef, abs_gate=ABS_GATE):
    """(e (ns,), z (nb,), gated (2,), counts (3,), margin dB) of one row's valid samples."""
    S = int(S)
    ns = len(x) // S
    nb = max(ns - 3, 0)
    y = k_filter(x, coef)
    e = np.array([np.sum(y[i * S:(i + 1) * S] ** 2) for i in range(ns)], dtype=np.float64)
    z = np.array([((e[j] + e[j + 1]) + (e[j + 2] + e[j + 3])) / (4 * S) for j in range(nb)], dtype=np.float64)
    p = z > abs_gate
    m_abs = float(z[p].mean()) if p.any() else 0.0
    q = p & (z > 0.1 * m_abs)
    both = float(z[q].mean()) if q.any() else 0.0
    margin = np.inf
    with np.errstate(divide="ignore"):
        if nb:
            margin = float(np.min(np.abs(10.0 * np.log10(z / abs_gate))))
            if p.any():
                margin = min(margin, float(np.min(np.abs(10.0 * np.log10(z / (0.1 * m_abs))))))
    return e, z, np.array([both, m_abs]), np.array([nb, int(p.sum()), int(q.sum())], dtype=np.int32), margin


def loudness(x, lengths, S, coef, abs_gate=ABS_GATE):
    """x (B, L) or (L,) -> {"sub" (B, NS), "block" (B, NB), "gated" (B, 2) float64, "counts" (B, 3) int32, "margin" (B,) dB, "integrated" (B,)
    LUFS}."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    B, L = x.shape
    NS = L // int(S)
    NB = max(NS - 3, 0)
    lens = [L] * B if lengths is None else [int(v) for v in lengths]
    out = {"sub": np.zeros((B, NS)), "block": np.zeros((B, NB)), "gated": np.zeros((B, 2)), "counts": np.zeros((B, 3), np.int32),
           "margin": np.full(B, np.inf)}
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        e, z, g, c, m = row_loudness(x[b, :n], S, coef, abs_gate)
        out["sub"][b, :len(e)], out["block"][b, :len(z)], out["gated"][b], out["counts"][b], out["margin"][b] = e, z, g, c, m
    out["integrated"] = lufs(out["gated"][:, 0])
    return out


def block_formula(sub, counts, S):
    """The header's block formula applied to GIVEN sub-block energies (B, NS) with counts[:, 0] blocks per row: (B, max(NS - 3, 0)), the same
    association and one division by 4 S.  What d_block must equal bit for bit on the device's own d_sub."""
    sub = np.asarray(sub, dtype=np.float64)
    B, NS = sub.shape
    out = np.zeros((B, max(NS - 3, 0)))
    for b in range(B):
        for j in range(int(counts[b][0])):
            out[b, j] = ((sub[b, j] + sub[b, j + 1]) + (sub[b, j + 2] + sub[b, j + 3])) / (4 * int(S))
    return out


# ---- the rows the tests share ---------------------------------------------------------------------------------------------------------------
def sine(freq, seconds, sr, amplitude=1.0):
    return (amplitude * np.sin(2 * np.pi * freq * np.arange(int(seconds * sr)) / sr)).astype(np.float32)


def padded(rows, L=None, tail=0):
    """(x (B, L) float32 with GARBAGE behind every row, lengths): L = the longest row + tail unless given."""
    lens = [len(r) for r in rows]
    L = max(lens) + tail if L is None else L
    x = np.full((len(rows), L), GARBAGE, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, lens


GATING_S = (64, 100, 250, 2205)
# what the restatement gives for gating_row(S) (tests/test_loudness_host.py asserts it on the CPU): counts, and integrated LUFS to 0.01
GATING_COUNTS = {64: (37, 31, 20), 100: (37, 31, 20), 250: (37, 31, 20), 2205: (37, 30, 20)}
GATING_LUFS = {64: -18.07, 100: -17.84, 250: -17.89, 2205: -17.82}


def gating_row(S):
    """Seed 1770: four segments of 10 S + 7 Gaussian samples at sigma 0.1, 0.1 * 10^(-30/20), 1e-5 and 0.1.  The middle segments exercise both
    gates, the filter's tail into near-silence, and energies 7e-9 of the row's maximum."""
    g = np.random.default_rng(1770)
    n = 10 * int(S) + 7
    return np.concatenate([s * g.standard_normal(n) for s in (0.1, 0.1 * 10 ** (-30 / 20), 1e-5, 0.1)]).astype(np.float32)


EDGE_S = 64
EDGE_LENS = [4 * EDGE_S - 1, 4 * EDGE_S, 4 * EDGE_S + 1, 5 * EDGE_S - 1, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + EDGE_S]


def edge_rows():
    """(x (11, 2171) with garbage, lengths): Gaussian rows (sigma 0.1, seed 64 + row) of the edge lengths at S = 64 — no block, exactly one, one
    and a sample, one and almost a sub-block, a single sample, one chunk of the device's filter minus / plus one sample, two chunks and a
    sub-block — then a row longer than L and an empty one, which must come out as zeros.  L = 2171 is odd: the rows of the batch start at
    every alignment."""
    rows = [(0.1 * np.random.default_rng(64 + i).standard_normal(n)).astype(np.float32) for i, n in enumerate(EDGE_LENS)]
    x, lens = padded(rows, L=2 * CHUNK + EDGE_S + 59)
    x = np.concatenate([x, np.full((2, x.shape[1]), GARBAGE, np.float32)])
    return x, lens + [x.shape[1] + 1, 0]


def realistic_rows(sr=22050):
    """(x (3, 3 sr) with garbage, lengths) of 1.0, 2.3 and 3.0 s: a 3-harmonic tone at 140 Hz under noise; the pitch tests' noise / silence /
    tone row; a louder tone at 220 Hz with a quiet second half."""
    g = np.random.default_rng(22050)
    n = [int(1.0 * sr), int(2.3 * sr), int(3.0 * sr)]
    a = P.harmonic_tone(140.0, n[0], sr) + (0.01 * g.standard_normal(n[0])).astype(np.float32)
    b = P.mixed_row(n[1], seed=7, sr=sr)
    c = P.harmonic_tone(220.0, n[2], sr, scale=0.5)
    c[n[2] // 2:] *= 0.05
    c = c + (0.002 * g.standard_normal(n[2])).astype(np.float32)
    return padded([a, b, c.astype(np.float32)])
