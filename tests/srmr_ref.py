"""The numpy restatement of ev_srmr (include/emojivoice.h), the yardstick of tests/test_gpu_srmr.py, and a plain form of itself.

  * ``srmr``: float64, with the header's structure: chunks of H samples, the carries s[c + 1] = M s[c] + z[c] with M run on unit states, three
    passes, four window-quarter sums per chunk, E[f] = ((p[f, 0] + p[f + 1, 1]) + (p[f + 2, 2] + p[f + 3, 3])), ascending sums, the closing
    rule.  It is vectorised over a row's chunks, so it costs H steps, not len.  numpy has no fma: where the header writes fma(a, b, c) this
    rounds the product first, a difference of float64 rounding size.
  * ``srmr_plain``: the same definition with NO chunks: one sequential run over the row's samples, in longdouble (or any dtype), frames
    summed directly.  tests/test_srmr_host.py holds the two against each other.
  * ``MUTANTS``: wrong readings of the definition, each of which tests/test_gpu_srmr.py must see the device disagree with.
A plain module: no GPU, no fixture.
"""
import numpy as np

from emojivoice_amd import audio

MUTANTS = ("no_carry", "quarter", "share_ge", "kstar_unclamped", "no_gain")
SHARE = 0.9


def tables(sr=1000, n_channels=23, n_bands=8, **kw):
    """``audio.srmr_tables`` at the GPU tests' geometry: sr = 1000 gives H = 64, W = 256 (channels from 125 Hz to below 500 Hz)."""
    return audio.srmr_tables(sr=sr, n_channels=n_channels, n_bands=n_bands, **kw)


def padded(rows, L=None, fill=np.nan):
    """Rows of different lengths as one (B, L) float32 batch with ``fill`` behind every row, and their lengths."""
    lens = [len(r) for r in rows]
    L = max(lens) if L is None else L
    x = np.full((len(rows), L), fill, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, lens


def frames_of(n, L, H):
    """nf of a row of n samples inside a batch of L: 0 for n < 4 H, n < 1 or n > L."""
    n = int(n)
    return (n - 4 * H) // H + 1 if 1 <= n <= L and n >= 4 * H else 0


def voice(n, sr, seed=0, f0=70.0, gate_hz=4.0, noise=0.02, scale=0.3):
    """A harmonic source under a raised-cosine gate at ``gate_hz`` with a little noise: something in every channel and in the low bands."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    h = np.arange(1, int(0.45 * sr / f0) + 1)
    src = (np.sin(2 * np.pi * f0 * h[:, None] * t[None, :] + g.uniform(0, 2 * np.pi, len(h))[:, None]) / h[:, None] ** 0.5).sum(0)
    gate = 0.5 - 0.5 * np.cos(2 * np.pi * gate_hz * t)
    return (scale * (src / np.abs(src).max() * gate + noise * g.standard_normal(n))).astype(np.float32)


# ---- the recurrences, one sample for arrays of any leading shape -------------------------------------------------------------------------------
def _cascade(ar, ai, r, i, xv):
    """One sample of the four stages, in place: r, i (..., N, 4); xv broadcasts against (..., N)."""
    vr, vi = xv, None
    for s in range(4):
        nr = vr + (ar * r[..., s] - ai * i[..., s])
        ni = ar * i[..., s] + ai * r[..., s]
        if vi is not None:
            ni = vi + ni
        r[..., s], i[..., s] = nr, ni
        vr, vi = nr, ni


def _biquad(m, s1, s2, e):
    """One sample of every band in transposed direct form II, in place: s1, s2 (..., N, K); e (..., N) -> the output (..., N, K)."""
    e = e[..., None]
    y = m[:, 0] * e + s1
    s1[...] = (m[:, 1] * e + s2) - m[:, 3] * y
    s2[...] = m[:, 2] * e - m[:, 4] * y
    return y


def transitions(tab, dt=np.float64):
    """The zero-input transitions over H samples, the recurrences run on unit states: Mr, Mi (N, 4, 4) lower triangular (row = stage reached),
    Mb (K, 2, 2)."""
    chan, mod, H = tab["chan"].astype(dt), tab["mod"].astype(dt), tab["hop"]
    N, K = chan.shape[0], mod.shape[0]
    Mr, Mi = np.zeros((N, 4, 4), dt), np.zeros((N, 4, 4), dt)
    for c in range(4):
        r, i = np.zeros((N, 4), dt), np.zeros((N, 4), dt)
        r[:, c] = 1
        for _ in range(H):
            _cascade(chan[:, 0], chan[:, 1], r, i, dt(0))
        Mr[:, :, c], Mi[:, :, c] = r, i
    Mb = np.zeros((K, 2, 2), dt)
    for c in range(2):
        s1, s2 = np.zeros((1, K), dt), np.zeros((1, K), dt)
        (s1 if c == 0 else s2)[...] = 1
        for _ in range(H):
            _biquad(mod, s1, s2, np.zeros(1, dt))
        Mb[:, 0, c], Mb[:, 1, c] = s1[0], s2[0]
    return Mr, Mi, Mb


def _pass(X, tab, r, i, s1, s2, bands, pieces, mutant=None):
    """All chunks of a row at once, H sequential steps: X (nc, H); r, i (nc, N, 4) and s1, s2 (nc, N, K) hold the states at the chunks' starts and
    end as the states at their ends.  -> the four quarter sums (4, nc, N, K) with ``pieces``."""
    chan, mod, win, H = tab["chan"], tab["mod"], tab["window"], tab["hop"]
    gain = np.ones_like(chan[:, 2]) if mutant == "no_gain" else chan[:, 2]
    acc = np.zeros((4,) + s1.shape) if pieces else None
    for t in range(H):
        _cascade(chan[:, 0], chan[:, 1], r, i, X[:, t, None])
        if not bands:
            continue
        e = gain * np.sqrt(r[..., 3] * r[..., 3] + i[..., 3] * i[..., 3])
        y = _biquad(mod, s1, s2, e)
        if pieces:
            for q in range(4):
                wq = (q + 1) % 4 if mutant == "quarter" else q           # (the mutant takes the next quarter of the window)
                v = win[wq * H + t] * y
                acc[q] = acc[q] + v * v
    return acc


def _carry_chan(zr, zi, Mr, Mi):
    """(nc, N, 4) results from zero -> the states at the chunks' starts."""
    sr_, si_ = np.zeros_like(zr), np.zeros_like(zi)
    s_r, s_i = np.zeros_like(zr[0]), np.zeros_like(zi[0])
    for c in range(zr.shape[0]):
        sr_[c], si_[c] = s_r, s_i
        n_r, n_i = zr[c].copy(), zi[c].copy()
        for row in range(4):
            for k in range(row + 1):
                n_r[:, row] = n_r[:, row] + (Mr[:, row, k] * s_r[:, k] - Mi[:, row, k] * s_i[:, k])
                n_i[:, row] = n_i[:, row] + (Mr[:, row, k] * s_i[:, k] + Mi[:, row, k] * s_r[:, k])
        s_r, s_i = n_r, n_i
    return sr_, si_


def _carry_band(z1, z2, Mb):
    o1, o2 = np.zeros_like(z1), np.zeros_like(z2)
    s1, s2 = np.zeros_like(z1[0]), np.zeros_like(z2[0])
    for c in range(z1.shape[0]):
        o1[c], o2[c] = s1, s2
        s1, s2 = (z1[c] + Mb[:, 0, 0] * s1) + Mb[:, 0, 1] * s2, (z2[c] + Mb[:, 1, 0] * s1) + Mb[:, 1, 1] * s2
    return o1, o2


def close_row(mean, tab, mutant=None):
    """The closing rule on Em (N, K) of a row with a frame -> ratio, bw, j90, K*, the cumulative shares."""
    N, K = mean.shape
    ch = np.cumsum(mean, axis=1)[:, -1]                                  # (cumsum adds in ascending order)
    total = np.cumsum(ch)[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        cum = np.cumsum(ch / total)
    over = np.nonzero(cum >= SHARE if mutant == "share_ge" else cum > SHARE)[0]
    j90 = int(over[0]) if over.size else N - 1
    bw = float(tab["erb"][j90])
    below = int(np.count_nonzero(tab["cutoff"] < bw))
    ks = below if mutant == "kstar_unclamped" else min(K, max(min(5, K), below))
    num = np.cumsum(mean[:, :min(4, K)].reshape(-1))[-1]
    hi = mean[:, 4:ks].reshape(-1)
    den = np.cumsum(hi)[-1] if hi.size else 0.0
    ratio = float(num / den) if K > 4 and den > 0 else 0.0
    return ratio, bw, j90, ks, cum


def srmr(x, lens, tab, mutant=None):
    """The restatement on a (B, L) batch -> {"frame" (B, NF, N, K), "mean" (B, N, K), "srmr" (B, 2), "counts" (B, 3) int32, "margin" (B,): the
    least distance of a cumulative share from 0.9 (inf for a row without a frame)}."""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(x)
    B, L = x.shape
    H, N, K = tab["hop"], tab["chan"].shape[0], tab["mod"].shape[0]
    NF = (L - 4 * H) // H + 1 if L >= 4 * H else 0
    Mr, Mi, Mb = transitions(tab)
    out = {"frame": np.zeros((B, NF, N, K)), "mean": np.zeros((B, N, K)), "srmr": np.zeros((B, 2)), "counts": np.zeros((B, 3), np.int32),
           "margin": np.full(B, np.inf)}
    for b in range(B):
        nf = frames_of(L if lens is None else lens[b], L, H)
        if nf == 0:
            continue
        nc = nf + 3
        X = x[b, :nc * H].astype(np.float64).reshape(nc, H)
        zero = lambda *s: np.zeros((nc,) + s)
        zr, zi = zero(N, 4), zero(N, 4)
        _pass(X, tab, zr, zi, None, None, False, False)
        cr, ci = (zero(N, 4), zero(N, 4)) if mutant == "no_carry" else _carry_chan(zr, zi, Mr, Mi)
        z1, z2 = zero(N, K), zero(N, K)
        _pass(X, tab, cr.copy(), ci.copy(), z1, z2, True, False, mutant)
        b1, b2 = (zero(N, K), zero(N, K)) if mutant == "no_carry" else _carry_band(z1, z2, Mb)
        p = _pass(X, tab, cr.copy(), ci.copy(), b1, b2, True, True, mutant)
        E = (p[0, 0:nf] + p[1, 1:nf + 1]) + (p[2, 2:nf + 2] + p[3, 3:nf + 3])
        mean = np.cumsum(E, axis=0)[-1] / float(nf)
        ratio, bw, j90, ks, cum = close_row(mean, tab, mutant)
        out["frame"][b, :nf], out["mean"][b], out["srmr"][b], out["counts"][b] = E, mean, (ratio, bw), (nf, j90, ks)
        out["margin"][b] = float(np.min(np.abs(cum - SHARE))) if np.all(np.isfinite(cum)) else np.inf
    return out


def srmr_plain(x, lens, tab, dt=np.longdouble):
    """The definition with no chunks: one run over the samples in ``dt``; frames summed directly.  Same keys as ``srmr`` (float outputs in ``dt``)."""
    x = np.asarray(x)
    B, L = x.shape
    H, N, K = tab["hop"], tab["chan"].shape[0], tab["mod"].shape[0]
    W = 4 * H
    NF = (L - W) // H + 1 if L >= W else 0
    chan, mod, win = tab["chan"].astype(dt), tab["mod"].astype(dt), tab["window"].astype(dt)
    out = {"frame": np.zeros((B, NF, N, K), dt), "mean": np.zeros((B, N, K), dt), "srmr": np.zeros((B, 2), dt), "counts": np.zeros((B, 3), np.int32)}
    for b in range(B):
        nf = frames_of(L if lens is None else lens[b], L, H)
        if nf == 0:
            continue
        n = (nf + 3) * H
        xs = x[b, :n].astype(dt)
        r, i, s1, s2 = np.zeros((N, 4), dt), np.zeros((N, 4), dt), np.zeros((N, K), dt), np.zeros((N, K), dt)
        m = np.zeros((n, N, K), dt)
        for t in range(n):
            _cascade(chan[:, 0], chan[:, 1], r, i, xs[t])
            e = chan[:, 2] * np.sqrt(r[:, 3] * r[:, 3] + i[:, 3] * i[:, 3])
            m[t] = _biquad(mod, s1, s2, e)
        E = np.stack([((win[:, None, None] * m[f * H: f * H + W]) ** 2).sum(0) for f in range(nf)])
        mean = E.sum(0) / dt(nf)
        ratio, bw, j90, ks, _ = close_row(mean, tab)
        out["frame"][b, :nf], out["mean"][b], out["srmr"][b], out["counts"][b] = E, mean, (ratio, bw), (nf, j90, ks)
    return out


def rel_err(dev, ref):
    """test_gpu_loudness.py's rule per row: max |dev - ref| / max(|ref|, 1e-9 x the row's largest |ref|); a reference row of zeros must be a row
    of zeros."""
    worst = 0.0
    B = np.asarray(ref).shape[0]
    for d, r in zip(np.asarray(dev).reshape(B, -1), np.asarray(ref).reshape(B, -1)):
        top = float(np.max(np.abs(r))) if r.size else 0.0
        if top == 0.0:
            assert not np.asarray(d).any(), "a row of zeros in the reference is a row of zeros"
            continue
        worst = max(worst, float(np.max(np.abs(d - r) / np.maximum(np.abs(r), 1e-9 * top))))
    return worst


# ---- the GPU cases: shared by tests/test_gpu_srmr.py (device against the restatement) and tests/test_srmr_host.py (restatement against its
# longdouble form: the figure the GPU gate max(1e-9, 16 x it) hangs on) ---------------------------------------------------------------------------
H0 = 64
LENGTHS = (4 * H0 - 1, 4 * H0, 4 * H0 + 1, 5 * H0 - 1, 5 * H0, 5 * H0 + 7, 40 * H0 + 3)
SHAPES = ((3, 3, 8), (1, 1, 1), (2, 23, 8), (1, 32, 5))                  # (B, N, K)


def case(name):
    """-> (x (B, L) float32 with NaN behind every row, lens, tab).  Names: "shape-B-N-K", "lengths", "big"."""
    if name == "lengths":                                                # every length, then len 0 and len > L, inside one batch
        tab = tables(n_channels=23, n_bands=8)
        rows = [voice(n, 1000, seed=n) for n in LENGTHS]
        x, lens = padded(rows + [voice(300, 1000, seed=1), voice(300, 1000, seed=2)], L=LENGTHS[-1] + 5)
        lens[-2], lens[-1] = 0, x.shape[1] + 1
        return x, lens, tab
    if name == "big":                                                    # H = 1024 at 16 kHz, 23 x 8, B = 2, 1.6 s
        tab = audio.srmr_tables()
        return (*padded([voice(25600, 16000, seed=5, f0=110.0), voice(25600 - 700, 16000, seed=6, f0=180.0)], L=25600 + 3), tab)
    _, B, N, K = name.split("-")
    B, N, K = int(B), int(N), int(K)
    tab = tables(n_channels=N, n_bands=K)
    rows = [voice(40 * H0 + 3 - 97 * b, 1000, seed=10 * N + b, f0=70.0 + 13.0 * b) for b in range(B)]
    return (*padded(rows, L=40 * H0 + 9), tab)


def tie_case():
    """Hand-made tables on which every step is EXACT in float64, fma or not, and the cumulative share after channel 2 is the double 0.9 itself:
    four channels with a = 0 (the cascade hands the sample through) and gains 1, 2, 2, 1, one band that hands the envelope through, a window
    of ones, a row of ones.  Em = W {1, 4, 4, 1}, the shares are fl(0.1), fl(0.4), fl(0.4), fl(0.1), fl(0.1) + fl(0.4) = 0.5 and
    0.5 + fl(0.4) = fl(0.9) exactly.  'Exceeds' must then pass channel 2 by: j90 = 3.  -> (x, lens, tab)."""
    tab = {"sr": 1000, "hop": H0, "chan": np.array([[0.0, 0.0, g] for g in (1.0, 2.0, 2.0, 1.0)]), "mod": np.array([[1.0, 0.0, 0.0, 0.0, 0.0]]),
           "window": np.ones(4 * H0), "erb": np.array([10.0, 20.0, 30.0, 40.0]), "cutoff": np.array([5.0])}
    return np.ones((1, 6 * H0), np.float32), None, tab


def kstar_case():
    """Modulation bands from 30 Hz under a low tone: the 90 % channel is one of the lowest, fewer than five lower band edges lie under its
    bandwidth, and the clamp max(min(5, K), .) of K* decides the denominator.  -> (x, lens, tab)."""
    tab = tables(n_channels=23, n_bands=8, mod_lo=30.0, mod_hi=200.0)
    n = 40 * H0 + 3
    t = np.arange(n) / 1000.0
    g = np.random.default_rng(11)
    x = 0.3 * np.sin(2 * np.pi * 126.0 * t) * (0.5 - 0.5 * np.cos(2 * np.pi * 37.0 * t)) + 0.002 * g.standard_normal(n)
    return (*padded([x.astype(np.float32)], L=n + 4), tab)


CASES = tuple(f"shape-{B}-{N}-{K}" for B, N, K in SHAPES) + ("lengths", "big")

FLOAT_OUTPUTS = ("frame", "mean", "srmr")
_HOST = {}


def host_error(name):
    """The restatement against its longdouble plain form on a GPU case, by ``rel_err``, worst of the float outputs; computed once per case."""
    if name not in _HOST:
        x, lens, tab = case(name)
        a, b = srmr(x, lens, tab), srmr_plain(x, lens, tab)
        assert np.array_equal(a["counts"], b["counts"]), name
        _HOST[name] = max(rel_err(a[k], b[k].astype(np.float64)) for k in FLOAT_OUTPUTS)
    return _HOST[name]


def gpu_gate(name):
    """The gate of the device against the restatement on a case: the project's 1e-9, or 16 x ``host_error`` where that is more (the band
    filters' poles sit within 4e-4 of the unit circle at 4 Hz and 16 kHz; the device and the restatement each stand one reordering away from
    the exact value)."""
    return max(1e-9, 16.0 * host_error(name))
