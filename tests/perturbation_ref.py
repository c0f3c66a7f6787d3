"""numpy restatement of ev_perturbation (include/emojivoice.h): jitter, shimmer and the harmonic strength per frame, from
peak-picked pitch marks around the frame's centre and the normalised cross-correlation at the frame's YIN lag.  It runs in float64 and, with
``dtype=np.longdouble``, in extended precision; both take the samples as the fp32 numbers they are.

For a row x of len samples (+0 outside [0, len)), H the hop, frame f, c = f H + H // 2, tau0 = lag[f]:
    unvoiced    tau0 < 16 or tau0 > 2048: zeros in frame and count, -1 in every mark
    marks       q = tau0 // 8, lo = tau0 - q, hi = tau0 + q;  m_0 = argmax x over [s, s + tau0), s = c - tau0 // 2;  m_{k+1} = argmax over
                [m_k + lo, m_k + hi];  m_{k-1} = argmax over [m_k - hi, m_k - lo];  k to n_cycles on each side; ties to the LOWEST index; a mark
                is accepted when x[m] > 0, x[m] > x[m - 1] and x[m] >= x[m + 1]; the first one that is not ends its direction (the anchor: all)
    refinement  a, b, c = x[m - 1], x[m], x[m + 1];  den = (a - 2 b) + c;  shift = 0.5 (a - c) / den when den < 0 and |shift| <= 1, else 0;
                t = m + shift;  A = b - 0.25 (a - c) shift
    periods     T_i = t_{i+1} - t_i;  a period pair counts when max <= period_factor min, an amplitude pair when max <= amplitude_factor min, a
                triple when both of its period pairs count;  every sum is one chain in ascending i
    frame       0 mean|T_i - T_{i+1}| / Tmean   1 mean|T_i - T_{i+1}|   2 mean|A_i - A_{i+1}| / Amean   3 mean|20 log10(A_{i+1} / A_i)|
                4 r   5 Tmean   6 Amean   7 mean|T_i - (T_{i-1} + T_i + T_{i+1}) / 3| / Tmean;  a mean over no terms is 0
    count       the periods, the counted period pairs, the counted amplitude pairs, the counted triples
    r           W = corr_length, s = c - (W + tau0) // 2;  for tau in tau0 - 1, tau0, tau0 + 1:  C = sum_j x[s + j] x[s + j + tau],  E1 = sum_j
                x[s + j + tau]^2,  E0 = sum_j x[s + j]^2  (j < W; lane l = j mod 64 adds its terms in ascending j, then an xor tree over the 64
                lanes with offsets 32 .. 1: ``lane_sum``);  r(tau) = C / sqrt(E0 E1) when E0 E1 > power_floor^2, else 0;  with a, b, c = the
                three r:  r = b - 0.25 (a - c) shift under the shift rule above
Frames at or past ceil(len / H), and rows with len < 1 or len > L, are zeros with -1 in the marks.

Besides the outputs every frame reports what the comparison on the device needs to know about the INPUT: the parabola branch of every mark and
of r, the least relative distance of a counted or excluded pair from its factor threshold, the least |E0 E1 - floor^2| / floor^2, and the
number of searches whose maximum occurs more than once (ties).
"""
from collections import namedtuple

import numpy as np

import pitch_ref

TAU_LO, TAU_HI = 16, 2048
TOL = 1e-9                               # the project's float64 margin: |device - restatement| <= TOL max(|restatement|, 1)
PAIR_MARGIN = 1e-6                       # input condition: every pair keeps this relative distance from its factor threshold
FLOOR_MARGIN = 1e-6                      # input condition: |E0 E1 - floor^2| >= FLOOR_MARGIN floor^2
GARBAGE = 50.0                           # what lies behind a row's length
MUTANTS = ("window_quarter", "no_refinement", "ties_highest", "no_period_factor", "anchor_from_frame_start", "unnormalised_hnr",
           "no_local_peak_rule")

Geo = namedtuple("Geo", "H W nc pf af floor")


def geo(H=64, W=128, nc=3, pf=1.3, af=1.6, floor=1e-10):
    return Geo(int(H), int(W), int(nc), float(pf), float(af), float(floor))


def frames(n, H):
    return -(-int(n) // int(H))


def err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0))) if got.size else 0.0


def lane_sum(v, dtype):
    """The device's order over W terms: lane l adds the terms j = l, l + 64, ... in ascending j, then an xor tree (offsets 32 .. 1)."""
    W = len(v)
    R = -(-W // 64)
    buf = np.zeros(R * 64, dtype=dtype)
    buf[:W] = v
    acc = np.zeros(64, dtype=dtype)
    for r in range(R):
        acc = acc + buf[r * 64: (r + 1) * 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return acc[0]


def parabola(a, b, c, dtype, refine=True):
    """(shift, vertex value, branch taken) of the parabola through (-1, a), (0, b), (1, c)."""
    a, b, c = dtype(a), dtype(b), dtype(c)
    den = (a - dtype(2) * b) + c
    shift, taken = dtype(0), False
    if refine and den < 0:
        s = dtype(0.5) * (a - c) / den
        if abs(s) <= 1:
            shift, taken = s, True
    return shift, b - dtype(0.25) * (a - c) * shift, taken


def _chain(terms, dtype):
    s = dtype(0)
    for v in terms:
        s = s + v
    return s


def frame(xp, pad, f, tau0, g, dtype=np.float64, mutant=None):
    """One frame of a row whose samples sit in ``xp`` (float32) behind ``pad`` zeros (and before as many).  -> (frame (8,), count (4,), marks
    (2 nc + 1,), branch (2 nc + 2,) int: 1 / 0 the parabola branch of each mark and, last, of r; -1 no mark), pair margin, floor margin, ties)."""
    nc = g.nc
    out, count = np.zeros(8, dtype=dtype), np.zeros(4, np.int32)
    marks, branch = np.full(2 * nc + 1, -1, np.int64), np.full(2 * nc + 2, -1, np.int64)
    info = [np.inf, np.inf, 0]
    tau0 = int(tau0)
    if tau0 < TAU_LO or tau0 > TAU_HI:
        return out, count, marks, branch, info
    X = lambda i: xp[pad + i]
    c = f * g.H + g.H // 2
    q = tau0 // (4 if mutant == "window_quarter" else 8)
    lo, hi = tau0 - q, tau0 + q

    def search(a, b):                                                    # argmax over [a, b]
        v = xp[pad + a: pad + b + 1]
        m = len(v) - 1 - int(np.argmax(v[::-1])) if mutant == "ties_highest" else int(np.argmax(v))
        if v[m] > 0 and int((v == v[m]).sum()) > 1:
            info[2] += 1
        return a + m

    def accepted(m):
        if mutant == "no_local_peak_rule":
            return X(m) > 0
        return X(m) > 0 and X(m) > X(m - 1) and X(m) >= X(m + 1)

    s = f * g.H if mutant == "anchor_from_frame_start" else c - tau0 // 2
    m0 = search(s, s + tau0 - 1)
    if accepted(m0):
        marks[nc] = m0
        m = m0
        for k in range(1, nc + 1):
            m = search(m + lo, m + hi)
            if not accepted(m):
                break
            marks[nc + k] = m
        m = m0
        for k in range(1, nc + 1):
            m = search(m - hi, m - lo)
            if not accepted(m):
                break
            marks[nc - k] = m
    ts, As = [], []
    for slot in range(2 * nc + 1):
        m = int(marks[slot])
        if m < 0:
            continue
        shift, A, taken = parabola(X(m - 1), X(m), X(m + 1), dtype, refine=mutant != "no_refinement")
        branch[slot] = int(taken)
        ts.append(dtype(m) + shift)
        As.append(A)
    N = len(ts)
    T = [ts[i + 1] - ts[i] for i in range(N - 1)]
    nT = len(T)
    pf, af = dtype(g.pf), dtype(g.af)

    def counts(u, v, factor):
        mx, mn = max(u, v), min(u, v)
        thr = factor * mn
        if thr != 0:
            info[0] = min(info[0], float(abs(mx - thr) / abs(thr)))
        return bool(mx <= thr)

    pp = [mutant == "no_period_factor" or counts(T[i], T[i + 1], pf) for i in range(nT - 1)]
    ap = [counts(As[i], As[i + 1], af) for i in range(N - 1)]
    tr = [pp[i - 1] and pp[i] for i in range(1, nT - 1)]                 # the triple centred on period i = 1 .. nT - 2
    Tmean = _chain(T, dtype) / dtype(nT) if nT else dtype(0)
    Amean = _chain(As, dtype) / dtype(N) if N else dtype(0)
    npp, nap, ntr = sum(pp), sum(ap), sum(tr)
    if npp:
        out[1] = _chain([abs(T[i] - T[i + 1]) for i in range(nT - 1) if pp[i]], dtype) / dtype(npp)
        out[0] = out[1] / Tmean
    if nap:
        out[2] = _chain([abs(As[i] - As[i + 1]) for i in range(N - 1) if ap[i]], dtype) / dtype(nap) / Amean
        out[3] = _chain([abs(dtype(20) * np.log10(As[i + 1] / As[i])) for i in range(N - 1) if ap[i]], dtype) / dtype(nap)
    if ntr:
        out[7] = _chain([abs(T[i] - ((T[i - 1] + T[i]) + T[i + 1]) / dtype(3)) for i in range(1, nT - 1) if tr[i - 1]], dtype) / dtype(ntr) / Tmean
    out[5], out[6] = Tmean, Amean
    count[:] = (nT, npp, nap, ntr)
    # the harmonic strength
    W = g.W
    s = c - (W + tau0) // 2
    base = xp[pad + s: pad + s + W].astype(dtype)
    e0 = lane_sum(base * base, dtype)
    r = []
    floor2 = dtype(g.floor) * dtype(g.floor)
    for tau in (tau0 - 1, tau0, tau0 + 1):
        sh = xp[pad + s + tau: pad + s + tau + W].astype(dtype)
        cc, e1 = lane_sum(base * sh, dtype), lane_sum(sh * sh, dtype)
        info[1] = min(info[1], float(abs(e0 * e1 - floor2) / floor2))
        if mutant == "unnormalised_hnr":
            r.append(cc / e0 if e0 * e1 > floor2 else dtype(0))
        else:
            r.append(cc / np.sqrt(e0 * e1) if e0 * e1 > floor2 else dtype(0))
    _, out[4], taken = parabola(r[0], r[1], r[2], dtype, refine=mutant != "no_refinement")
    branch[2 * nc + 1] = int(taken)
    return out, count, marks, branch, info


def batch(x, lens, lag, g, dtype=np.float64, mutant=None):
    """x (B, L) float32, lens (B,) or None, lag (B, F) integers, F = ceil(L / H) -> {"frame" (B, F, 8) in ``dtype``, "count" (B, F, 4) int32,
    "marks" (B, F, 2 nc + 1) int32, "branch" (B, F, 2 nc + 2), "pair_margin", "floor_margin" (floats: the least over all frames), "ties"}."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    B, L = x.shape
    F = frames(L, g.H)
    lag = np.asarray(lag).reshape(B, F)
    lens = [L] * B if lens is None else [int(v) for v in lens]
    nm = 2 * g.nc + 1
    out = {"frame": np.zeros((B, F, 8), dtype=dtype), "count": np.zeros((B, F, 4), np.int32), "marks": np.full((B, F, nm), -1, np.int32),
           "branch": np.full((B, F, nm + 1), -1, np.int64), "pair_margin": np.inf, "floor_margin": np.inf, "ties": 0}
    pad = (g.nc + 2) * (TAU_HI + TAU_HI // 4) + g.W + 8
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        xp = np.zeros(n + 2 * pad, np.float32)
        xp[pad: pad + n] = x[b, :n]
        for f in range(frames(n, g.H)):
            fr, ct, mk, br, info = frame(xp, pad, f, lag[b, f], g, dtype, mutant)
            out["frame"][b, f], out["count"][b, f], out["marks"][b, f], out["branch"][b, f] = fr, ct, mk, br
            out["pair_margin"] = min(out["pair_margin"], info[0])
            out["floor_margin"] = min(out["floor_margin"], info[1])
            out["ties"] += info[2]
    return out


def input_conditions(r64, rld, what):
    """The conditions on the INPUT that come before any comparison with the device; they hold for every frame or the case is no case."""
    for k in ("marks", "count", "branch"):
        assert np.array_equal(r64[k], rld[k]), f"{what}: the float64 and longdouble restatements disagree on {k}"
    for r in (r64, rld):
        assert r["pair_margin"] >= PAIR_MARGIN, f"{what}: a pair {r['pair_margin']:.3e} from its factor threshold, under {PAIR_MARGIN:g}"
        assert r["floor_margin"] >= FLOOR_MARGIN, f"{what}: E0 E1 {r['floor_margin']:.3e} floor^2 from the floor, under {FLOOR_MARGIN:g}"


def hnr_db(r):
    r = np.clip(np.asarray(r, dtype=np.float64), 1e-6, 1.0 - 1e-9)
    return 10.0 * np.log10(r / (1.0 - r))


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def pulse(t, sr=22050):
    """One glottal pulse through two resonances, a continuous-time function of t >= 0 in samples at ``sr`` (the constants are those of 22050 Hz,
    scaled with sr: 700 and 1200 Hz, decays of 60 and 40 samples at 22050 Hz, an attack of 6)."""
    u = np.asarray(t, dtype=np.float64) * (22050.0 / sr)
    return (1.0 - np.exp(-u / 6.0)) ** 2 * (np.exp(-u / 60.0) * np.sin(2.0 * np.pi * 700.0 * u / 22050.0 + 1.0)
                                          + 0.5 * np.exp(-u / 40.0) * np.sin(2.0 * np.pi * 1200.0 * u / 22050.0))


def perturbed_pulses(n, f0, jitter=0.0, shimmer=0.0, seed=0, sr=22050, noise=0.0):
    """n samples of pulses at f0 Hz: the onset times advance by T0 (1 + jitter N(0, 1)) (fractional, the pulse is evaluated at n - t_k), the
    amplitudes are 1 + shimmer N(0, 1); ``noise`` adds white Gaussian noise of that deviation.  float32, peak about 0.5."""
    g = np.random.default_rng(seed)
    T0 = sr / float(f0)
    onsets, t = [], 0.37 * T0
    while t < n:
        onsets.append(t)
        t += T0 * (1.0 + jitter * g.standard_normal())
    onsets = np.array(onsets)
    amps = 1.0 + shimmer * g.standard_normal(len(onsets))
    d = np.arange(n, dtype=np.float64)[:, None] - onsets[None, :]
    y = (np.where(d > 0, pulse(np.maximum(d, 0.0), sr), 0.0) * amps[None, :]).sum(axis=1)
    if noise:
        y = y + noise * g.standard_normal(n)
    return (0.5 * y).astype(np.float32)


def padded(rows, L=None):
    """rows (float32 arrays) -> (x (B, L) with GARBAGE behind each row, lens)."""
    lens = [len(r) for r in rows]
    L = max(lens) if L is None else L
    x = np.full((len(rows), L), GARBAGE, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, lens


def yin_lags(x, lens, g, tau_min=16, tau_max=100, frame_length=None):
    return pitch_ref.pitch_yin(x, lens, frame_length=g.W if frame_length is None else frame_length, hop_length=g.H, tau_min=tau_min, tau_max=tau_max,
                               threshold=0.1)["lag"]


# ---- the cases tests/test_gpu_perturbation.py runs on the device (tests/test_perturbation_host.py checks their input conditions on the CPU) ----
SR_SMALL = 4000
SMALL_LENS = [2490, 2560, 2600]          # 39, 40 and 41 frames at H = 64: 3, 0 and 1 past a workgroup's four


def small_rows(seed=0):
    spec = ((100.0, 0.01, 0.05), (125.0, 0.01, 0.0), (80.0, 0.0, 0.1))
    return padded([perturbed_pulses(n, f0, j, s, seed=seed + 7 * i, sr=SR_SMALL, noise=1e-3) for i, (n, (f0, j, s)) in enumerate(zip(SMALL_LENS, spec))])


def plateau_rows():
    """Samples quantised to 1 / 64: equal maxima occur inside a search's range and the tie rule decides."""
    rows = [np.round(pitch_ref.harmonic_tone(f0, n, sr=SR_SMALL, scale=0.4) * 64.0) / 64.0 for f0, n in ((100.0, 2490), (62.5, 1300))]
    return padded([r.astype(np.float32) for r in rows])


def edge_rows():
    """Zero except the first and the last 200 samples: the chains stop at the silence, and marks near 0 and len - 1 read +0 outside."""
    rows = []
    for i, n in enumerate((2490, 2533)):
        y = perturbed_pulses(n, 100.0, 0.01, 0.05, seed=50 + i, sr=SR_SMALL)
        y[200: n - 200] = 0.0
        rows.append(y)
    return padded(rows)


HAND_LAGS = (0, 15, 16, 2048, 2049, -3, 10 ** 9, 40, 40, 80, 20, 40, 39, 41)


def hand_rows():
    """(x, lens, lag): a good row under hand-made lags (out of range ones, twice and half the true period of 40), a zero row, a row with a silent
    middle, a row of one sample, len 0 and len > L beside a good row; the last five rows carry the lag 40 everywhere."""
    n = 2560
    good = perturbed_pulses(n, 100.0, 0.01, 0.05, seed=3, sr=SR_SMALL, noise=1e-3)
    hole = good.copy()
    hole[900:1700] = 0.0
    one = np.full(1, 0.5, np.float32)
    x, lens = padded([good, np.zeros(n, np.float32), hole, one, good, good, good])
    lens[4], lens[5] = 0, n + 1
    F = frames(n, 64)
    lag = np.full((7, F), 40, np.int64)
    lag[0] = [HAND_LAGS[f % len(HAND_LAGS)] for f in range(F)]
    return x, lens, lag.astype(np.int32)


def cases():
    """name -> (x, lens, lag, geo): every case of the device test that needs no device to state."""
    out = {}
    x, lens = small_rows()
    for nc in (1, 3, 16):
        g = geo(nc=nc)
        out[f"small-nc{nc}"] = (x, lens, yin_lags(x, lens, g), g)
    for W in (70, 8):
        g = geo(W=W)
        out[f"corr{W}"] = (x, lens, yin_lags(x, lens, g, frame_length=128), g)
    x, lens, lag = hand_rows()
    out["hand"] = (x, lens, lag, geo())
    x, lens = edge_rows()
    out["edges"] = (x, lens, np.full((2, frames(x.shape[1], 64)), 40, np.int32), geo())
    x, lens = plateau_rows()
    lag = np.stack([np.full(frames(x.shape[1], 64), t, np.int32) for t in (40, 64)])
    out["plateau"] = (x, lens, lag, geo())
    return out


AUDIO_LENS = [4000, 2600, 700]


def audio_rows():
    """The rows of the audio.perturbation case at 22050 Hz (H 256, W 1024, n_cycles 3)."""
    spec = ((120.0, 0.01, 0.05), (180.0, 0.005, 0.02), (100.0, 0.0, 0.0))
    return padded([perturbed_pulses(n, f0, j, s, seed=11 + i, noise=1e-3) for i, (n, (f0, j, s)) in enumerate(zip(AUDIO_LENS, spec))])


AUDIO_GEO = geo(H=256, W=1024, nc=3)
