"""numpy float64 restatement of probabilistic YIN (include/emojivoice.h): Mauch and Dixon's pYIN (ICASSP 2014) with a
Viterbi pass over (voiced / unvoiced) x pitch bins.  librosa is not a dependency: this file IS the yardstick, librosa.pyin the model.

Framing, d(tau) and d'(tau) for 1 <= tau <= n = tau_max + 1 are tests/pitch_ref.py's, unchanged; d'(0) := 1.

Observation, per frame
    troughs     the lags tau in [tau_min, tau_max] with d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1), ascending: tau_0 < tau_1 < ...
                (d' exists one lag beyond each end of the range, so the ends need no special rule; a silent frame, d' = 1, has none)
    thresholds  theta_t = t / n_thr, t = 1 .. n_thr, with the weights w_t = Beta(a, b) mass of (theta_{t-1}, theta_t]
    activity    active(k, t) = d'(tau_k) < theta_t;  pos(k, t) = #{m < k : active(m, t)};  N(t) = #{m : active(m, t)}
    P_k         sum_t [active(k, t)] G_t e^{-lambda pos(k, t)} in ascending t, G_t = w_t (1 - e^{-lambda}) / (1 - e^{-lambda N(t)})
    global min  g = the trough of smallest d', lowest lag on ties: P_g += no_trough_prob * sum_{t : not active(g, t)} w_t (the inactive t are
                a prefix 1 .. a_g - 1: the sum is the ascending chain of w up to there)
    period_k    tau_k + the parabolic shift of ev_pitch_yin (denominator > 0 and |shift| <= 1, else 0)
    bin_k       clip(rint(bins_per_octave * log2(sr / (period_k * fmin))), 0, n_bins - 1), half to even
    outputs     obs[bin_k] += P_k over the troughs with P_k > 0 in ascending k;  pv = min(sum_i obs[i], 1) in ascending i

Decoding, per row, over its ceil(len / H) frames; state s = v n_bins + i, v = 0 voiced, 1 unvoiced
    emission    e(0, i) = obs[i], e(1, i) = (1 - pv) / n_bins;  l = log(e + tiny), tiny the smallest normal double
    transition  (v', j) -> (v, i) for |i - j| <= R: log a = T_{v' = v}[|i - j|] - log Z_j, where T_stay[d] = log_tri[d] + log_stay and
                T_switch[d] = log_tri[d] + log_switch are formed first, log_tri[d] = log(R + 1 - d), Z_j = the sum of R + 1 - |i - j| over
                the i inside [0, n_bins)
    recursion   delta_0(s) = -log(2 n_bins) + l_0(s);  delta_t(s) = max_{s'} [(delta_{t-1}(s') - log Z_j) + T[|i - j|]] + l_t(s), the
                predecessors visited in ascending s', a later one replacing an earlier one only when STRICTLY greater; the end state is the
                lowest s of greatest delta
"""
import math

import numpy as np

import pitch_ref as P

TINY = np.finfo(np.float64).tiny


# ---- host tables ----------------------------------------------------------------------------------------------------------------------------
def beta_cdf_integer(x, a, b):
    """I_x(a, b) for integer a, b >= 1: the binomial tail sum_{j >= a} C(n, j) x^j (1 - x)^(n - j), n = a + b - 1."""
    n = a + b - 1
    return float(sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1)))


def threshold_prior(n_thr=100, beta_parameters=(2, 18)):
    """w_t, t = 1 .. n_thr (index t - 1): scipy's regularised incomplete beta function where scipy is present, else the closed form."""
    a, b = beta_parameters
    theta = np.arange(n_thr + 1, dtype=np.float64) / n_thr
    try:
        from scipy.special import betainc
        cdf = betainc(float(a), float(b), theta)
    except ImportError:
        cdf = np.array([beta_cdf_integer(float(t), int(a), int(b)) for t in theta])
    return np.diff(cdf)


def bins_of(fmin, fmax, resolution):
    bpo = 12 * int(math.ceil(1.0 / resolution))
    return bpo, int(math.floor(bpo * math.log2(fmax / fmin))) + 1


def transition_radius(sr, hop_length, bins_per_octave, max_transition_rate=35.92):
    return int((bins_per_octave // 12) * round(max_transition_rate * 12 * hop_length / sr) / 2)


def transition_tables(n_bins, R, switch_prob=0.01, truncate=True):
    """{"log_tri" (R + 1,), "log_Z" (n_bins,), "log_stay", "log_switch", "n_bins", "R"}; truncate=False is the mutant whose Z ignores the edges."""
    num = (R + 1 - np.arange(R + 1)).astype(np.float64)
    Z = np.zeros(n_bins)
    for j in range(n_bins):
        for i in range(j - R, j + R + 1):
            if not truncate or 0 <= i < n_bins:
                Z[j] += R + 1 - abs(i - j)
    return {"log_tri": np.log(num), "log_Z": np.log(Z), "log_stay": math.log(1.0 - switch_prob), "log_switch": math.log(switch_prob),
            "n_bins": int(n_bins), "R": int(R)}


# ---- observation ----------------------------------------------------------------------------------------------------------------------------
def troughs_of(dp, tau_min, tau_max, strict=True):
    """Ascending trough lags of d' (index tau - 1, length tau_max + 1); strict=False is the mutant with <= for <."""
    at = lambda t: 1.0 if t == 0 else float(dp[t - 1])
    left = (lambda t: at(t) < at(t - 1)) if strict else (lambda t: at(t) <= at(t - 1))
    return [t for t in range(tau_min, tau_max + 1) if left(t) and at(t) <= at(t + 1)]


def parabolic_period(dp, tau):
    a, b, c = (1.0 if tau == 1 else float(dp[tau - 2])), float(dp[tau - 1]), float(dp[tau])
    den = a - 2.0 * b + c
    shift = 0.0
    if den > 0:
        shift = 0.5 * (a - c) / den
        if not abs(shift) <= 1.0:
            shift = 0.0
    return tau + shift


def observe_frame(dp, tau_min, tau_max, sr, fmin, bpo, n_bins, w, boltzmann, no_trough_prob, strict=True, no_trough=True):
    """(obs (n_bins,), pv before the clip, fragile) of one frame from d'."""
    n_thr = len(w)
    obs = np.zeros(n_bins)
    taus = troughs_of(dp, tau_min, tau_max, strict)
    at = lambda t: 1.0 if t == 0 else float(dp[t - 1])
    fragile = False
    for t in range(tau_min, tau_max + 1):                                # the trough tests' margins, relative
        for u in (t - 1, t + 1):
            if abs(at(t) - at(u)) < 1e-7 * max(abs(at(t)), abs(at(u))) and not (at(t) == 1.0 and at(u) == 1.0):
                fragile = True
    if not taus:
        return obs, 0.0, fragile
    K = len(taus)
    v = np.array([dp[t - 1] for t in taus])
    theta = np.arange(1, n_thr + 1, dtype=np.float64) / n_thr
    if np.any(np.abs(v[:, None] - theta[None, :]) < 1e-7):
        fragile = True
    active = v[:, None] < theta[None, :]                                 # (K, n_thr), monotone in t
    pos = np.cumsum(active, axis=0) - active
    N = active.sum(axis=0)
    c0 = 1.0 - math.exp(-boltzmann)
    E = np.exp(-boltzmann * np.arange(K + 1, dtype=np.float64))
    G = np.where(N > 0, w * c0 / np.where(N > 0, 1.0 - E[N], 1.0), 0.0)
    Pk = np.zeros(K)
    for t in range(n_thr):                                               # ascending t
        Pk += np.where(active[:, t], G[t] * E[pos[:, t]], 0.0)
    if no_trough:
        g = int(np.argmin(v))                                            # (the first of the smallest)
        a_g = int(np.argmax(active[g])) if active[g].any() else n_thr    # inactive t (0-based): 0 .. a_g - 1
        Pk[g] += no_trough_prob * (float(np.cumsum(w)[a_g - 1]) if a_g > 0 else 0.0)
    for k, tau in enumerate(taus):
        q = bpo * math.log2(sr / (parabolic_period(dp, tau) * fmin))
        if abs(abs(q - math.floor(q)) - 0.5) < 1e-7:
            fragile = True
        b = int(min(max(np.rint(q), 0), n_bins - 1))
        if Pk[k] > 0:
            obs[b] += Pk[k]
    pv = 0.0
    for i in range(n_bins):
        pv += obs[i]
    return obs, pv, fragile


def observe(x, lengths=None, frame_length=1024, hop_length=256, tau_min=36, tau_max=340, sr=22050, fmin=65.0, bins_per_octave=120, n_bins=385,
            w=None, boltzmann=2.0, no_trough_prob=0.01, strict=True, no_trough=True):
    """x (B, L) or (L,) -> {"obs" (B, F, n_bins), "pv" (B, F) clipped to 1, "pv_raw" (B, F), "fragile" (B, F) bool}, F = ceil(L / H); frames past
    a row's own count and bad rows are zeros."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    B, L = x.shape
    F = P.frame_count(L, hop_length)
    w = threshold_prior() if w is None else np.asarray(w, dtype=np.float64)
    lens = [L] * B if lengths is None else [int(v) for v in lengths]
    out = {"obs": np.zeros((B, F, n_bins)), "pv": np.zeros((B, F)), "pv_raw": np.zeros((B, F)), "fragile": np.zeros((B, F), bool)}
    for b, n in enumerate(lens):
        if n < 1 or n > L:
            continue
        for f in range(P.frame_count(n, hop_length)):
            span = P.frame_span(x[b, :n], f, frame_length, hop_length, tau_max)
            dp = P.cmnd(P.difference(span, frame_length, tau_max))
            o, pv, fr = observe_frame(dp, int(tau_min), int(tau_max), float(sr), float(fmin), float(bins_per_octave), int(n_bins), w,
                                      float(boltzmann), float(no_trough_prob), strict, no_trough)
            out["obs"][b, f], out["pv_raw"][b, f], out["pv"][b, f], out["fragile"][b, f] = o, pv, min(pv, 1.0), fr
    return out


def fragile_frames(x, lengths=None, **kw):
    """(B, F) bool: the frames where a comparison of the observation lies within 1e-7 of flipping (a trough's d' against a threshold, a
    trough test, relative, or a candidate's bin position against a half-integer)."""
    return observe(x, lengths, **kw)["fragile"]


# ---- decoding -------------------------------------------------------------------------------------------------------------------------------
def emissions(obs, pv, n_bins):
    """l (F, 2 n_bins)."""
    obs, pv = np.asarray(obs, dtype=np.float64), np.asarray(pv, dtype=np.float64)
    e = np.concatenate([obs, np.repeat(((1.0 - pv) / n_bins)[:, None], n_bins, axis=1)], axis=1)
    return np.log(e + TINY)


def _T(tables):
    return tables["log_tri"] + tables["log_stay"], tables["log_tri"] + tables["log_switch"]


def viterbi(obs, pv, tables, lowest_on_ties=True):
    """(states (F,) int32, loglik) of one row; lowest_on_ties=False is the mutant whose ties go to the higher state."""
    nb, R = tables["n_bins"], tables["R"]
    l = emissions(obs, pv, nb)
    F, S = l.shape
    T_stay, T_switch = _T(tables)
    lz = np.tile(tables["log_Z"], 2)
    delta = -math.log(2 * nb) + l[0]
    back = np.zeros((F, S), np.int64)
    better = (lambda c, best: c > best) if lowest_on_ties else (lambda c, best: c >= best)
    for t in range(1, F):
        dz = delta - lz
        new = np.empty(S)
        for s in range(S):
            v, i = divmod(s, nb)
            best, arg = -np.inf, -1
            for vp in (0, 1):
                T = T_stay if vp == v else T_switch
                for j in range(max(i - R, 0), min(i + R, nb - 1) + 1):
                    c = dz[vp * nb + j] + T[abs(i - j)]
                    if arg < 0 or better(c, best):
                        best, arg = c, vp * nb + j
            new[s] = best + l[t, s]
            back[t, s] = arg
        delta = new
    end = int(np.argmax(delta)) if lowest_on_ties else int(S - 1 - np.argmax(delta[::-1]))
    states = np.zeros(F, np.int32)
    s = end
    for t in range(F - 1, -1, -1):
        states[t] = s
        s = int(back[t, s])
    return states, float(delta[end])


def viterbi_fast(obs, pv, tables):
    """The same recursion, the same additions in the same order, vectorised over the states (for the GPU tests' shapes)."""
    nb, R = tables["n_bins"], tables["R"]
    l = emissions(obs, pv, nb)
    F, S = l.shape
    T_stay, T_switch = _T(tables)
    lz = np.tile(tables["log_Z"], 2)
    delta = -math.log(2 * nb) + l[0]
    back = np.zeros((F, S), np.int64)
    idx = np.arange(nb)
    for t in range(1, F):
        dz = (delta - lz).reshape(2, nb)
        best = np.full((2, nb), -np.inf)
        arg = np.full((2, nb), -1, np.int64)
        for vp in (0, 1):
            for o in range(-R, R + 1):                                   # ascending j = i + o for every i at once
                j = idx + o
                ok = (j >= 0) & (j < nb)
                src = dz[vp, np.clip(j, 0, nb - 1)]
                for v in (0, 1):
                    c = src + (T_stay if vp == v else T_switch)[abs(o)]
                    take = ok & ((arg[v] < 0) | (c > best[v]))
                    best[v] = np.where(take, c, best[v])
                    arg[v] = np.where(take, vp * nb + j, arg[v])
        delta = best.reshape(S) + l[t]
        back[t] = arg.reshape(S)
    end = int(np.argmax(delta))
    states = np.zeros(F, np.int32)
    s = end
    for t in range(F - 1, -1, -1):
        states[t] = s
        s = int(back[t, s])
    return states, float(delta[end])


def path_score(states, obs, pv, tables):
    """The log-likelihood of a given state path under the model, summed in the recursion's order; -inf for a forbidden step."""
    nb, R = tables["n_bins"], tables["R"]
    l = emissions(obs, pv, nb)
    T_stay, T_switch = _T(tables)
    states = [int(s) for s in states]
    score = -math.log(2 * nb) + l[0, states[0]]
    for t in range(1, len(states)):
        (vp, j), (v, i) = divmod(states[t - 1], nb), divmod(states[t], nb)
        if abs(i - j) > R:
            return -np.inf
        score = ((score - tables["log_Z"][j]) + (T_stay if vp == v else T_switch)[abs(i - j)]) + l[t, states[t]]
    return float(score)


def pitch_pyin(y, sr=22050, fmin=65.0, fmax=600.0, frame_length=1024, hop_length=256, lengths=None, n_thresholds=100, beta_parameters=(2, 18),
               boltzmann_parameter=2.0, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01):
    """{"f0" (B, F) float64 Hz (0 unvoiced), "voiced" (B, F) bool, "voiced_prob" (B, F), "states" (B, F) int32 (-1 past a row)}."""
    x = np.atleast_2d(np.asarray(y, dtype=np.float32))
    B, L = x.shape
    tau_min, tau_max = int(math.floor(sr / fmax)), int(math.ceil(sr / fmin))
    bpo, nb = bins_of(fmin, fmax, resolution)
    R = transition_radius(sr, hop_length, bpo, max_transition_rate)
    tables = transition_tables(nb, R, switch_prob)
    o = observe(x, lengths, frame_length, hop_length, tau_min, tau_max, sr, fmin, bpo, nb, threshold_prior(n_thresholds, beta_parameters),
                boltzmann_parameter, no_trough_prob)
    F = o["pv"].shape[1]
    lens = [L] * B if lengths is None else [int(v) for v in lengths]
    states = np.full((B, F), -1, np.int32)
    for b, n in enumerate(lens):
        nf = P.frame_count(n, hop_length) if 1 <= n <= L else 0
        if nf:
            states[b, :nf] = viterbi_fast(o["obs"][b, :nf], o["pv"][b, :nf], tables)[0]
    voiced = (states >= 0) & (states < nb)
    f0 = np.where(voiced, fmin * 2.0 ** (np.where(voiced, states, 0) / bpo), 0.0)
    return {"f0": f0, "voiced": voiced, "voiced_prob": o["pv"], "states": states}


# ---- the cases tests/test_gpu_pyin.py runs on the device (tests/test_pyin_host.py checks their fragile share on the CPU) ------------------------
def vibrato_tone(f0, n, sr=22050, depth=0.03, rate=5.5, amps=(1.0, 0.5, 0.25), scale=0.3):
    t = np.arange(n) / sr
    phase = 2 * np.pi * f0 * (t - depth / (2 * np.pi * rate) * np.cos(2 * np.pi * rate * t))
    return (scale * sum(a * np.sin((k + 1) * phase + 0.3 * k) for k, a in enumerate(amps))).astype(np.float32)


def geometry(sr, fmin, fmax, frame_length, hop_length, resolution, n_thr=100, beta_parameters=(2, 18)):
    bpo, nb = bins_of(fmin, fmax, resolution)
    return dict(frame_length=frame_length, hop_length=hop_length, tau_min=int(math.floor(sr / fmax)), tau_max=int(math.ceil(sr / fmin)), sr=sr,
                fmin=fmin, bins_per_octave=bpo, n_bins=nb, w=threshold_prior(n_thr, beta_parameters), boltzmann=2.0, no_trough_prob=0.01)


def std_case(seed=3):
    """(x (3, 8192) with garbage behind each length, lengths, observe keywords): the defaults, lags 36 .. 340, 385 bins."""
    L, lens = 8192, [8192, 7000, 5001]
    g = np.random.default_rng(seed)
    x = np.full((3, L), P.GARBAGE, np.float32)
    x[0] = vibrato_tone(170.0, L)
    x[1, :7000] = P.chirp(100.0, 300.0, 7000) + (0.02 * g.standard_normal(7000)).astype(np.float32)
    x[2, :5001] = P.mixed_row(5001, seed=1)
    return x, lens, geometry(22050, 65.0, 600.0, 1024, 256, 0.1)


def small_case(seed=5):
    """W 512, H 128, 100 - 400 Hz, resolution 0.5 (49 bins); the row lengths are no multiples of the hop."""
    L, lens = 3001, [3001, 2500]
    g = np.random.default_rng(seed)
    x = np.full((2, L), P.GARBAGE, np.float32)
    x[0] = vibrato_tone(210.0, L)
    x[1, :2500] = P.chirp(120.0, 350.0, 2500) + (0.02 * g.standard_normal(2500)).astype(np.float32)
    return x, lens, geometry(22050, 100.0, 400.0, 512, 128, 0.5)


def tables_for(kw, switch_prob=0.01):
    return transition_tables(kw["n_bins"], transition_radius(kw["sr"], kw["hop_length"], kw["bins_per_octave"]), switch_prob)


def random_model(n_bins, R, F, seed):
    """A decoding problem of its own: sparse random obs rows (a track that moves by at most R bins a frame and is absent from some frames,
    plus a few stray bins) and the tables."""
    g = np.random.default_rng(seed)
    obs = np.zeros((F, n_bins))
    track = int(g.integers(0, n_bins))
    for t in range(F):
        track = int(np.clip(track + g.integers(-R, R + 1), 0, n_bins - 1))
        if g.random() < 0.75:
            obs[t, track] += 0.3 + 0.5 * g.random()
        for _ in range(int(g.integers(0, 3))):
            obs[t, int(g.integers(0, n_bins))] += g.random() * 0.1
    pv = np.minimum(obs.sum(axis=1), 1.0)
    return obs, pv, transition_tables(n_bins, R)
