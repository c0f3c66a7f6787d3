"""numpy restatement of ev_formant_track (include/emojivoice.h): a Viterbi pass over the ways of mapping n_tracks tracks onto the candidates of a
frame, in float64 and in np.longdouble.  Vectorised over the states of a frame.

    states     the strictly increasing index tuples c(0) < .. < c(n_tracks - 1) over 0 .. n_cand - 1 in lexicographic order (itertools.combinations)
    trackable  m = min(count, n_cand) >= n_tracks and the first m candidates have finite f > 0 and finite bw; every other frame is a GAP
    valid      c(n_tracks - 1) < m, else the state costs +inf
    local      sum_k (cost_f |f - ref[k]|) / 1000 + (cost_b bw) / f            (ascending k from the first term)
    trans      sum_k cost_j |log2 f_{t-1}[c_s(k)] - log2 f_t[c_s'(k)]|         (ascending k from the first term)
    delta      local at a segment's first frame, else min_s (delta_{t-1}(s) + trans) + local, of equal minima the lowest s
    end        the lowest s of least delta at the segment's last frame; back-pointers give the rest; nothing crosses a gap
The device uses its own log2, so it differs from the float64 restatement by float64 rounding in the costs; the longdouble evaluation and
``margins`` measure how much rounding the INPUT admits before a decision moves.
"""
import itertools
import math

import numpy as np

TOL = 1e-9                       # device d_cost against the float64 restatement: |got - ref| <= TOL max(|ref|, 1)
INPUT_TOL = 1e-11                # float64 against longdouble restatement, the same form: the condition on the input
MIN_MARGIN = 1e-6                # every decision's second best lies at least this far over the best
REFERENCE = (550.0, 1650.0, 2750.0)
MUTANTS = ("no_bandwidth_cost", "linear_hz_transition", "ties_to_highest", "cross_gaps", "local_cost_twice_at_start", "unordered_states")


def n_states(n_cand, n_tracks):
    return math.comb(int(n_cand), int(n_tracks))


def states(n_cand, n_tracks, unordered=False):
    """(S, n_tracks) int: the tuples in lexicographic order (``unordered``: the mutant that lets tracks cross, every arrangement)."""
    it = itertools.permutations if unordered else itertools.combinations
    return np.array(list(it(range(int(n_cand)), int(n_tracks))), dtype=np.int64).reshape(-1, int(n_tracks))


def default_reference(n_tracks):
    """550, 1650, 2750, .. Hz: the neutral vocal tract's resonances, Praat's defaults continued."""
    return tuple(550.0 * (2 * k + 1) for k in range(int(n_tracks)))


def trackable(fm, ct, n_tracks):
    """fm (NF, n_cand, 2), ct (NF,) -> m (NF,) int: min(count, n_cand) on trackable frames, -1 on gaps."""
    fm, ct = np.asarray(fm, dtype=np.float64), np.asarray(ct).astype(np.int64)
    nc = fm.shape[1]
    m = np.minimum(ct, nc)
    inside = np.arange(nc)[None, :] < m[:, None]
    with np.errstate(invalid="ignore"):
        good = np.isfinite(fm[..., 0]) & (fm[..., 0] > 0) & np.isfinite(fm[..., 1])
    ok = (m >= int(n_tracks)) & (good | ~inside).all(axis=1)
    return np.where(ok, m, -1)


def _chain(terms):
    """terms (.., K): the sum over the last axis in ascending index starting from the first term."""
    s = terms[..., 0]
    for k in range(1, terms.shape[-1]):
        s = s + terms[..., k]
    return s


def _local(f, bw, m, T, ref, cf, cb, dtype):
    with np.errstate(all="ignore"):
        term = (dtype(cf) * np.abs(f[T] - ref[None, :])) / dtype(1000) + (dtype(cb) * bw[T]) / f[T]       # (S, K)
    loc = _chain(np.where(T < m, term, dtype(0)))
    return np.where(T.max(axis=1) < m, loc, dtype(np.inf))        # (the greatest index is the last one, except for the mutant's arrangements)


def _trans(lp, mp, l, m, T, cj, dtype):
    """(S, S): [s, s'] = the transition from s in the frame before to s' in this one (0 where a candidate at or past m is involved)."""
    nc = lp.shape[0]
    with np.errstate(all="ignore"):
        D = dtype(cj) * np.abs(lp[:, None] - l[None, :])
    D = np.where((np.arange(nc)[:, None] < mp) & (np.arange(nc)[None, :] < m), D, dtype(0))
    tr = D[T[:, 0][:, None], T[:, 0][None, :]]
    for k in range(1, T.shape[1]):
        tr = tr + D[T[:, k][:, None], T[:, k][None, :]]
    return tr


def row(fm, ct, n_tracks, ref=None, cost_f=1.0, cost_b=1.0, cost_j=1.0, dtype=np.float64, mutant=None, want_margin=False):
    """One row: fm (NF, n_cand, 2) {f, bw}, ct (NF,) -> (track (NF, n_tracks, 2) float64: the chosen candidates, zeros on gaps; sel (NF,) int32:
    the state, -1 on gaps; cost (NF,) ``dtype``: the segment's optimum at its last frame, 0 elsewhere; choice (NF, n_tracks) int: the chosen
    candidate indices, -1 on gaps; margin: with ``want_margin`` the least over all decisions (every valid target state of every frame behind a
    segment's first, and every segment's end state) of second best minus best, inf without a decision)."""
    assert mutant is None or mutant in MUTANTS
    fm64 = np.asarray(fm, dtype=np.float64)
    NF, nc, _ = fm64.shape
    K = int(n_tracks)
    ref = np.asarray(default_reference(K) if ref is None else ref, dtype=np.float64).astype(dtype)
    T = states(nc, K, unordered=mutant == "unordered_states")
    S = T.shape[0]
    m_all = trackable(fm64, ct, K)
    if mutant == "no_bandwidth_cost":
        cost_b = 0.0
    fa, ba = fm64[..., 0].astype(dtype), fm64[..., 1].astype(dtype)
    with np.errstate(all="ignore"):
        la = fa / dtype(1000) if mutant == "linear_hz_transition" else np.log2(fa)
    track, sel, cost = np.zeros((NF, K, 2)), np.full(NF, -1, np.int32), np.zeros(NF, dtype)
    choice = np.full((NF, K), -1, np.int64)
    margin = np.inf
    pick = (lambda v: len(v) - 1 - int(np.argmin(v[::-1]))) if mutant == "ties_to_highest" else (lambda v: int(np.argmin(v)))

    def second_minus_best(v):
        v = np.sort(v[np.isfinite(v)])
        return float(v[1] - v[0]) if len(v) > 1 else np.inf

    def finish(frames, deltas, backs):
        nonlocal margin
        end = pick(deltas[-1])
        if want_margin:
            margin = min(margin, second_minus_best(deltas[-1]))
        cost[frames[-1]] = deltas[-1][end]
        s = end
        for i in range(len(frames) - 1, -1, -1):
            t = frames[i]
            sel[t], choice[t] = s, T[s]
            track[t] = fm64[t, T[s]]
            if i > 0:
                s = backs[i][s]

    frames, deltas, backs = [], [], []
    for t in range(NF):
        m = m_all[t]
        if m < 0:
            if mutant != "cross_gaps" and frames:
                finish(frames, deltas, backs)
                frames, deltas, backs = [], [], []
            continue
        loc = _local(fa[t], ba[t], m, T, ref, cost_f, cost_b, dtype)
        if not frames:
            deltas.append(loc + loc if mutant == "local_cost_twice_at_start" else loc)
            backs.append(None)
        else:
            tp = frames[-1]
            cand = deltas[-1][:, None] + _trans(la[tp], m_all[tp], la[t], m, T, cost_j, dtype)       # (S, S'): inf where s is not valid
            arg = np.array([pick(cand[:, s2]) for s2 in range(S)]) if mutant == "ties_to_highest" else np.argmin(cand, axis=0)
            best = cand[arg, np.arange(S)]
            valid = np.isfinite(loc)
            if want_margin and S > 1:
                two = np.partition(cand[:, valid], 1, axis=0)[:2]
                with np.errstate(invalid="ignore"):
                    gap = np.where(np.isfinite(two[1]), two[1] - two[0], np.inf)
                margin = min(margin, float(gap.min()))
            deltas.append(np.where(valid, best + loc, dtype(np.inf)))
            backs.append(np.where(valid, arg, 0))
        frames.append(t)
    if frames:
        finish(frames, deltas, backs)
    return (track, sel, cost, choice, margin) if want_margin else (track, sel, cost, choice)


def batch(fm, ct, n_tracks, ref=None, cost_f=1.0, cost_b=1.0, cost_j=1.0, dtype=np.float64, mutant=None):
    """ev_formant_track's shapes: fm (B, NF, n_cand, 2), ct (B, NF) -> track (B, NF, n_tracks, 2), sel (B, NF) int32, cost (B, NF), choice (B, NF,
    n_tracks), margin (B,)."""
    fm, ct = np.asarray(fm), np.asarray(ct)
    rows = [row(fm[b], ct[b], n_tracks, ref, cost_f, cost_b, cost_j, dtype, mutant, want_margin=True) for b in range(fm.shape[0])]
    return tuple(np.stack([r[i] for r in rows]) for i in range(4)) + (np.array([r[4] for r in rows]),)


def margins(fm, ct, n_tracks, ref=None, cost_f=1.0, cost_b=1.0, cost_j=1.0):
    """(B,): per row the least margin of a decision (``row``), float64."""
    return batch(fm, ct, n_tracks, ref, cost_f, cost_b, cost_j)[4]


def path_score(sel, fm, ct, n_tracks, ref=None, cost_f=1.0, cost_b=1.0, cost_j=1.0, dtype=np.float64):
    """The definition's cost of the path ``sel`` (NF,) through one row, segment by segment -> (NF,) ``dtype``: each segment's total at its last
    frame, 0 elsewhere; inf where the path takes a state that is not valid in its frame.  ``sel`` must hold a state on every trackable frame."""
    fm64 = np.asarray(fm, dtype=np.float64)
    NF, nc, _ = fm64.shape
    K = int(n_tracks)
    ref = np.asarray(default_reference(K) if ref is None else ref, dtype=np.float64).astype(dtype)
    T = states(nc, K)
    m_all = trackable(fm64, ct, K)
    fa, ba = fm64[..., 0].astype(dtype), fm64[..., 1].astype(dtype)
    with np.errstate(all="ignore"):
        la = np.log2(fa)
    out = np.zeros(NF, dtype)
    total, inside = dtype(0), False
    for t in range(NF):
        m = m_all[t]
        if m >= 0:
            s = int(sel[t])
            loc = _local(fa[t], ba[t], m, T[s:s + 1], ref, cost_f, cost_b, dtype)[0]
            if not inside:
                total = loc
            else:
                sp = int(sel[t - 1])
                valid_p = T[sp].max() < m_all[t - 1]
                tr = _trans(la[t - 1], m_all[t - 1], la[t], m, np.stack([T[sp], T[s]]), cost_j, dtype)[0, 1]
                total = (total + tr) + loc if valid_p else dtype(np.inf)
            inside = True
            if t + 1 == NF or m_all[t + 1] < 0:
                out[t] = total
                inside = False
    return out


def err(got, ref):
    """max over the entries of |got - ref| / max(|ref|, 1)."""
    got, ref = np.asarray(got).astype(np.longdouble), np.asarray(ref).astype(np.longdouble)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1)))


def random_candidates(B, NF, n_cand, n_tracks, seed, lo=500.0, hi=5000.0):
    """Seeded ascending candidates with counts drawn from n_tracks .. n_cand: (fm (B, NF, n_cand, 2), ct (B, NF) int32); zeros past the count.
    Frequencies wander from frame to frame around n_cand evenly spread centres, so that neither the reference nor the continuity decides alone."""
    rng = np.random.default_rng(seed)
    centre = np.linspace(lo, hi, n_cand + 2)[1:-1]
    step = (hi - lo) / (n_cand + 1)
    f = centre[None, None, :] + rng.uniform(-1.5, 1.5, (B, NF, n_cand)) * step
    f = np.sort(150.0 + np.abs(f - 150.0), axis=-1)                      # (reflected at 150 Hz: every frequency is positive)
    bw = rng.uniform(40.0, 600.0, (B, NF, n_cand))
    ct = rng.integers(n_tracks, n_cand + 1, (B, NF)).astype(np.int32)
    fm = np.stack([f, bw], axis=-1)
    fm[np.arange(n_cand)[None, None, :] >= ct[..., None]] = 0.0
    return fm, ct


def planted_row(NF=30, every=3, seed=0):
    """A row of 5 candidates whose frames hold three planted contours near 600 / 1500 / 2600 Hz (steps of at most 25 Hz between frames) and a
    fourth near 3700 Hz; on every ``every``-th frame a spurious narrow candidate sits at 260 Hz, below F1 -> (fm (NF, 5, 2), ct (NF,), planted
    (NF, 3), step: the largest step of a planted contour)."""
    rng = np.random.default_rng(seed)
    base = np.array([600.0, 1500.0, 2600.0, 3700.0])
    walk = np.cumsum(rng.uniform(-25.0, 25.0, (NF, 4)), axis=0) * 0.5
    true = base[None, :] + walk
    fm, ct = np.zeros((NF, 5, 2)), np.zeros(NF, np.int32)
    for t in range(NF):
        cands = [(f, 90.0 + 10.0 * i) for i, f in enumerate(true[t])]
        if t % every == every - 1:
            cands = [(260.0, 60.0)] + cands
        ct[t] = len(cands)
        fm[t, :len(cands)] = cands
    return fm, ct, true[:, :3], float(np.abs(np.diff(true[:, :3], axis=0)).max())


# ---- the cases the device is held to (tests/test_gpu_formant_track.py); their input conditions are measured on the CPU (tests/test_formant_track_host.py)
SPEECH_CASES = ((2000, 24, 10, 6, 3, 2), (2000, 64, 16, 8, 4, 3), (11025, 512, 128, 10, 5, 3))    # sr, W, H, order, candidates, tracks
SPEECH_IDS = ["-".join(str(v) for v in c) for c in SPEECH_CASES]
RANDOM_CASES = ((1, 1), (4, 4), (3, 2), (5, 3), (8, 4), (16, 3), (12, 5))                          # (n_cand, n_tracks): S = 1, 1, 3, 10, 70, 560, 792
RANDOM_IDS = [f"{c}-{k}" for c, k in RANDOM_CASES]


def speech_case(i):
    """(fm (3, NF, n_cand, 2), ct (3, NF), n_tracks): the float64 restatement of ev_formants (formants_ref.batch) on formants_ref.rows_for at
    geometry ``SPEECH_CASES[i]``: three ragged speech-like rows."""
    import formants_ref as F

    sr, W, H, order, nc, nt = SPEECH_CASES[i]
    g = F.geometry(sr, W, H, order, nform=nc)
    x, lens = F.rows_for(g)
    _, fm, ct, _, _ = F.batch(x, lens, g)
    return fm, ct, nt


def random_case(n_cand, n_tracks):
    """(fm, ct, n_tracks) of ``random_candidates``: two rows of 61 frames, or one row of 40 where S > 64."""
    big = n_states(n_cand, n_tracks) > 64
    fm, ct = random_candidates(1 if big else 2, 40 if big else 61, n_cand, n_tracks, seed=100 * n_cand + n_tracks)
    return fm, ct, n_tracks


def edge_case(name):
    """(fm (1, NF, 5, 2), ct (1, NF), 3): 5 candidates, 3 tracks, 24 frames of ``random_candidates`` with the named damage."""
    fm, ct = random_candidates(1, 24, 5, 3, seed=7)
    fm, ct = fm.copy(), ct.copy()
    if name == "gap_at_frame_0":
        ct[0, 0] = 0
    elif name == "gap_at_the_last_frame":
        ct[0, -1] = 2
    elif name == "two_adjacent_gaps":
        ct[0, 9:11] = 0
    elif name == "single_frame_segments":
        ct[0, 1::2] = 0
    elif name == "all_gaps":
        ct[0, :] = (0, -1, 1, 2) * 6
    elif name == "unconverged_frames":
        ct[0, (3, 4, 15), ] = -1
    elif name == "count_over_n_cand":
        full = np.flatnonzero(ct[0] == 5)
        assert len(full) >= 3
        ct[0, full[::2]] = 9
    elif name == "zero_and_nan_candidates":
        fm[0, 5, 1, 0] = 0.0                                             # f = 0 inside the count
        fm[0, 12, 0, 0] = np.nan                                         # f = NaN inside the count
        fm[0, 18, 2, 1] = np.inf                                         # bw = inf inside the count
        t = [int(q) for q in np.flatnonzero(ct[0] == 5) if q not in (5, 12, 18)][-1]
        fm[0, t, 4, 0], ct[0, t] = np.nan, 4                             # NaN PAST the count: not looked at, the frame stays trackable
    elif name == "one_frame":
        fm, ct = fm[:, :1], ct[:, :1]
    elif name == "two_frames":
        fm, ct = fm[:, :2], ct[:, :2]
    else:
        raise KeyError(name)
    return fm, ct, 3


EDGE_CASES = ("gap_at_frame_0", "gap_at_the_last_frame", "two_adjacent_gaps", "single_frame_segments", "all_gaps", "unconverged_frames",
              "count_over_n_cand", "zero_and_nan_candidates", "one_frame", "two_frames")


def conditioned(fm, ct, n_tracks, what, ref=None, cost_f=1.0, cost_b=1.0, cost_j=1.0):
    """The conditions on the INPUT of a device case, asserted: the float64 and the longdouble restatements choose EQUAL paths, their costs agree
    within INPUT_TOL max(|ref|, 1), and every decision's margin is at least MIN_MARGIN -> the float64 restatement (``batch``) and the figures
    {"cost_spread", "margin"}."""
    r64 = batch(fm, ct, n_tracks, ref, cost_f, cost_b, cost_j)
    rld = batch(fm, ct, n_tracks, ref, cost_f, cost_b, cost_j, dtype=np.longdouble)
    spread, margin = err(r64[2], rld[2]), float(r64[4].min())
    assert np.array_equal(r64[1], rld[1]), f"{what}: the float64 and longdouble restatements choose different paths"
    assert spread <= INPUT_TOL, f"{what}: the float64 and longdouble restatements' costs differ by {spread:.3e}, over {INPUT_TOL:g}"
    assert margin >= MIN_MARGIN, f"{what}: a decision's margin is {margin:.3e}, under {MIN_MARGIN:g}"
    return r64, {"cost_spread": spread, "margin": margin}
