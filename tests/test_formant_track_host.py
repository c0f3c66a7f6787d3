"""Formant tracking on the host: tests/formant_track_ref.py (the numpy restatement of ev_formant_track's definition in include/emojivoice.h) against
brute-force enumeration, its mutants, a planted row, the argument checks of audio.formant_tracks, and the input conditions of the cases
tests/test_gpu_formant_track.py holds the device to.  No GPU.
"""
import itertools

import numpy as np
import pytest
import torch

import formant_track_ref as R
from emojivoice_amd import audio
from emojivoice_amd._lib import EvLibraryError


def brute_force(fm, ct, nt, ref=None, cf=1.0, cb=1.0, cj=1.0):
    """Every path through every segment of one row, enumerated: (sel (NF,), cost (NF,)) of the cheapest, summed in the definition's order
    ((total + trans) + local, frame by frame).  Among equal totals the first in lexicographic order: the cases have no ties."""
    fm = np.asarray(fm, dtype=np.float64)
    NF, nc, _ = fm.shape
    refv = np.asarray(R.default_reference(nt) if ref is None else ref, dtype=np.float64)
    T = R.states(nc, nt)
    S = len(T)
    m = R.trackable(fm, ct, nt)
    with np.errstate(all="ignore"):
        lg = np.log2(fm[..., 0])
    sel, cost = np.full(NF, -1, np.int32), np.zeros(NF)
    t = 0
    while t < NF:
        if m[t] < 0:
            t += 1
            continue
        e = t
        while e + 1 < NF and m[e + 1] >= 0:
            e += 1
        loc = [R._local(fm[q, :, 0], fm[q, :, 1], m[q], T, refv, cf, cb, np.float64) for q in range(t, e + 1)]
        tr = [None] + [R._trans(lg[q - 1], m[q - 1], lg[q], m[q], T, cj, np.float64) for q in range(t + 1, e + 1)]
        best = (np.inf, None)
        for path in itertools.product(range(S), repeat=e - t + 1):
            total = loc[0][path[0]]
            for i in range(1, len(path)):
                total = (total + tr[i][path[i - 1], path[i]]) + loc[i][path[i]]
            if total < best[0]:
                best = (total, path)
        sel[t:e + 1], cost[e] = best[1], best[0]
        t = e + 1
    return sel, cost


def small_cases():
    """(fm (NF, n_cand, 2), ct (NF,), n_tracks, kw) on 4 to 6 frames with (3, 2) and (4, 2): random rows, one with a gap in the middle, one whose
    reference frequencies are not ascending (the tracks still may not cross)."""
    out = []
    for i, (nc, NF) in enumerate(((3, 4), (3, 6), (4, 5), (4, 6), (4, 6))):
        fm, ct = R.random_candidates(1, NF, nc, 2, seed=50 + i)
        out.append((fm[0], ct[0], 2, {}))
    fm, ct = R.random_candidates(1, 6, 4, 2, seed=60)
    ct = ct.copy()
    ct[0, 3] = 1                                                         # too few candidates: a gap between two segments
    out.append((fm[0], ct[0], 2, {}))
    fm, ct = R.random_candidates(1, 5, 4, 2, seed=61)
    out.append((fm[0], ct[0], 2, {"ref": (1650.0, 550.0)}))
    return out


def tied_case():
    """Four frames of 3 candidates whose candidates 0 and 1 are the same entry in the last frame: the states (0, 2) and (1, 2) tie there."""
    fm, ct = R.random_candidates(1, 4, 3, 2, seed=70)
    fm, ct = fm[0].copy(), np.full(4, 3, np.int32)
    fm[:, :, 0] = np.array([600.0, 1400.0, 1700.0]) + np.arange(4)[:, None] * 5.0
    fm[:, :, 1] = 100.0
    fm[3, 0] = fm[3, 1] = (640.0, 100.0)
    return fm, ct, 2, {}


def test_the_restatement_finds_the_cheapest_of_all_paths():
    for i, (fm, ct, nt, kw) in enumerate(small_cases()):
        track, sel, cost, choice = R.row(fm, ct, nt, **kw)
        bsel, bcost = brute_force(fm, ct, nt, **kw)
        assert np.array_equal(sel, bsel), f"case {i}: {sel.tolist()} against the enumeration's {bsel.tolist()}"
        assert np.array_equal(cost, bcost), f"case {i}: the optimum's cost, summed in the same order, is the same number"
        assert np.array_equal(R.path_score(sel, fm, ct, nt, **kw), cost), f"case {i}: path_score of the chosen path"
        on = sel >= 0
        assert np.array_equal(track[on], np.stack([fm[t, choice[t]] for t in np.flatnonzero(on)])) and not track[~on].any() and (choice[~on] == -1).all()
        assert (np.diff(choice[on], axis=1) > 0).all(), "tracks do not cross"
        ld = R.row(fm, ct, nt, dtype=np.longdouble, **kw)
        assert np.array_equal(ld[1], sel) and R.err(cost, ld[2]) <= R.INPUT_TOL


def test_states_are_the_increasing_tuples_in_lexicographic_order():
    T = R.states(5, 3)
    assert len(T) == R.n_states(5, 3) == 10 and T[0].tolist() == [0, 1, 2] and T[1].tolist() == [0, 1, 3] and T[-1].tolist() == [2, 3, 4]
    assert sorted(map(tuple, T)) == list(map(tuple, T)) and (np.diff(T, axis=1) > 0).all()
    assert np.array_equal(audio.formant_track_states(5, 3), T) and np.array_equal(audio.formant_track_states(12, 5), R.states(12, 5))
    assert [R.n_states(*c) for c in R.RANDOM_CASES] == [1, 1, 3, 10, 70, 560, 792] and R.n_states(16, 8) == 12870


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_moves_an_output_on_the_small_cases(mutant):
    """The true definition agrees with the enumeration on every small case (above); each mutant differs from it in a selection, a track or a
    cost of at least one of them, by far more than rounding."""
    moved = []
    for fm, ct, nt, kw in small_cases() + [tied_case()]:
        good, bad = R.row(fm, ct, nt, **kw), R.row(fm, ct, nt, mutant=mutant, **kw)
        d_track, d_cost = np.abs(bad[0] - good[0]).max(), np.abs(bad[2] - good[2]).max()
        d_sel = 0 if mutant == "unordered_states" else int((bad[1] != good[1]).sum())        # (the mutant numbers its states differently)
        moved.append(d_sel > 0 or d_track > 1.0 or d_cost > 1e-6)
    assert any(moved), f"{mutant} moves nothing on the small cases"
    if mutant in ("ties_to_highest", "cross_gaps", "unordered_states"):
        assert not all(moved), f"{mutant} is only visible where its rule is exercised"


def test_a_spurious_low_candidate_shifts_lowest_n_and_not_the_tracks():
    fm, ct, planted, step = R.planted_row()
    track, sel, cost, choice, margin = R.row(fm, ct, 3, want_margin=True)
    spurious = ct == 5
    assert spurious.sum() == 10 and (sel >= 0).all() and margin >= R.MIN_MARGIN
    lowest = fm[:, :3, 0]
    jumps = np.abs(np.diff(lowest, axis=0)).max(axis=1)
    assert (jumps[spurious[1:] != spurious[:-1]] > 300.0).all(), "lowest-n: every slot jumps where the spurious candidate comes and goes"
    assert np.array_equal(track[..., 0], planted), "the tracks are the planted contours"
    assert np.abs(np.diff(track[..., 0], axis=0)).max() <= step <= 25.0
    assert (choice[spurious] == [1, 2, 3]).all() and (choice[~spurious] == [0, 1, 2]).all()


# ---- audio.formant_tracks: every check happens on the host, before a device is touched ------------------------------------------------------
def _fm(B=2, F=7, n=5, one=False):
    fm, ct = R.random_candidates(B, F, n, min(3, n), seed=5)
    d = {"frequency": torch.from_numpy(fm[..., 0]), "bandwidth": torch.from_numpy(fm[..., 1]), "count": torch.from_numpy(ct)}
    return {k: v[0] for k, v in d.items()} if one else d


BAD_ARGUMENTS = [
    ("n_tracks=0", dict(n_tracks=0)), ("n_tracks=6", dict(n_tracks=6)), ("n_tracks=2.5", dict(n_tracks=2.5)),
    ("reference must hold", dict(reference=(550.0, 1650.0))), ("reference=", dict(reference=(550.0, 0.0, 2750.0))),
    ("reference=", dict(reference=(550.0, float("nan"), 2750.0))), ("reference=", dict(reference=(550.0, float("inf"), 2750.0))),
    ("frequency_cost=", dict(frequency_cost=-1.0)), ("bandwidth_cost=", dict(bandwidth_cost=float("nan"))),
    ("transition_cost=", dict(transition_cost=float("inf"))),
]


@pytest.mark.parametrize("word,kw", BAD_ARGUMENTS, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_ARGUMENTS)])
def test_formant_tracks_checks_its_arguments_on_the_host(word, kw):
    with pytest.raises(ValueError, match="formant_tracks") as e:
        audio.formant_tracks(_fm(), **kw)
    assert word in str(e.value), str(e.value)


def test_formant_tracks_checks_its_input_on_the_host():
    fm = _fm()
    for bad, word in ((dict(fm, count=fm["count"][:, :-1]), "count"), (dict(fm, bandwidth=fm["bandwidth"][..., :4]), "bandwidth"),
                      ({k: v for k, v in fm.items() if k != "count"}, "dict"), (dict(fm, frequency=fm["frequency"][0, 0], bandwidth=fm["bandwidth"][0, 0]), "(F, n_cand)")):
        with pytest.raises(ValueError, match="formant_tracks") as e:
            audio.formant_tracks(bad)
        assert word in str(e.value), str(e.value)
    wide = {"frequency": torch.ones(1, 3, 17, dtype=torch.float64), "bandwidth": torch.ones(1, 3, 17, dtype=torch.float64), "count": torch.ones(1, 3, dtype=torch.int32)}
    with pytest.raises(ValueError, match="n_cand=17"):
        audio.formant_tracks(wide)
    many = {k: (v[..., :16] if v.dim() == 3 else v) for k, v in wide.items()}
    with pytest.raises(ValueError, match="S=12870"):
        audio.formant_tracks(many, n_tracks=8, reference=R.default_reference(8))
    empty = {"frequency": torch.ones(1, 0, 5, dtype=torch.float64), "bandwidth": torch.ones(1, 0, 5, dtype=torch.float64), "count": torch.ones(1, 0, dtype=torch.int32)}
    with pytest.raises(ValueError, match="no frames"):
        audio.formant_tracks(empty)


def test_formant_tracks_has_no_fallback_on_the_host():
    a = audio.formant_track_arguments(_fm(one=True))
    assert a["one"] and (a["n_cand"], a["n_tracks"], a["S"]) == (5, 3, 10) and a["reference"].tolist() == list(audio.FORMANT_TRACK_REFERENCE)
    assert audio.FORMANT_TRACK_REFERENCE == R.REFERENCE == R.default_reference(3)
    for fm in (_fm(), _fm(one=True)):
        with pytest.raises(EvLibraryError, match="no CPU fallback"):
            audio.formant_tracks(fm)


# ---- the input conditions of the device's cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SPEECH_CASES)), ids=R.SPEECH_IDS)
def test_input_conditions_of_the_speech_cases(i):
    """No frame needs to be left out of the device's comparison, and none may be: equal paths in float64 and longdouble, costs within 1e-11,
    every margin at least 1e-6.  The tracker chooses another assignment than "lowest n" on a good part of the trackable frames."""
    fm, ct, nt = R.speech_case(i)
    r, fig = R.conditioned(fm, ct, nt, R.SPEECH_IDS[i])
    on = r[1] >= 0
    other = on & (r[0][..., 0] != fm[:, :, :nt, 0]).any(axis=-1)
    print(f"\nformant_track {R.SPEECH_IDS[i]}: {fm.shape[1]} frames, trackable {on.sum(axis=1).tolist()}, another assignment than lowest-n on "
          f"{other.sum(axis=1).tolist()}, least margin {fig['margin']:.3e}, float64 against longdouble {fig['cost_spread']:.3e}")
    assert on.sum() > on.size // 2 and (other.sum(axis=1) >= 5).all()
    for b in range(fm.shape[0]):
        assert np.array_equal(R.path_score(r[1][b], fm[b], ct[b], nt), r[2][b])


@pytest.mark.parametrize("c", R.RANDOM_CASES, ids=R.RANDOM_IDS)
def test_input_conditions_of_the_random_cases(c):
    fm, ct, nt = R.random_case(*c)
    r, fig = R.conditioned(fm, ct, nt, f"random {c}")
    print(f"\nformant_track random {c}: S {R.n_states(*c)}, {fm.shape[1]} frames, states used {np.unique(r[1]).size}, least margin {fig['margin']:.3e}, "
          f"float64 against longdouble {fig['cost_spread']:.3e}")
    assert (r[1] >= 0).all() and (ct >= nt).all() and (ct <= c[0]).all()
    assert np.unique(r[1]).size > 1 or R.n_states(*c) == 1, "more than one state is chosen"


@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_input_conditions_of_the_edge_cases(name):
    fm, ct, nt = R.edge_case(name)
    r, fig = R.conditioned(fm, ct, nt, name)
    gaps = R.trackable(fm[0], ct[0], nt) < 0
    assert np.array_equal(r[1][0] < 0, gaps) and not r[0][0][gaps].any() and not r[2][0][gaps].any() and np.isfinite(r[0]).all() and np.isfinite(r[2]).all()
    expect = {"gap_at_frame_0": lambda: gaps[0] and not gaps[1], "gap_at_the_last_frame": lambda: gaps[-1] and not gaps[-2],
              "two_adjacent_gaps": lambda: gaps[9] and gaps[10] and gaps.sum() == 2, "single_frame_segments": lambda: gaps[1::2].all() and not gaps[::2].any(),
              "all_gaps": lambda: gaps.all(), "unconverged_frames": lambda: gaps.sum() == 3, "count_over_n_cand": lambda: not gaps.any() and (ct > 5).sum() >= 2,
              "zero_and_nan_candidates": lambda: gaps.sum() == 3 and gaps[[5, 12, 18]].all() and np.isnan(fm).sum() == 2,
              "one_frame": lambda: fm.shape[1] == 1 and not gaps.any(), "two_frames": lambda: fm.shape[1] == 2 and not gaps.any()}[name]
    assert expect(), name
    ends = ~gaps & np.append(gaps[1:], True)
    assert np.array_equal(r[2][0] != 0, ends), "a cost at every segment's last frame and nowhere else"


# ---- the CLI's flag ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", (["--voice_report", "x.txt", "--track_formants"], ["--evaluate_pairs", "x.txt", "--track_formants"],
                                  ["--prosody_report", "x.txt", "--track_formants"], ["--voice_report", "x.txt", "--perturbation", "--track_formants"]))
def test_track_formants_is_refused_without_its_home(argv):
    from emojivoice_amd import cli

    with pytest.raises(AssertionError, match="--track_formants is an option of --formants and of --harmonics under --voice_report and --evaluate_pairs"):
        cli.cli(argv)


def test_report_families_count_the_tracks_only_when_asked():
    from emojivoice_amd import cli

    plain, tracked = cli.report_families(), cli.report_families(True)
    assert [f[:5] for f in plain] == [f[:5] for f in tracked]
    assert [f.counts for f in plain if f.block == "formants"] == [("unconverged_frames",)]
    assert [f.counts for f in tracked if f.block == "formants"] == [("unconverged_frames", "tracked_frames", "track_segments")]
    assert cli.formant_tracking_parameters()["reference_hz"] == list(audio.FORMANT_TRACK_REFERENCE)
