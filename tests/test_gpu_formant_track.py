"""ev_formant_track on the MI355X, through the C ABI, and what stands on it (Engine.formant_track, audio.formant_tracks).

Yardstick: tests/formant_track_ref.py, the numpy float64 restatement of the definition in include/emojivoice.h.  The inputs are the REFERENCE's
formant and count (formants_ref.batch on speech-like rows, seeded random candidates, damaged rows), so the call stands alone.  The device's
log2 is its own library's, so its costs may differ from the restatement's by float64 rounding.  The rule of every comparison (``check``):
  * first, conditions on the INPUT, not on the device (formant_track_ref.conditioned; measured on the CPU in tests/test_formant_track_host.py):
    the float64 and the longdouble restatements choose EQUAL paths, their costs agree within 1e-11 max(|ref|, 1), and every decision's second
    best lies at least 1e-6 over its best, so no frame is left out of the comparison;
  * d_sel EQUAL everywhere;
  * d_track bit-equal to the input's entries at the chosen candidates: it is a copy;
  * d_cost within 1e-9 max(|ref|, 1): the project's float64 margin (tests/test_gpu_formants.py); the restatements' own spread is under 1e-15;
  * gaps hold exact zeros and -1.
Observed on the MI355X: every d_sel equal and every d_cost EQUAL to the float64 restatement's (the device's log2 gave numpy's bits on every candidate)
over all cases, S = 1 to 792; least margins 5.6e-5 to 2.4e-2, the restatements' own spread at most 8.2e-16.  Every case prints its figures, DESIGN
section 3.25 records them; the gate stays at 1e-9.  Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py), d_back included.
"""
import numpy as np
import pytest
import torch

import analysis_gpu as A
import formant_track_ref as R
import formants_ref as F
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

_REF = {}


def ref_of(key, fm, ct, nt, **kw):
    """(the float64 restatement's (track, sel, cost, choice, margin), the input's figures), computed once per case and never modified; the
    input conditions are asserted on the way."""
    return A.frozen(_REF, key, lambda: R.conditioned(fm, ct, nt, str(key), **kw))


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


def raw(eng, fm, ct, nt, ref=None, cost_f=1.0, cost_b=1.0, cost_j=1.0, B=None, NF=None, nc=None, null=(), back_words=None):
    """ev_formant_track into guarded buffers: (rc, track (B, NF, nt, 2), sel (B, NF), cost (B, NF)) on the host; an argument named in ``null`` is
    passed as NULL (an output comes back None).  ``B`` / ``NF`` / ``nc`` override what is passed to the library; d_back is (B, NF, S) 16-bit
    words between margins too (``back_words``: another size, for calls that must fail before they use it)."""
    fm = np.ascontiguousarray(fm, dtype=np.float64)
    Bx, NFx, ncx, _ = fm.shape
    d_fm = torch.from_numpy(fm).to(DEV)
    d_ct = torch.from_numpy(np.ascontiguousarray(ct, dtype=np.int32)).to(DEV)
    ntx = max(int(nt), 1)
    S = R.n_states(ncx, ntx) if ntx <= ncx else 1
    words = Bx * NFx * S if back_words is None else back_words
    out = A.Guarded({"back": ((2 * words,), torch.uint8), "track": ((Bx, NFx, ntx, 2), torch.float64), "sel": ((Bx, NFx), torch.int32),
                     "cost": ((Bx, NFx), torch.float64)}, null)
    rv = np.ascontiguousarray(R.default_reference(ntx) if ref is None else ref, dtype=np.float64)
    rc = eng.lib.ev_formant_track(eng.h, None if "formant" in null else d_fm.data_ptr(), None if "count" in null else d_ct.data_ptr(),
                                  Bx if B is None else B, NFx if NF is None else NF, ncx if nc is None else nc, int(nt),
                                  None if "ref" in null else rv.ctypes.data, float(cost_f), float(cost_b), float(cost_j), out.ptr("back"),
                                  out.ptr("track"), out.ptr("sel"), out.ptr("cost"), _stream_ptr())
    res = out.collect(rc)
    return rc, res["track"], res["sel"], res["cost"]


def check(dev, fm, ct, nt, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    track, sel, cost = dev
    (rt, rs, rc, _, _), fig = ref
    gaps = rs < 0
    e_c = R.err(cost, rc) if cost is not None else 0.0
    T = R.states(fm.shape[2], nt)
    gathered = np.take_along_axis(np.asarray(fm, dtype=np.float64), T[np.maximum(rs, 0)][..., None].repeat(2, axis=-1), axis=2)
    gathered[gaps] = 0.0
    ends = ~gaps & np.concatenate([gaps[:, 1:], np.ones((gaps.shape[0], 1), bool)], axis=1)
    print(f"\nformant_track {what}: S {len(T)}  frames {rs.shape[1]}  rows {rs.shape[0]}  d_sel differing {int((sel != rs).sum())}  d_cost err {e_c:.3e} "
          f"(gate {R.TOL:g})  restatement float64 against longdouble {fig['cost_spread']:.3e}  least margin {fig['margin']:.3e}  gaps {int(gaps.sum())}  "
          f"segments {int(ends.sum())}  states used {np.unique(rs[~gaps]).size}")
    assert np.array_equal(sel, rs), f"{what}: d_sel"
    assert np.array_equal(track.view(np.uint64), gathered.view(np.uint64)) and np.array_equal(gathered, rt), f"{what}: d_track is a copy of the chosen entries"
    assert not track[gaps].any() and (sel[gaps] == -1).all(), f"{what}: exact zeros and -1 on gaps"
    assert np.isfinite(track).all()
    if cost is not None:
        assert e_c <= R.TOL, f"{what}: d_cost"
        assert np.isfinite(cost).all() and not cost[~ends].any() and (cost[ends] > 0).all(), f"{what}: a cost at every segment's last frame, 0 elsewhere"


# ---- 1. speech-like rows: ev_formants' restatement as the input -----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SPEECH_CASES)), ids=R.SPEECH_IDS)
def test_speech_rows_against_the_restatement(eng, i):
    """Three ragged rows each: the frames past a row's end have count 0 and are gaps."""
    fm, ct, nt = R.speech_case(i)
    ref = ref_of(("speech", i), fm, ct, nt)
    rc, *dev = raw(eng, fm, ct, nt)
    assert rc == 0, err_of(eng)
    check(dev, fm, ct, nt, ref, f"speech {R.SPEECH_IDS[i]}")
    tracked = (dev[1] >= 0).sum(axis=1)
    assert (tracked > fm.shape[1] // 2).all() and len(set(tracked.tolist())) == 3, "ragged rows, mostly trackable"


# ---- 2. every lane layout: S = 1, 3, 10 (4 lanes a state), 70 (past one wave), 560, 792 (past 512 threads) --------------------------------------
@pytest.mark.parametrize("c", R.RANDOM_CASES, ids=R.RANDOM_IDS)
def test_random_candidates_against_the_restatement(eng, c):
    fm, ct, nt = R.random_case(*c)
    ref = ref_of(("random", c), fm, ct, nt)
    rc, *dev = raw(eng, fm, ct, nt)
    assert rc == 0, err_of(eng)
    check(dev, fm, ct, nt, ref, f"random {c}")


def test_other_costs_and_another_reference(eng):
    """Every cost and the reference reach the kernel: each setting is held to the restatement under the same setting, and moves the path."""
    fm, ct, nt = R.random_case(5, 3)
    base = ref_of(("random", (5, 3)), fm, ct, nt)[0][1]
    for i, kw in enumerate((dict(cost_f=0.0), dict(cost_b=0.0), dict(cost_j=0.0), dict(cost_f=0.25, cost_b=2.0, cost_j=3.5), dict(ref=(400.0, 2100.0, 3300.0)))):
        ref = ref_of(("costs", i), fm, ct, nt, **kw)
        rc, *dev = raw(eng, fm, ct, nt, **kw)
        assert rc == 0, err_of(eng)
        check(dev, fm, ct, nt, ref, f"costs {kw}")
        assert not np.array_equal(dev[1], base), f"{kw} moves the path"


# ---- 3. gaps, segments, damaged frames, NF = 1 and 2 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_gaps_and_segments(eng, name):
    fm, ct, nt = R.edge_case(name)
    ref = ref_of(("edge", name), fm, ct, nt)
    rc, *dev = raw(eng, fm, ct, nt)
    assert rc == 0, err_of(eng)
    check(dev, fm, ct, nt, ref, name)
    gaps = R.trackable(fm[0], ct[0], nt) < 0
    assert np.array_equal(dev[1][0] < 0, gaps)
    if name == "all_gaps":
        assert gaps.all() and not dev[0].any() and not dev[2].any() and (dev[1] == -1).all()
    if name == "zero_and_nan_candidates":
        assert gaps.sum() == 3 and np.isnan(fm).sum() == 2 and np.isfinite(dev[0]).all() and np.isfinite(dev[2]).all()


def test_cost_null(eng):
    fm, ct, nt = R.random_case(5, 3)
    ref = ref_of(("random", (5, 3)), fm, ct, nt)
    rc, track, sel, cost = raw(eng, fm, ct, nt, null=("cost",))
    assert rc == 0 and cost is None, err_of(eng)
    check((track, sel, None), fm, ct, nt, ref, "d_cost = NULL")


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("speech-5-3", "random-8-4"))
def test_row_alone_in_a_batch_padded_again_and_under_every_arithmetic_give_the_same_bits(eng, which):
    if which == "speech-5-3":
        fm, ct, nt = R.speech_case(2)
    else:
        fm, ct = R.random_candidates(3, 40, 8, 4, seed=9)
        nt = 4
    n0 = eng.alloc_count()
    rc, *alone = raw(eng, fm[1:2], ct[1:2], nt)
    assert rc == 0, err_of(eng)
    rc, *again = raw(eng, fm[1:2], ct[1:2], nt)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    rc, *batch = raw(eng, fm, ct, nt)
    assert rc == 0
    NF = fm.shape[1]
    pad_fm = np.concatenate([fm[[2, 1]], np.full((2, 7, fm.shape[2], 2), 321.0)], axis=1)       # gap frames behind: count 0, entries that are not zeros
    pad_ct = np.concatenate([ct[[2, 1]], np.zeros((2, 7), np.int32)], axis=1)
    pad_ct[:, NF + 3] = -1
    rc, *padded = raw(eng, pad_fm, pad_ct, nt)
    assert rc == 0
    assert (alone[1] >= 0).sum() > NF // 2
    for i, out in enumerate(("d_track", "d_sel", "d_cost")):
        assert np.array_equal(alone[i][0], batch[i][1]), f"{out}: alone against inside a batch"
        assert np.array_equal(alone[i][0], padded[i][1, :NF]), f"{out}: alone against a larger NF"
        assert (padded[i][:, NF:] == (-1 if i == 1 else 0)).all(), f"{out}: the gap frames behind"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (16, 6, 0):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, fm, ct, nt)
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0, "ev_alloc_count never moves"


def test_no_allocation_and_capturable():
    e = Engine(0)
    fm, ct, nt = R.speech_case(2)
    d_fm, d_ct = torch.from_numpy(fm).to(DEV), torch.from_numpy(ct).to(DEV)
    n0 = e.alloc_count()
    ref = e.formant_track(d_fm, d_ct, nt, R.REFERENCE)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        e.formant_track(d_fm, d_ct, nt, R.REFERENCE)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = e.formant_track(d_fm, d_ct, nt, R.REFERENCE)
        for t in out:
            t.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b), "the replay equals the eager call"
    r64 = ref_of(("speech", 2), fm, ct, nt)[0]
    assert np.array_equal(out[1].cpu().numpy(), r64[1]) and np.array_equal(out[0].cpu().numpy(), r64[0])
    assert e.alloc_count() == n0
    e.close()


# ---- 5. limits ------------------------------------------------------------------------------------------------------------------------------------
BAD_CALL = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("NF=", dict(NF=0)), ("n_cand=", dict(nc=0)), ("n_cand=", dict(nc=17)), ("n_tracks=", dict(nt=0)),
    ("n_tracks=", dict(nt=6)), ("ref[1]", dict(ref=(550.0, 0.0, 2750.0))), ("ref[2]", dict(ref=(550.0, 1650.0, float("nan")))),
    ("ref[0]", dict(ref=(float("inf"), 1650.0, 2750.0))), ("ref[0]", dict(ref=(-550.0, 1650.0, 2750.0))),
    ("cost_f=", dict(cost_f=-1.0)), ("cost_f=", dict(cost_f=float("nan"))), ("cost_b=", dict(cost_b=float("inf"))), ("cost_b=", dict(cost_b=-0.5)),
    ("cost_j=", dict(cost_j=float("nan"))), ("cost_j=", dict(cost_j=-2.0)),
    ("ref", dict(null=("ref",))), ("d_formant", dict(null=("formant",))), ("d_count", dict(null=("count",))), ("d_back", dict(null=("back",))),
    ("d_track", dict(null=("track",))), ("d_sel", dict(null=("sel",))),
]


@pytest.mark.parametrize("word,kw", BAD_CALL, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_fails_with_a_message_naming_it(eng, word, kw):
    fm, ct = R.random_candidates(2, 6, 5, 3, seed=3)
    kw = dict(kw)
    rc, *_ = raw(eng, fm, ct, kw.pop("nt", 3), **kw)                      # (a failed call writes nothing: raw checks that)
    msg = err_of(eng)
    assert rc != 0 and "ev_formant_track" in msg and word in msg, msg


def test_too_many_states_fail_with_a_message_naming_s(eng):
    fm, ct = R.random_candidates(1, 4, 16, 8, seed=4)
    rc, *_ = raw(eng, fm, ct, 8, back_words=64)
    msg = err_of(eng)
    assert rc != 0 and "S=12870" in msg and "1024" in msg, msg
    fm, ct = R.random_candidates(1, 4, 13, 4, seed=4)                       # C(13, 4) = 715 passes, C(13, 5) = 1287 does not
    rc, *dev = raw(eng, fm, ct, 4)
    assert rc == 0, err_of(eng)
    rc, *_ = raw(eng, fm, ct, 5, back_words=64)
    assert rc != 0 and "S=1287" in err_of(eng)


# ---- 6. audio.formants -> audio.formant_tracks ---------------------------------------------------------------------------------------------------
def test_audio_formant_tracks_end_to_end():
    lens = [4000, 2600, 700]
    sig = [F.speech_like(n, seed=18 * i, fs=22050) for i, n in enumerate(lens)]
    x, _, _ = F.padded([(s, s) for s in sig])
    xd = torch.from_numpy(x).to(DEV)
    fm = audio.formants(xd, lengths=lens, n_formants=5)
    tk = audio.formant_tracks(fm)
    B, NF = fm["count"].shape
    assert tk["frequency"].shape == tk["bandwidth"].shape == (B, NF, 3) and tk["frequency"].dtype == torch.float64
    assert tk["selection"].shape == (B, NF, 3) and tk["count"].shape == tk["cost"].shape == (B, NF) and tk["count"].dtype == torch.int32 and tk["segments"].shape == (B,)
    cand = np.stack([fm["frequency"].cpu().numpy(), fm["bandwidth"].cpu().numpy()], axis=-1)
    ct = fm["count"].cpu().numpy()
    (rt, rs, rc, rch, _), fig = ref_of("audio", cand, ct, 3)
    print(f"\nformant_track audio.formant_tracks 4000 / 2600 / 700 samples: tracked {(rs >= 0).sum(axis=1).tolist()} of {NF} frames, least margin "
          f"{fig['margin']:.3e}, cost err {R.err(tk['cost'].cpu().numpy(), rc):.3e}")
    assert np.array_equal(tk["selection"].cpu().numpy(), rch) and np.array_equal(tk["frequency"].cpu().numpy(), rt[..., 0])
    assert np.array_equal(tk["bandwidth"].cpu().numpy(), rt[..., 1]) and R.err(tk["cost"].cpu().numpy(), rc) <= R.TOL
    gaps = rs < 0
    assert np.array_equal(tk["count"].cpu().numpy(), np.where(gaps, np.where(ct < 0, -1, 0), 3))
    ends = ~gaps & np.concatenate([gaps[:, 1:], np.ones((B, 1), bool)], axis=1)
    assert tk["segments"].cpu().tolist() == ends.sum(axis=1).tolist() and (rs >= 0).sum() > NF
    one = audio.formant_tracks({k: v[1] for k, v in fm.items()})
    assert one["frequency"].shape == (1, NF, 3) and all(torch.equal(one[k][0], tk[k][1]) for k in tk), "a single row is the same row"
    pitch = audio.pitch_yin(xd, lengths=lens)
    fl = [F.frames(n, 256) for n in lens]
    st = audio.formant_statistics(tk, pitch["voiced"], lengths=fl)
    use = pitch["voiced"].cpu().numpy() & ~gaps & (np.arange(NF)[None, :] < np.array(fl)[:, None])
    assert st["frames"].cpu().tolist() == use.sum(axis=1).tolist() and use[0].sum() > 3
    ok = use & (rt[..., 0, 1] <= 700.0)
    assert abs(float(st["f1_hz"][0]) - rt[0, :, 0, 0][ok[0]].mean()) <= 1e-9 * rt[0, :, 0, 0][ok[0]].mean()
    hm = audio.harmonics(xd, lengths=lens, formants=tk)
    hs = audio.harmonic_statistics(hm, pitch["voiced"], lengths=fl, fm=tk)
    assert hm["h1_a3_db"].shape == (B, NF) and torch.isfinite(hm["h1_a3_db"]).all() and hs["frames"].shape == (B,)
    with pytest.raises(ValueError, match="n_tracks=6"):
        audio.formant_tracks(fm, n_tracks=6, reference=R.default_reference(6))


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------------------
def _wavs(tmp_path, short):
    from emojivoice_amd import cli

    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    for i, name in enumerate(names):
        cli.write_wav_pcm16(tmp_path / name, F.speech_like((16000, 19000, short)[i], seed=20 + i, fs=22050), 22050)
    return cli, names


TRACK_KEYS = {"tracked_frames", "track_segments"}


def test_voice_report_with_tracked_formants(tmp_path):
    cli, names = _wavs(tmp_path, 300)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{tmp_path / name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    base = ["--voice_report", str(flist), "--batch_size", "2", "--formants", "--harmonics", "--functionals"]
    plain = cli.cli(base)
    rep = cli.cli(base + ["--track_formants"])
    assert "formant_tracking" not in plain and not TRACK_KEYS & set(plain["files"][0]) and not TRACK_KEYS & set(plain["overall"])
    assert rep["formant_tracking"] == {"candidates": 5, "tracks": 3, "reference_hz": [550.0, 1650.0, 2750.0], "frequency_cost": 1.0, "bandwidth_cost": 1.0,
                                       "transition_cost": 1.0}
    assert set(rep) - {"formant_tracking"} == set(plain)
    assert [set(f_) - TRACK_KEYS for f_ in rep["files"]] == [set(f_) for f_ in plain["files"]] and all(TRACK_KEYS <= set(f_) for f_ in rep["files"])
    assert set(rep["overall"]) - TRACK_KEYS == set(plain["overall"]) and set(rep["files"][0]["functionals"]) == set(plain["files"][0]["functionals"])
    a, b, c = rep["files"]
    print(f"\nformant_track --voice_report --track_formants: {[[f_[k] for k in ('formant_frames', 'tracked_frames', 'track_segments') + audio.FORMANT_FIGURES] for f_ in rep['files']]}"
          f"\n  lowest three: {[[f_[k] for k in ('formant_frames',) + audio.FORMANT_FIGURES] for f_ in plain['files']]}")
    assert a["tracked_frames"] >= a["formant_frames"] > 5 and a["track_segments"] >= 1 and 150.0 < a["f1_hz"] < a["f2_hz"] < a["f3_hz"] < 5500.0
    assert rep["overall"]["tracked_frames"] == sum(f_["tracked_frames"] for f_ in rep["files"])
    assert rep["speakers"]["7"]["track_segments"] == a["track_segments"] + b["track_segments"]
    assert all(isinstance(a[k], float) and np.isfinite(a[k]) for k in audio.FORMANT_FIGURES + audio.HARMONIC_FIGURES)
    assert [f_[k] for f_ in rep["files"] for k in audio.VOICE_QUALITY_FIGURES] == [f_[k] for f_ in plain["files"] for k in audio.VOICE_QUALITY_FIGURES]
    with pytest.raises(AssertionError, match="--track_formants is an option of --formants"):
        cli.cli(["--voice_report", str(flist), "--track_formants"])


def test_evaluate_pairs_with_tracked_formants(tmp_path):
    cli, names = _wavs(tmp_path, 600)
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(f"{tmp_path / 'a.wav'}|{tmp_path / 'b.wav'}|7\n{tmp_path / 'b.wav'}|{tmp_path / 'a.wav'}|7\n", encoding="utf-8")
    plain = cli.cli(["--evaluate_pairs", str(pairs), "--formants"])
    rep = cli.cli(["--evaluate_pairs", str(pairs), "--formants", "--track_formants"])
    assert set(rep) - {"formant_tracking"} == set(plain) and rep["formant_tracking"]["tracks"] == 3
    assert [set(p) for p in rep["pairs"]] == [set(p) for p in plain["pairs"]]
    p0, p1 = rep["pairs"]
    for k in audio.FORMANT_FIGURES:
        assert isinstance(p0["formants"]["recorded"][k], float) and abs(p0["formants"]["delta"][k] + p1["formants"]["delta"][k]) < 1e-9
    assert p0["mcd_db"] == plain["pairs"][0]["mcd_db"], "nothing but the formants moves"
