"""ev_perturbation on the MI355X, through the C ABI, and what stands on it (audio.perturbation, audio.perturbation_statistics, --voice_report
--perturbation, --evaluate_pairs --perturbation).

Yardstick: tests/perturbation_ref.py, the numpy restatement of the definition in include/emojivoice.h, in float64 and in longdouble.  The rule of
every comparison (``check``):
  * first, conditions on the INPUT, computed from the restatements alone: float64 and longdouble agree on every mark, count and parabola branch;
    every counted or excluded pair keeps a relative margin of 1e-6 from its factor threshold; |E0 E1 - floor^2| >= 1e-6 floor^2.  No frame is left
    out of the comparison (tests/test_perturbation_host.py checks the same on the CPU);
  * d_marks and d_count EQUAL;
  * every entry of d_frame within 1e-9 max(|ref|, 1): the project's float64 margin.
Observed on the MI355X: every mark and count equal, d_frame 3.3e-16 at worst over all cases (the restatement adds in the device's order, so what
remains is the device library's log10 in the shimmer in dB).  Every case prints its worst figure; DESIGN section 3.21 records them.  Every raw call writes into buffers with 64-element sentinel margins (tests/analysis_gpu.py); 50.0 lies
behind every row's length.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import perturbation_ref as R
import pitch_ref
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

_REF, _CASES = {}, {}


def case(name):
    if not _CASES:
        _CASES.update(R.cases())
    return _CASES[name]


def ref_of(key, x, lens, lag, g):
    """The restatements' results (float64, longdouble), computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: (R.batch(x, lens, lag, g), R.batch(x, lens, lag, g, dtype=np.longdouble)))


def raw(eng, g, x, lens, lag, B=None, L=None, null=(), **kw):
    """ev_perturbation into guarded buffers: (rc, frame (B, F, 8), count (B, F, 4), marks (B, F, 2 nc + 1)) on the host; an argument named in
    ``null`` is passed as NULL (an output then comes back None).  ``B`` / ``L`` override the shape passed to the library, ``kw`` one argument of
    the geometry (H, W, nc, pf, af, floor)."""
    a = g._asdict()
    a.update(kw)
    x = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    F = R.frames(Lx, g.H)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    d_lag = torch.as_tensor(np.asarray(lag, dtype=np.int32).reshape(Bx, F)).to(DEV).contiguous()
    out = A.Guarded({"frame": ((Bx, F, 8), torch.float64), "count": ((Bx, F, 4), torch.int32), "marks": ((Bx, F, 2 * g.nc + 1), torch.int32)}, null)
    rc = eng.lib.ev_perturbation(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, a["H"],
                                 None if "lag" in null else d_lag.data_ptr(), a["nc"], a["W"], float(a["pf"]), float(a["af"]), float(a["floor"]),
                                 out.ptr("frame"), out.ptr("count"), out.ptr("marks"), _stream_ptr())
    return (rc, *out.collect(rc).values())


NAMES = ("jitter", "jitter_abs", "shimmer", "shimmer_db", "r", "Tmean", "Amean", "rap")


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    fr, ct, mk = dev
    r64, rld = ref
    R.input_conditions(r64, rld, what)
    errs = [R.err(fr[..., i], r64["frame"][..., i]) for i in range(8)]
    voiced = int((r64["branch"][..., -1] >= 0).sum())
    print(f"\nperturbation {what}: worst d_frame err {max(errs):.3e} ({', '.join(f'{n} {e:.1e}' for n, e in zip(NAMES, errs))}; gate {R.TOL:g})  "
          f"float64 against longdouble {R.err(r64['frame'], rld['frame'].astype(np.float64)):.3e}  marks differing {int((mk != r64['marks']).sum()) if mk is not None else 0}  "
          f"counts differing {int((ct != r64['count']).sum())}  voiced frames {voiced} of {ct.shape[0] * ct.shape[1]}  periods {int(r64['count'][..., 0].sum())}  "
          f"least pair margin {r64['pair_margin']:.2e}  least floor margin {r64['floor_margin']:.2e}  ties {r64['ties']}")
    if mk is not None:
        assert np.array_equal(mk, r64["marks"]), f"{what}: d_marks"
    assert np.array_equal(ct, r64["count"]), f"{what}: d_count"
    assert np.isfinite(fr).all() and max(errs) <= R.TOL, f"{what}: d_frame"
    off = r64["branch"][..., -1] < 0
    assert not fr[off].any() and not ct[off].any() and (mk is None or (mk[off] == -1).all()), f"{what}: exact zeros and -1 on unvoiced and empty frames"


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


def run_case(eng, name):
    x, lens, lag, g = case(name)
    rc, *dev = raw(eng, g, x, lens, lag)
    assert rc == 0, err_of(eng)
    ref = ref_of(name, x, lens, lag, g)
    check(dev, ref, f"{name} {tuple(g)[:3]} lens {lens}")
    return x, lens, lag, g, dev, ref


# ---- 1. the small geometries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small-nc1", "small-nc3", "small-nc16", "corr70", "corr8"))
def test_small_geometry_against_the_restatement(eng, name):
    """Four frames to a workgroup: the rows' frame counts leave 3, 0 and 1.  corr_length 70 is no multiple of 64 (6 lanes add two terms, 58 one), 8
    leaves 56 lanes without a term.  The lags are the restatement of YIN's at tau_min = 16."""
    x, lens, lag, g, (fr, ct, mk), _ = run_case(eng, name)
    nfs = [R.frames(n, g.H) for n in lens]
    assert [n % 4 for n in nfs] == [3, 0, 1] and x.shape[1] <= 2600
    for b in range(3):
        assert not fr[b, nfs[b]:].any() and not ct[b, nfs[b]:].any() and (mk[b, nfs[b]:] == -1).all(), "zeros and -1 past the row's own frames"
        # (16 cycles each side span 1300 to 1600 of a row's 2500 samples: only the frames in the middle can have them all)
        assert (ct[b, :nfs[b], 0] == 2 * g.nc).sum() > (nfs[b] // 3 if g.nc <= 3 else 8), "the chains run their full length on many frames"
    k = ct[..., 1] > 0
    print(f"perturbation {name}: median local jitter {100 * np.median(fr[..., 0][k]):.3f} %, shimmer {100 * np.median(fr[..., 2][ct[..., 2] > 0]):.3f} %, "
          f"HNR {np.median(R.hnr_db(fr[..., 4][ct[..., 0] > 0])):.1f} dB")


# ---- 2. hand-made lags, degenerate rows ----------------------------------------------------------------------------------------------------------
def test_hand_made_lags_and_degenerate_rows(eng):
    x, lens, lag, g, (fr, ct, mk), _ = run_case(eng, "hand")
    F = lag.shape[1]
    for f in range(F):
        if not 16 <= R.HAND_LAGS[f % len(R.HAND_LAGS)] <= 2048:           # 0, 15, 2049, -3, 10^9: unvoiced
            assert not fr[0, f].any() and not ct[0, f].any() and (mk[0, f] == -1).all(), f"lag {lag[0, f]} must read as unvoiced"
    by_lag = {t: [int(ct[0, f, 0]) for f in range(F) if lag[0, f] == t] for t in (16, 20, 39, 40, 41, 80, 2048)}
    print(f"perturbation hand-made lags: periods found per frame, by lag (the true period is 40): {by_lag}")
    assert sum(k == 6 for k in by_lag[40]) > len(by_lag[40]) // 2, "the true period finds all six periods on most frames"
    assert not fr[1].any() and not ct[1].any() and (mk[1] == -1).all(), "a zero row: no marks, r = 0"
    mid = slice(900 // 64 + 3, 1700 // 64 - 3)
    assert not ct[2, mid].any() and (mk[2, mid] == -1).all() and not fr[2, mid].any() and (ct[2, :8, 0] > 0).any(), "the silent middle"
    assert (mk[3] == -1).all() and not ct[3].any(), "a row of one sample has no marks"
    for b in (4, 5):
        assert not fr[b].any() and not ct[b].any() and (mk[b] == -1).all(), "len 0 and len > L: rows of zeros"
    assert (ct[6, 4:-4, 0] == 6).sum() > F // 2, "the good row beside them"


def test_a_row_of_one_sample_alone(eng):
    g = R.geo()
    x = np.full((1, 1), 0.5, np.float32)
    lag = np.full((1, 1), 40, np.int32)
    rc, *dev = raw(eng, g, x, None, lag)
    assert rc == 0, err_of(eng)
    check(dev, ref_of("one", x, None, lag, g), "a (1, 1) row")
    assert dev[1].shape == (1, 1, 4) and not dev[1].any() and (dev[2] == -1).all()


# ---- 3. the edges and the tie rule -----------------------------------------------------------------------------------------------------------------
def test_chains_stop_at_the_silence_and_zeros_lie_outside_the_row(eng):
    x, lens, lag, g, (fr, ct, mk), (r64, _) = run_case(eng, "edges")
    for b, n in enumerate(lens):
        m = mk[b][mk[b] >= 0]
        assert m.size and ((m < 200) | (m >= n - 200)).all(), "no mark inside the silence"
        assert (m < 64).any() and (m >= n - 64).any(), "marks within the first and the last frame of the row"
        nf = R.frames(n, g.H)
        assert (ct[b, :nf, 0] < 2 * g.nc).any() and ct[b, 8: nf - 8].sum() == 0


def test_ties_go_to_the_lowest_index(eng):
    x, lens, lag, g, (fr, ct, mk), (r64, _) = run_case(eng, "plateau")
    other = R.batch(x, lens, lag, g, mutant="ties_highest")
    differ = int((other["marks"] != r64["marks"]).any(axis=-1).sum())
    print(f"perturbation plateau: the restatement meets {r64['ties']} searches with equal maxima; 'ties to the highest index' changes the marks of {differ} frames")
    assert r64["ties"] >= 1 and differ >= 1


# ---- 4. the identities -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small-nc3", "small-nc16", "corr70"))
def test_row_alone_in_a_batch_as_a_prefix_without_marks_twice_and_under_every_arithmetic_give_the_same_bits(eng, name):
    x, lens, lag, g = case(name)
    n = lens[0]
    nf = R.frames(n, g.H)
    c = x[0, :n].copy()
    n0 = eng.alloc_count()
    rc, *alone = raw(eng, g, c[None], None, lag[:1, :nf])
    assert rc == 0, err_of(eng)
    rc, *again = raw(eng, g, c[None], None, lag[:1, :nf])
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    rc, f2, c2, none = raw(eng, g, c[None], None, lag[:1, :nf], null=("marks",))
    assert rc == 0 and none is None and np.array_equal(f2, alone[0]) and np.array_equal(c2, alone[1]), "d_marks = NULL"
    xb, lb = R.padded([x[2, :lens[2]], c, x[1, :lens[1]]])
    rc, *batch = raw(eng, g, xb, lb, lag[[2, 0, 1]])
    assert rc == 0
    Lp = n + 1235
    xp, lp = R.padded([x[1, :lens[1]], c], L=Lp)
    xp[1, n:] = -7.5e3                                                   # other garbage than in the batch of three
    Fp = R.frames(Lp, g.H)
    lagp = np.full((2, Fp), 33, np.int32)                                # (a voiced lag behind the row's own frames must not matter)
    lagp[0, :lag.shape[1]], lagp[1, :nf] = lag[1], lag[0, :nf]
    rc, *prefix = raw(eng, g, xp, lp, lagp)
    assert rc == 0
    assert (alone[1][0, :, 0] > 0).any()
    for what, other in (("inside a batch", batch), ("the prefix of a padded row", prefix)):
        for i, out in enumerate(("d_frame", "d_count", "d_marks")):
            assert np.array_equal(alone[i][0, :nf], other[i][1, :nf]), f"{out}: alone against {what}"
            assert not other[i][1, nf:].any() if i < 2 else (other[i][1, nf:] == -1).all(), f"{out}: past the row's frames, {what}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 3, 6):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, g, xb, lb, lag[[2, 0, 1]])
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0, "ev_alloc_count never moves"


def test_no_allocation_and_capturable():
    e = Engine(0)
    x, lens, lag, g = case("small-nc3")
    xd = torch.from_numpy(x).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    lg = torch.from_numpy(np.ascontiguousarray(lag, dtype=np.int32)).to(DEV)
    n0 = e.alloc_count()
    ref = e.perturbation(xd, ld, lg, g.H, g.nc, g.W, g.pf, g.af, g.floor)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        e.perturbation(xd, ld, lg, g.H, g.nc, g.W, g.pf, g.af, g.floor)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = e.perturbation(xd, ld, lg, g.H, g.nc, g.W, g.pf, g.af, g.floor)
        for t in out:
            t.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b), "the replay equals the eager call"
    r64 = ref_of("small-nc3", x, lens, lag, g)[0]
    assert np.array_equal(out[2].cpu().numpy(), r64["marks"]) and np.array_equal(out[1].cpu().numpy(), r64["count"])
    assert e.alloc_count() == n0
    e.close()


# ---- 5. limits -----------------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
BAD_CALL = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)), ("hop_length=", dict(H=0)), ("hop_length=", dict(H=4097)),
    ("n_cycles=", dict(nc=0)), ("n_cycles=", dict(nc=17)), ("corr_length=", dict(W=7)), ("corr_length=", dict(W=4097)),
    ("period_factor=", dict(pf=1.0)), ("period_factor=", dict(pf=INF)), ("period_factor=", dict(pf=NAN)),
    ("amplitude_factor=", dict(af=0.5)), ("amplitude_factor=", dict(af=INF)), ("amplitude_factor=", dict(af=NAN)),
    ("power_floor=", dict(floor=0.0)), ("power_floor=", dict(floor=-1e-7)), ("power_floor=", dict(floor=INF)), ("power_floor=", dict(floor=NAN)),
    ("d_x", dict(null=("x",))), ("d_lag", dict(null=("lag",))), ("d_frame", dict(null=("frame",))), ("d_count", dict(null=("count",))),
]


@pytest.mark.parametrize("word,kw", BAD_CALL, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_fails_with_a_message_naming_it_and_writes_nothing(eng, word, kw):
    g = R.geo()
    z = np.zeros((2, 256), np.float32)
    rc, *_ = raw(eng, g, z, None, np.full((2, 4), 40, np.int32), **kw)    # (a failed call writes nothing: raw checks that)
    msg = err_of(eng)
    assert rc != 0 and "ev_perturbation" in msg and word in msg, msg


# ---- 6. audio.perturbation ---------------------------------------------------------------------------------------------------------------------------
def test_audio_perturbation_on_three_ragged_rows():
    """H 256, corr_length 1024, n_cycles 3 at 22050 Hz on 4000 / 2600 / 700 samples, at the device's own ev_pitch_yin lags, which must equal the
    restatement's."""
    x, lens = R.audio_rows()
    g = R.AUDIO_GEO
    xd = torch.from_numpy(x).to(DEV)
    eng = audio._trim_engine(xd.device)
    out = audio.perturbation(xd, lengths=lens)
    n0 = eng.alloc_count()
    out2 = audio.perturbation(xd, lengths=lens)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0, "no allocation"
    F = R.frames(x.shape[1], 256)
    assert out["jitter"].shape == (3, F) and out["jitter"].dtype == torch.float64 and out["count"].shape == (3, F, 4) and out["marks"].shape == (3, F, 7)
    assert out["count"].dtype == out["marks"].dtype == out["lag"].dtype == torch.int32
    assert all(torch.equal(out[k], out2[k]) for k in out)
    lag = pitch_ref.pitch_yin(x, lens, **pitch_ref.STD)["lag"]
    assert np.array_equal(out["lag"].cpu().numpy(), lag), "ev_pitch_yin's lags equal the restatement's"
    ref = ref_of("audio", x, lens, lag, g)
    fr = np.stack([out[k].cpu().numpy() for k in audio._PERTURBATION_FRAME], axis=-1)
    check((fr, out["count"].cpu().numpy(), out["marks"].cpu().numpy()), ref, "audio.perturbation 4000 / 2600 / 700 samples at 22050 Hz")
    given = audio.perturbation(xd, lengths=lens, lag=out["lag"])
    assert all(torch.equal(out[k], given[k]) for k in out), "the lags given are the lags found"
    fl = [R.frames(n, 256) for n in lens]
    voiced = out["lag"] > 0
    st = audio.perturbation_statistics(out, voiced, lengths=fl)
    v, ct = voiced.cpu().numpy() & (np.arange(F)[None, :] < np.array(fl)[:, None]), out["count"].cpu().numpy()
    assert st["frames"].cpu().tolist() == v.sum(axis=1).tolist() and v[0].sum() > 3
    for name, val, ok in (("jitter_pct", 100 * fr[..., 0], ct[..., 1] > 0), ("rap_pct", 100 * fr[..., 7], ct[..., 3] > 0),
                          ("shimmer_pct", 100 * fr[..., 2], ct[..., 2] > 0), ("shimmer_db", fr[..., 3], ct[..., 2] > 0),
                          ("hnr_db", R.hnr_db(fr[..., 4]), np.ones_like(v))):
        for b in range(3):
            sel = v[b] & ok[b]
            got = float(st[name][b])
            assert int(st["used"][name][b]) == sel.sum()
            assert (np.isnan(got) and not sel.any()) or abs(got - val[b][sel].mean()) <= 1e-12 * max(1.0, abs(val[b][sel].mean())), (name, b)
    one = audio.perturbation(xd[0, :lens[0]])
    nf = fl[0]
    assert one["jitter"].shape == (1, nf) and torch.equal(one["count"][0], out["count"][0, :nf]) and torch.equal(one["r"][0], out["r"][0, :nf]), \
        "a 1-D input is the same row"
    print(f"perturbation, pulse rows: {[{k: round(float(st[k][b]), 3) for k in audio.PERTURBATION_FIGURES} for b in range(3)]}")


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------------------------
def _wavs(tmp_path):
    from emojivoice_amd import cli

    sr = 22050
    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    sig = [R.perturbed_pulses(16000, 120.0, 0.01, 0.05, seed=20), R.perturbed_pulses(19000, 150.0, 0.02, 0.1, seed=21, noise=0.01),
           (0.01 * np.random.default_rng(22).standard_normal(3000)).astype(np.float32)]      # (noise alone: no voiced frame)
    for name, y in zip(names, sig):
        cli.write_wav_pcm16(tmp_path / name, y, sr)
    return cli, names


PERT_KEYS = set(audio.PERTURBATION_FIGURES) | {"perturbation_frames"}


def test_voice_report_with_perturbation(tmp_path):
    cli, names = _wavs(tmp_path)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{tmp_path / name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    plain = cli.cli(["--voice_report", str(flist), "--batch_size", "2"])
    rep = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--perturbation"])
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert PERT_KEYS == {"jitter_pct", "rap_pct", "shimmer_pct", "shimmer_db", "hnr_db", "perturbation_frames"}
    assert [set(f_) - PERT_KEYS for f_ in saved["files"]] == [set(f_) for f_ in plain["files"]] and not PERT_KEYS & set(plain["files"][0])
    assert set(saved["overall"]) - PERT_KEYS == set(plain["overall"]) and not PERT_KEYS & set(plain["overall"])
    assert all(PERT_KEYS <= set(f_) for f_ in saved["files"]) and PERT_KEYS <= set(saved["overall"]) and PERT_KEYS <= set(saved["speakers"]["7"])
    a, b, c = saved["files"]
    print(f"\nperturbation --voice_report --perturbation: {[[f_[k] for k in ('perturbation_frames',) + audio.PERTURBATION_FIGURES] for f_ in saved['files']]}")
    assert a["perturbation_frames"] > 5 and b["perturbation_frames"] > 5 and c["perturbation_frames"] == 0 and all(c[k] is None for k in audio.PERTURBATION_FIGURES)
    assert all(isinstance(f_[k], float) and np.isfinite(f_[k]) for f_ in (a, b) for k in audio.PERTURBATION_FIGURES)
    assert 0.2 < a["jitter_pct"] < b["jitter_pct"] < 6.0 and 1.0 < a["shimmer_pct"] < b["shimmer_pct"] < 30.0 and a["hnr_db"] > b["hnr_db"]
    s7 = saved["speakers"]["7"]
    assert s7["perturbation_frames"] == a["perturbation_frames"] + b["perturbation_frames"] == saved["overall"]["perturbation_frames"]
    lo, hi = min(a["jitter_pct"], b["jitter_pct"]), max(a["jitter_pct"], b["jitter_pct"])
    assert lo - 1e-9 <= s7["jitter_pct"] <= hi + 1e-9 and saved["overall"]["jitter_pct"] == s7["jitter_pct"] and saved["speakers"]["12"]["jitter_pct"] is None


def test_evaluate_pairs_with_perturbation(tmp_path):
    cli, names = _wavs(tmp_path)
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(f"{tmp_path / 'a.wav'}|{tmp_path / 'b.wav'}|7\n{tmp_path / 'b.wav'}|{tmp_path / 'a.wav'}|7\n{tmp_path / 'a.wav'}|{tmp_path / 'c.wav'}|12\n",
                     encoding="utf-8")
    plain = cli.cli(["--evaluate_pairs", str(pairs)])
    rep = cli.cli(["--evaluate_pairs", str(pairs), "--perturbation"])
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    figs = set(audio.PERTURBATION_FIGURES)
    assert all("perturbation" not in p for p in plain["pairs"]) and "perturbation" not in plain["overall"]
    assert [set(p) - {"perturbation"} for p in saved["pairs"]] == [set(p) for p in plain["pairs"]], "without the flag the key sets are the old ones"
    assert set(saved["overall"]) - {"perturbation"} == set(plain["overall"]) and set(saved) == set(plain)
    p0, p1, p2 = saved["pairs"]
    for p in saved["pairs"]:
        assert set(p["perturbation"]) == {"recorded", "synthesised", "delta"} and all(set(p["perturbation"][k]) == figs for k in p["perturbation"])
    for k in figs:
        assert abs(p0["perturbation"]["delta"][k] - (p0["perturbation"]["synthesised"][k] - p0["perturbation"]["recorded"][k])) < 1e-9
        assert abs(p0["perturbation"]["delta"][k] + p1["perturbation"]["delta"][k]) < 1e-9, "the swapped pair has the opposite deltas"
        assert p2["perturbation"]["synthesised"][k] is None and p2["perturbation"]["delta"][k] is None and isinstance(p2["perturbation"]["recorded"][k], float)
        s7 = saved["speakers"]["7"]["perturbation"][k]
        assert set(s7) == {"mean_delta", "mean_abs_delta"} and abs(s7["mean_delta"]) < 1e-9 and abs(s7["mean_abs_delta"] - abs(p0["perturbation"]["delta"][k])) < 1e-9
        assert saved["speakers"]["12"]["perturbation"][k] == {"mean_delta": None, "mean_abs_delta": None}
        assert abs(saved["overall"]["perturbation"][k]["mean_abs_delta"] - s7["mean_abs_delta"]) < 1e-9
