"""ev_load_stoi / ev_stoi on the MI355X, through the C ABI, and what stands on them (audio.stoi, --vocoder_report).

Yardstick: tests/stoi_ref.py, the numpy float64 restatement of the published algorithm with np.fft.rfft for the spectra.  The device runs
one fixed order of its own (include/emojivoice.h), so it differs from the restatement by float64 rounding.  The rule of every comparison
(``check``):
  * first, two conditions on the INPUT, not on the device: the restatement's mask margin is at least 1e-3 dB and its conditioning at least
    1e-3 (stoi_ref.py says what they are);
  * d_keep and d_counts are EQUAL;
  * d_tob within 1e-9, relative to max(|ref|, 1e-9 x the largest value of that row and signal);
  * d_seg and d_score within 1e-9 absolute.
A direct DFT as 256-term fma chains and an FFT differ by float64 rounding, some 1e-13 of a band's value; 1e-9 is four orders above
that, the margin tests/test_gpu_loudness.py takes for the same reason.  Observed on the MI355X (every case prints its worst figures, DESIGN
section 3.17 records them; the gate stays at 1e-9): d_tob 6.1e-14 (standard geometry), d_seg 1.7e-14, d_score 1.4e-15.  Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py); 50.0 / -50.0 sit behind every row's length in the two signals.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import stoi_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

_REF = {}


def ref_of(key, x, y, lens, g):
    """The restatement's result, computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: R.stoi(x, y, lens, g))


def load(eng, g, null=(), **kw):
    a = dict(W=g.W, H=g.H, nfft=g.nfft, n_bands=len(g.bands), N=g.N, window=g.window, twiddle=g.twiddle, bands=g.bands)
    a.update(kw)
    w = np.ascontiguousarray(a["window"], dtype=np.float64)
    tw = np.ascontiguousarray(a["twiddle"], dtype=np.float64)
    bd = np.ascontiguousarray(a["bands"], dtype=np.int32)
    p = lambda v, name: None if name in null else v.ctypes.data
    return eng.lib.ev_load_stoi(eng.h, p(w, "window"), p(tw, "twiddle"), p(bd, "bands"), a["W"], a["H"], a["nfft"], a["n_bands"], a["N"])


def raw(eng, g, x, y, lens, ratio=R.SILENCE_RATIO, clip=R.CLIP, B=None, L=None, null=()):
    """ev_stoi into guarded buffers: (rc, keep (B, NF), tob (B, 2, n_bands, NM), seg (B, NSEG, 2), score (B, 2), counts (B, 3)) on the host;
    an output named in ``null`` is passed as NULL and comes back None.  ``B`` / ``L`` override the shape passed to the library."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    y = torch.as_tensor(y, dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    NF, NM, NSEG = g.sizes(Lx)
    nb = len(g.bands)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"keep": ((Bx, NF), torch.uint8), "tob": ((Bx, 2, nb, NM), torch.float64), "seg": ((Bx, NSEG, 2), torch.float64),
                     "score": ((Bx, 2), torch.float64), "counts": ((Bx, 3), torch.int32)}, null)
    rc = eng.lib.ev_stoi(eng.h, None if "x" in null else x.data_ptr(), None if "y" in null else y.data_ptr(), None if d_len is None else d_len.data_ptr(),
                         B, L, float(ratio), float(clip), out.ptr("keep"), out.ptr("tob"), out.ptr("seg"), out.ptr("score"), out.ptr("counts"),
                         _stream_ptr())
    return (rc, *out.collect(rc).values())


def tob_err(dev, ref):
    """max |dev - ref| / max(|ref|, 1e-9 x the largest |ref| of that row and signal); an all-zero reference must be all zeros."""
    worst = 0.0
    for b in range(ref.shape[0]):
        for s in range(2):
            d, r = dev[b, s], ref[b, s]
            top = float(np.max(np.abs(r))) if r.size else 0.0
            if top == 0.0:
                assert not d.any(), "a row of zeros in the reference is a row of zeros on the device"
                continue
            worst = max(worst, float(np.max(np.abs(d - r) / np.maximum(np.abs(r), 1e-9 * top))))
    return worst


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    keep, tob, seg, score, counts = dev
    rows = ref["counts"][:, 0] > 0
    margin = float(ref["margin"][rows].min()) if rows.any() else float("inf")
    cond = float(ref["conditioning"].min())
    assert margin >= R.MIN_MARGIN_DB, f"{what}: the reference's mask margin {margin:.3e} dB is under {R.MIN_MARGIN_DB:g} dB"
    assert cond >= R.MIN_CONDITIONING, f"{what}: the reference's conditioning {cond:.3e} is under {R.MIN_CONDITIONING:g}"
    e_t = tob_err(tob, ref["tob"])
    e_s = float(np.max(np.abs(seg - ref["seg"]))) if seg.size else 0.0
    e_c = float(np.max(np.abs(score - ref["score"])))
    print(f"\nSTOI {what}: tob rel err {e_t:.3e}  seg abs err {e_s:.3e}  score abs err {e_c:.3e} (gate {R.TOL:g})  counts {counts.tolist()}  "
          f"margin {margin:.3f} dB  conditioning {cond:.3f}  scores {np.round(score, 6).tolist()}")
    assert np.array_equal(counts, ref["counts"]), f"{what}: d_counts {counts.tolist()} against {ref['counts'].tolist()}"
    assert np.array_equal(keep, ref["keep"]), f"{what}: d_keep"
    assert e_t <= R.TOL, f"{what}: d_tob"
    assert e_s <= R.TOL, f"{what}: d_seg"
    assert e_c <= R.TOL, f"{what}: d_score"


def engine_with(g):
    return A.engine_with(load, g)


@pytest.fixture(scope="module")
def std():
    yield from A.one_engine(load, R.STANDARD)


@pytest.fixture(scope="module")
def small():
    yield from A.one_engine(load, R.SMALL)


# ---- 1. the standard geometry -------------------------------------------------------------------------------------------------------------
def test_standard_geometry_three_snrs(std):
    x, y, lens = R.standard_rows()
    ref = ref_of("standard", x, y, lens, R.STANDARD)
    assert ref["counts"][:, 0].tolist() == [155, 103, 69] and (ref["counts"][:, 2] > 0).all()
    rc, *dev = raw(std, R.STANDARD, x, y, lens)
    assert rc == 0, err_of(std)
    check(dev, ref, f"standard 256/128/512 lens {lens} SNR {R.SNRS_DB}")
    for b in range(3):
        nf, nk, nseg = dev[4][b]
        assert not dev[0][b, nf:].any() and not dev[1][b, :, :, max(nk - 1, 0):].any() and not dev[2][b, nseg:].any(), "zeros past the row's own sizes"


# ---- 2. the small geometry: edges ---------------------------------------------------------------------------------------------------------
def test_small_geometry_edges_in_one_ragged_batch(small):
    x, y, lens = R.small_rows()
    ref = ref_of("small", x, y, lens, R.SMALL)
    assert ref["counts"].tolist() == R.SMALL_COUNTS
    rc, *dev = raw(small, R.SMALL, x, y, lens)
    assert rc == 0, err_of(small)
    check(dev, ref, f"small 64/32/128 lens {lens}")
    score = dev[3]
    assert not score[1:6].any() and not score[8].any(), "no segment: score 0"
    assert score[9, 0] == dev[2][9, 0, 0] and score[9, 1] == dev[2][9, 0, 1], "one segment: the score is that segment"


# ---- 3. the scan: masks wider than a wave and than a workgroup --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SCAN_SHAPES)
def test_scan_shapes(small, shape):
    c, d = R.scan_row(shape)
    x, y, lens = R.padded([(c, d)], tail=37)
    ref = ref_of(("scan", shape), x, y, lens, R.SMALL)
    k = ref["keep"][0, :ref["counts"][0, 0]].astype(bool)
    run = max((len(s) for s in "".join("x" if v else " " for v in ~k).split()), default=0)
    assert ref["counts"][0, 0] == 698
    assert {"first_dropped": not k[0] and k[1:].all(), "last_dropped": not k[-1] and k[0], "run_over_64": 64 < run <= 256, "run_over_256": run > 256,
            "all_kept": k.all()}[shape], f"{shape}: the mask (longest dropped run {run}) is not the shape the case is about"
    rc, *dev = raw(small, R.SMALL, x, y, lens)
    assert rc == 0, err_of(small)
    check(dev, ref, f"scan {shape} (longest dropped run {run})")


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------------------
def test_row_alone_in_a_batch_and_as_a_prefix_give_the_same_bits(small):
    g = R.SMALL
    c = R.small_clean(3000, seed=0)
    d = R.processed(c, 5.0, seed=0)
    n = len(c)
    rc, *alone = raw(small, g, c[None], d[None], None)
    assert rc == 0, err_of(small)
    rc, *again = raw(small, g, c[None], d[None], None)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    o1, o2 = R.dense_row(90, seed=5), R.dense_row(17, seed=6)
    xb, yb, lb = R.padded([o1, (c, d), o2])
    rc, *batch = raw(small, g, xb, yb, lb)
    assert rc == 0
    xp, yp, lp = R.padded([o2, (c, d)], L=n + 1235)
    xp[1, n:], yp[1, n:] = -7.5e3, 3.25e4                               # other garbage than in the batch of three
    rc, *prefix = raw(small, g, xp, yp, lp)
    assert rc == 0
    nf, nk, nseg = alone[4][0]
    for name, a, b, c_ in zip(("keep", "tob", "seg", "score", "counts"), alone, batch, prefix):
        valid = {"keep": nf, "tob": nk - 1, "seg": nseg}.get(name)
        cut = (lambda v: v) if valid is None else (lambda v: v[..., :valid] if name != "seg" else v[:valid])
        rest = (lambda v: np.zeros(0)) if valid is None else (lambda v: v[..., valid:] if name != "seg" else v[valid:])
        assert np.array_equal(cut(a[0]), cut(b[1])) and not rest(b[1]).any(), f"{name}: alone against inside a batch"
        assert np.array_equal(cut(a[0]), cut(c_[1])) and not rest(c_[1]).any(), f"{name}: alone against the prefix of a padded row"
    rc, _, _, _, score, counts = raw(small, g, xb, yb, lb, null=("keep", "tob", "seg"))
    assert rc == 0 and np.array_equal(score, batch[3]) and np.array_equal(counts, batch[4]), "without the optional outputs"
    base = small.lib.ev_get_arithmetic(small.h)
    try:
        for setting in (0, 3, 6):
            small.set_arithmetic(setting)
            rc, *got = raw(small, g, xb, yb, lb)
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        small.set_arithmetic(base)


# ---- 5. identical signals -----------------------------------------------------------------------------------------------------------------
def test_identical_signals_score_one(std, small):
    x, _, lens = R.standard_rows()
    rc, _, _, seg, score, counts = raw(std, R.STANDARD, x, x, lens)
    assert rc == 0, err_of(std)
    print(f"\nSTOI identical signals, standard geometry: 1 - score {(1.0 - score).tolist()}  counts {counts.tolist()}")
    assert (counts[:, 2] > 0).all() and (score[:, 0] >= 1.0 - 1e-12).all() and (score[:, 1] >= 1.0 - 1e-12).all()
    c = R.small_clean(3000)
    rc, _, _, _, score, _ = raw(small, R.SMALL, c[None], c[None], None)
    assert rc == 0 and score[0, 0] >= 1.0 - 1e-12


# ---- 6. bad rows, optional outputs, allocations -------------------------------------------------------------------------------------------------
def test_bad_rows_are_zeros_and_optional_outputs_may_be_null(small):
    g = R.SMALL
    c = R.small_clean(3000, seed=3)
    d = R.processed(c, 5.0, seed=3)
    x = np.stack([c, c, c, np.zeros_like(c), c])
    y = np.stack([d, d, d, d, d])
    lens = [0, -4, 3001, 3000, 3000]
    rc, keep, tob, seg, score, counts = raw(small, g, x, y, lens)
    assert rc == 0, err_of(small)
    assert counts[:3].tolist() == [[0, 0, 0]] * 3 and counts[3].tolist() == [92, 0, 0], "len < 1, len > L: empty rows; all-zero clean row: no frame kept"
    for b in range(4):
        assert not keep[b].any() and not tob[b].any() and not seg[b].any() and not score[b].any(), f"row {b} must be zeros"
    ref = ref_of("bad", x, y, lens, g)
    check((keep, tob, seg, score, counts), ref, "bad rows beside a good one")
    n0 = small.alloc_count()
    for null in (("keep",), ("tob",), ("seg",), ("keep", "tob", "seg")):
        rc, *got = raw(small, g, x, y, lens, null=null)
        assert rc == 0, err_of(small)
        assert np.array_equal(got[3], score) and np.array_equal(got[4], counts), f"without {null}"
        if "seg" not in null:
            assert np.array_equal(got[2], seg)
    n1 = small.alloc_count()
    rc, *_ = raw(small, g, x, y, lens, null=("keep", "tob", "seg"))
    torch.cuda.synchronize()
    assert rc == 0 and small.alloc_count() == n1, "a second call at a shape allocates nothing"
    assert n1 - n0 <= 2, "the arena grows when an optional output moves into it, not per call"


# ---- 7. limits ----------------------------------------------------------------------------------------------------------------------------
BAD_STOI = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)), ("silence_ratio", dict(ratio=0.0)), ("silence_ratio", dict(ratio=1.0)),
    ("silence_ratio", dict(ratio=float("nan"))), ("clip", dict(clip=1.0)), ("clip", dict(clip=float("nan"))),
    ("d_score", dict(null=("score",))), ("d_counts", dict(null=("counts",))), ("d_x", dict(null=("x",))), ("d_y", dict(null=("y",))),
]


@pytest.mark.parametrize("word,kw", BAD_STOI, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_STOI)])
def test_each_limit_of_ev_stoi_fails_with_a_message_naming_it(small, word, kw):
    z = np.zeros((2, 1024), np.float32)
    rc, *_ = raw(small, R.SMALL, z, z, None, **kw)                       # (a failed call writes nothing: raw checks that)
    msg = err_of(small)
    assert rc != 0 and "ev_stoi" in msg and word in msg, msg


_NAN_W = R.SMALL.window.copy()
_NAN_W[5] = float("nan")
_INF_T = R.SMALL.twiddle.copy()
_INF_T[7, 1] = float("inf")
BAD_LOAD = [
    ("H=", dict(H=16, W=32)), ("H=", dict(H=288, W=576, nfft=1024)), ("H=", dict(H=48, W=96)), ("W=", dict(W=65)), ("nfft=", dict(nfft=32)),
    ("nfft=", dict(nfft=2048)), ("n_bands=", dict(n_bands=0)), ("n_bands=", dict(n_bands=33)), ("N=", dict(N=1)), ("N=", dict(N=65)),
    ("bands[1]", dict(bands=[[2, 4], [4, 4], [7, 12]])), ("bands[2]", dict(bands=[[2, 4], [4, 7], [7, 66]])), ("bands[0]", dict(bands=[[-1, 4], [4, 7], [7, 12]])),
    ("window[5]", dict(window=_NAN_W)), ("twiddle[15]", dict(twiddle=_INF_T)), ("non-null", dict(null=("window",))), ("non-null", dict(null=("bands",))),
]


@pytest.mark.parametrize("word,kw", BAD_LOAD, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_LOAD)])
def test_each_limit_of_ev_load_stoi_fails_with_a_message_naming_it(small, word, kw):
    kw = dict(kw)
    if kw.get("nfft", 128) != 128 and "twiddle" not in kw:
        kw["twiddle"] = R.Geometry(64, 32, kw["nfft"], R.SMALL.bands, 4).twiddle
    if kw.get("W", 64) > 64 and "window" not in kw:
        kw["window"] = np.hanning(kw["W"] + 2)[1:-1]
    if kw.get("n_bands") == 33:
        kw["bands"] = [[2, 4]] * 33
    rc = load(small, R.SMALL, **kw)
    msg = err_of(small)
    assert rc != 0 and "ev_load_stoi" in msg and word in msg, msg
    c = R.small_clean(1500, seed=1)                                      # the tables loaded before are still the ones in use
    ref = ref_of("after-bad-load", c[None], R.processed(c, 5.0)[None], None, R.SMALL)
    rc, *dev = raw(small, R.SMALL, c[None], R.processed(c, 5.0)[None], None)
    assert rc == 0 and np.array_equal(dev[4], ref["counts"]) and abs(dev[3] - ref["score"]).max() <= R.TOL


def test_ev_stoi_before_ev_load_stoi_fails_and_loading_again_replaces_the_tables():
    e = Engine(0)
    try:
        z = np.zeros((1, 1024), np.float32)
        rc, *_ = raw(e, R.SMALL, z, z, None)
        assert rc != 0 and "ev_load_stoi" in err_of(e)
        assert load(e, R.STANDARD) == 0 and load(e, R.SMALL) == 0, err_of(e)
        c = R.small_clean(1500, seed=1)
        d = R.processed(c, 5.0)
        rc, *dev = raw(e, R.SMALL, c[None], d[None], None)
        assert rc == 0, err_of(e)
        check(dev, ref_of("after-bad-load", c[None], d[None], None, R.SMALL), "after loading twice")
    finally:
        e.close()


# ---- 8. audio.stoi at 22.05 kHz -------------------------------------------------------------------------------------------------------------
def test_audio_stoi_at_22050_hz():
    """audio.stoi resamples both signals to 10 kHz on the device; the restatement is fed host copies of the device's own resampled rows, so
    that what is compared is ev_stoi and the wrapper, not two resamplers."""
    sr = 22050
    lens = [44100, 30011, 400]
    pairs = []
    for i, n in enumerate(lens):
        c = R.speech_like(n, seed=10 + i, fs=sr)
        pairs.append((c, R.processed(c, (15.0, 0.0, 5.0)[i], seed=10 + i)))
    x, y, _ = R.padded(pairs)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    out = audio.stoi(xd, yd, sr, lengths=lens)
    e = audio._stoi_engine(xd.device)
    n0 = e.alloc_count()
    out2 = audio.stoi(xd, yd, sr, lengths=lens)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0, "a second call at the same shape allocates nothing"
    assert all(torch.equal(out[k], out2[k]) if k not in ("stoi", "estoi") else torch.equal(out[k].nan_to_num(-9.0), out2[k].nan_to_num(-9.0)) for k in out), "two calls"
    x10, y10 = audio.resample(xd, sr, 10000, lengths=lens).cpu().numpy(), audio.resample(yd, sr, 10000, lengths=lens).cpu().numpy()
    lens10 = [-(-n * 200 // 441) for n in lens]
    ref = R.stoi(x10, y10, lens10, R.STANDARD)
    rows = ref["counts"][:, 0] > 0
    assert float(ref["margin"][rows].min()) >= R.MIN_MARGIN_DB and float(ref["conditioning"].min()) >= R.MIN_CONDITIONING
    assert ref["counts"][:2, 2].min() > 0 and ref["counts"][2, 2] == 0
    got = np.stack([out["stoi"].cpu().numpy(), out["estoi"].cpu().numpy()], axis=1)
    e_s = float(np.max(np.abs(out["segments"].cpu().numpy() - ref["seg"])))
    e_c = float(np.max(np.abs(got[:2] - ref["score"][:2])))
    print(f"\nSTOI audio.stoi 2.0 / 1.36 / 0.02 s at 22.05 kHz: seg abs err {e_s:.3e} score abs err {e_c:.3e} (gate {R.TOL:g})  counts {out['counts'].tolist()}  "
          f"stoi {out['stoi'].tolist()} estoi {out['estoi'].tolist()}")
    assert out["stoi"].dtype == torch.float64 and np.array_equal(out["counts"].cpu().numpy(), ref["counts"])
    assert np.array_equal(out["keep"].cpu().numpy(), ref["keep"])
    assert e_s <= R.TOL and e_c <= R.TOL
    assert np.isnan(got[2]).all(), "a row too short to score gets NaN, not a number that looks like a score"
    one = audio.stoi(xd[0, :lens[0]], yd[0, :lens[0]], sr)
    assert one["stoi"].shape == (1,) and float(one["stoi"][0]) == float(out["stoi"][0]), "a 1-D input is the same row"


# ---- 9. the CLI -----------------------------------------------------------------------------------------------------------------------------
def test_vocoder_report_with_synthetic_weights(tmp_path):
    from emojivoice_amd import cli

    sr = 22050
    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    for i, (name, spk) in enumerate(names.items()):
        cli.write_wav_pcm16(tmp_path / name, R.speech_like((16000, 19000, 300)[i], seed=20 + i, fs=sr), sr)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    rep = cli.cli(["--vocoder_report", str(flist), "--synthetic", "--vocoder_config", "v3", "--batch_size", "2"])
    with open(f"{flist}.vocoder.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep)) and set(saved) >= {"sample_rate", "vocoder_config", "files", "speakers", "overall"}
    assert [set(f_) for f_ in saved["files"]] == [{"path", "speaker", "seconds", "stoi", "estoi", "mel_l1", "lufs_shift"}] * 3
    a, b, c = saved["files"]
    print(f"\nSTOI --vocoder_report (random weights): {[(f_['stoi'], f_['estoi'], f_['mel_l1'], f_['lufs_shift']) for f_ in saved['files']]}")
    for f_ in (a, b):
        assert -1.0 <= f_["stoi"] <= 1.0 and -1.0 <= f_["estoi"] <= 1.0 and f_["mel_l1"] > 0
    assert (a["seconds"], b["seconds"]) == (15872 / sr, 18944 / sr), "the recording is cut to 256 x frames samples"
    assert c["stoi"] is None and c["estoi"] is None and c["seconds"] is None, "300 samples: nothing to analyse"
    assert set(saved["speakers"]) == {"7", "12"}
    s7 = saved["speakers"]["7"]
    assert set(s7) == {"files", "unscored", "stoi", "estoi", "mel_l1", "lufs_shift"} and s7["files"] == 2 and s7["unscored"] == []
    assert abs(s7["stoi"]["mean"] - (a["stoi"] + b["stoi"]) / 2) < 1e-12 and s7["stoi"]["min"] == min(a["stoi"], b["stoi"])
    assert saved["speakers"]["12"]["stoi"] == {"mean": None, "min": None} and len(saved["speakers"]["12"]["unscored"]) == 1
    assert saved["overall"]["files"] == 3 and saved["overall"]["estoi"]["min"] == min(a["estoi"], b["estoi"])
