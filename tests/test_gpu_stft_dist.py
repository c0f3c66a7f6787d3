"""ev_load_stft_dist / ev_stft_dist on the MI355X, through the C ABI, and what stands on them (audio.stft_distance, --vocoder_report
--spectral_distance).

Yardstick: tests/stft_dist_ref.py, the numpy float64 restatement of the definition in include/emojivoice.h (frames x basis as a matrix
product, the same basis formula).  The device sums in the matrix instruction's own order, so it differs from the restatement by float64
rounding.  The rule of every comparison (``check``):
  * first, a condition on the INPUT, not on the device: the float64 and the longdouble restatements agree to 1e-11 relative on every entry
    (2.9e-14 at worst for the inputs below; the smallest per-frame sum is 2.8e-3 for the speech-like rows and 3.3e-6 for the reflection
    rows, so nothing divides by nearly zero);
  * d_counts EQUAL;
  * every entry of d_frame and d_sums within 1e-9 relative; an entry that is exactly 0 in the restatement is 0 on the device.
1e-9 is the project's float64 margin (tests/test_gpu_stoi.py, tests/test_gpu_loudness.py): four orders above float64 order effects.
Observed on the MI355X: d_frame 9.2e-15 and d_sums 5.0e-16 at worst over all cases.  Every case prints its worst figure, DESIGN section 3.18
records them; the gate stays at 1e-9.  Every raw call writes into buffers with
sentinel margins (tests/analysis_gpu.py); 50.0 / -50.0 sit behind every row's length in the two signals.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import stft_dist_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

SMALL = R.GEOMETRIES[0]                  # (64, 10, 24): NB = 33, a one-column bin tail
_REF = {}
IDS = [f"{g[0]}-{g[1]}-{g[2]}" for g in R.GEOMETRIES]


def ref_of(key, x, y, lens, geom):
    """The restatements' results (float64, longdouble), computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: R.batch(x, y, lens, geom) + R.batch(x, y, lens, geom, dtype=np.longdouble)[:2])


def load(eng, geom, null=(), **kw):
    nfft, H, W = geom
    a = dict(W=W, H=H, nfft=nfft)
    a.update({k: v for k, v in kw.items() if k in a})
    w = np.ascontiguousarray(kw.get("window", R.hann(a["W"])), dtype=np.float64)
    tw = np.ascontiguousarray(kw.get("twiddle", R.twiddle(a["nfft"])), dtype=np.float64)
    p = lambda v, name: None if name in null else v.ctypes.data
    return eng.lib.ev_load_stft_dist(eng.h, p(w, "window"), p(tw, "twiddle"), a["W"], a["H"], a["nfft"])


def raw(eng, geom, x, y, lens, floor=R.POWER_FLOOR, B=None, L=None, null=()):
    """ev_stft_dist into guarded buffers: (rc, frame (B, NF, 4), sums (B, 4), counts (B,)) on the host; an output named in ``null`` is passed
    as NULL and comes back None.  ``B`` / ``L`` override the shape passed to the library."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    y = torch.as_tensor(y, dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    NF = R.frames(Lx, geom[0], geom[1])
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"frame": ((Bx, NF, 4), torch.float64), "sums": ((Bx, 4), torch.float64), "counts": ((Bx,), torch.int32)}, null)
    rc = eng.lib.ev_stft_dist(eng.h, None if "x" in null else x.data_ptr(), None if "y" in null else y.data_ptr(), None if d_len is None else d_len.data_ptr(),
                              B, L, float(floor), out.ptr("frame"), out.ptr("sums"), out.ptr("counts"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    frame, sums, counts = dev
    rf, rs, rc, lf, ls = ref
    e_in = max(R.rel_err(rf, lf), R.rel_err(rs, ls))
    nz = rf[rf != 0]
    assert e_in <= R.INPUT_TOL, f"{what}: the float64 and longdouble restatements differ by {e_in:.3e}, over {R.INPUT_TOL:g}: the input is ill-conditioned"
    assert np.array_equal(counts, rc), f"{what}: d_counts {counts.tolist()} against {rc.tolist()}"
    e_f, e_s = R.rel_err(frame, rf), R.rel_err(sums, rs)
    print(f"\nSTFT distance {what}: d_frame rel err {e_f:.3e}  d_sums rel err {e_s:.3e} (gate {R.TOL:g})  restatement float64 against longdouble {e_in:.3e}  "
          f"smallest per-frame sum {nz.min() if nz.size else 0:.3e}  counts {counts.tolist()}")
    assert e_f <= R.TOL, f"{what}: d_frame"
    assert e_s <= R.TOL, f"{what}: d_sums"


def engine_with(geom):
    return A.engine_with(load, geom)


@pytest.fixture(scope="module")
def engines():
    yield from A.engines_on_demand(engine_with)


@pytest.fixture(scope="module")
def small(engines):
    return engines(SMALL)


# ---- 1. the four geometries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=IDS)
def test_geometry_against_the_restatement(engines, geom):
    x, y, lens = R.rows_for(geom)
    ref = ref_of(("rows", geom), x, y, lens, geom)
    assert [c % 16 for c in ref[2].tolist()] == [15, 0, 1]
    eng = engines(geom)
    rc, *dev = raw(eng, geom, x, y, lens)
    assert rc == 0, err_of(eng)
    check(dev, ref, f"{geom} lens {lens}")
    for b in range(3):
        assert not dev[0][b, dev[2][b]:].any(), "zeros past the row's own frames"
    sc, lm, lsd = R.figures(dev[1], dev[2], geom[0])
    print(f"STFT distance {geom}: sc {np.round(sc, 5).tolist()} log_mag {np.round(lm, 5).tolist()} lsd_db {np.round(lsd, 4).tolist()}")


@pytest.mark.parametrize("geom", R.EDGE_GEOMETRIES, ids=[f"{g[0]}-{g[1]}-{g[2]}" for g in R.EDGE_GEOMETRIES])
def test_edge_geometry_against_the_restatement(engines, geom):
    """The same check where the skew walk and the K loop take their rare paths: H < 4, a skew of 3, W / 4 = 2 and 1 (under one round of four steps)."""
    test_geometry_against_the_restatement(engines, geom)


# ---- 2. identical signals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", (SMALL, R.GEOMETRIES[2]), ids=(IDS[0], IDS[2]))
def test_identical_signals_give_exact_zeros(engines, geom):
    x, _, lens = R.rows_for(geom)
    eng = engines(geom)
    rc, frame, sums, counts = raw(eng, geom, x, x, lens)
    assert rc == 0, err_of(eng)
    assert not frame[:, :, 0].any() and not frame[:, :, 2].any() and not frame[:, :, 3].any(), "y = x: both signals take the same path, bit for bit"
    assert not sums[:, 0].any() and not sums[:, 2].any() and not sums[:, 3].any()
    assert (sums[:, 1] > 0).all() and counts.tolist() == [R.frames(n, geom[0], geom[1]) for n in lens]
    for b, n in enumerate(lens):
        assert (frame[b, :counts[b], 1] > 0).all()


# ---- 3. invariance ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", (SMALL, R.GEOMETRIES[3]), ids=(IDS[0], IDS[3]))
def test_row_alone_in_a_batch_and_as_a_prefix_give_the_same_bits(engines, geom):
    eng = engines(geom)
    x, y, lens = R.rows_for(geom, seed=40)
    n = lens[0]
    c, d = x[0, :n].copy(), y[0, :n].copy()
    rc, *alone = raw(eng, geom, c[None], d[None], None)
    assert rc == 0, err_of(eng)
    rc, *again = raw(eng, geom, c[None], d[None], None)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    xb, yb, lb = R.padded([(x[2, :lens[2]], y[2, :lens[2]]), (c, d), (x[1, :lens[1]], y[1, :lens[1]])])
    rc, *batch = raw(eng, geom, xb, yb, lb)
    assert rc == 0
    xp, yp, lp = R.padded([(x[1, :lens[1]], y[1, :lens[1]]), (c, d)], L=n + 1235)
    xp[1, n:], yp[1, n:] = -7.5e3, 3.25e4                               # other garbage than in the batch of three
    rc, *prefix = raw(eng, geom, xp, yp, lp)
    assert rc == 0
    nf = int(alone[2][0])
    assert nf == R.frames(n, geom[0], geom[1])
    for name, other in (("inside a batch", batch), ("the prefix of a padded row", prefix)):
        assert np.array_equal(alone[0][0, :nf], other[0][1, :nf]) and not other[0][1, nf:].any(), f"d_frame: alone against {name}"
        assert np.array_equal(alone[1][0], other[1][1]) and alone[2][0] == other[2][1], f"d_sums, d_counts: alone against {name}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 3, 6):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, geom, xb, yb, lb)
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


# ---- 4. reflection ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", (SMALL, R.GEOMETRIES[1]), ids=(IDS[0], IDS[1]))
def test_reflection_at_both_ends(engines, geom):
    """A signal that is zero except inside its first and last W / 2 samples: a wrong fold shows in the first and last frames, which the CPU
    test of the folds shows to differ there by far more than the gate."""
    nfft, H, W = geom
    eng = engines(geom)
    rows = []
    for i, n in enumerate((3000, 3000 + H // 2 + 1)):                     # the last frame's centre at and before the row's end
        c = R.edge_signal(n, W, seed=i)
        rows.append((c, (c + 1e-3 * np.random.default_rng(800 + i).standard_normal(n)).astype(np.float32)))
    x, y, lens = R.padded(rows)
    ref = ref_of(("edge", geom), x, y, lens, geom)
    rc, *dev = raw(eng, geom, x, y, lens)
    assert rc == 0, err_of(eng)
    check(dev, ref, f"reflection {geom} lens {lens}")
    for b, n in enumerate(lens):
        nf = dev[2][b]
        for fold in ("edge", "reflect_even"):
            bad = R.row(x[b, :n], y[b, :n], geom, fold=fold)[0]
            for f in (0, nf - 1):
                moved = np.abs(bad[f] - ref[0][b, f]).max() / np.abs(ref[0][b, f]).max()
                assert moved > 1e-6, f"row {b} frame {f}: the {fold} fold would not show ({moved:.3e})"
                assert np.abs(dev[0][b, f] - ref[0][b, f]).max() / np.abs(ref[0][b, f]).max() <= R.TOL


# ---- 5. bad rows, NF = 0 ------------------------------------------------------------------------------------------------------------------------
def test_bad_rows_are_zeros_and_a_call_without_frames_succeeds(small):
    geom = SMALL
    x, y, lens = R.rows_for(geom)
    L = x.shape[1]
    x = np.concatenate([x, x[:1], x[:1], x[:1], x[:1]])
    y = np.concatenate([y, y[:1], y[:1], y[:1], y[:1]])
    lens = lens + [0, -3, L + 1, geom[0] // 2]
    rc, frame, sums, counts = raw(small, geom, x, y, lens)
    assert rc == 0, err_of(small)
    assert counts[3:].tolist() == [0, 0, 0, 0], "len 0, len < 0, len > L, len = nfft / 2: empty rows"
    assert not frame[3:].any() and not sums[3:].any()
    check((frame, sums, counts), ref_of("bad", x, y, lens, geom), "bad rows beside good ones")
    rc, frame, sums, counts = raw(small, geom, x[:, :geom[0] // 2 + 1], y[:, :geom[0] // 2 + 1], None)
    assert rc == 0 and counts.tolist() == [1 + (geom[0] // 2 + 1) // geom[1]] * 7, "len = nfft / 2 + 1: the shortest row with frames"
    check((frame, sums, counts), ref_of("shortest", x[:, :geom[0] // 2 + 1], y[:, :geom[0] // 2 + 1], None, geom), "the shortest rows with frames")
    z = np.zeros((2, geom[0] // 2), np.float32)
    rc, frame, sums, counts = raw(small, geom, z, z, None)               # L <= nfft / 2: NF = 0
    assert rc == 0, err_of(small)
    assert frame.shape == (2, 0, 4) and not sums.any() and counts.tolist() == [0, 0]


# ---- 6. d_frame NULL, allocations ---------------------------------------------------------------------------------------------------------------
def test_without_d_frame_the_sums_are_the_same_bits_and_a_second_call_allocates_nothing():
    geom = R.GEOMETRIES[1]
    eng = engine_with(geom)
    try:
        x, y, lens = R.rows_for(geom)
        rc, frame, sums, counts = raw(eng, geom, x, y, lens)
        assert rc == 0, err_of(eng)
        n0 = eng.alloc_count()
        rc, none, sums2, counts2 = raw(eng, geom, x, y, lens, null=("frame",))
        torch.cuda.synchronize()
        n1 = eng.alloc_count()
        assert rc == 0 and none is None and np.array_equal(sums2, sums) and np.array_equal(counts2, counts)
        assert n1 == n0 + 1, "the arena of the per-frame sums is allocated on the first call without d_frame"
        rc, _, sums3, _ = raw(eng, geom, x, y, lens, null=("frame",))
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(sums3, sums) and eng.alloc_count() == n1, "a second call at the same shape allocates nothing"
        n2 = eng.alloc_count()
        assert load(eng, geom) == 0 and eng.alloc_count() == n2 + 1, "the basis counts in ev_alloc_count"
    finally:
        eng.close()


# ---- 7. limits ----------------------------------------------------------------------------------------------------------------------------------
BAD_CALL = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)), ("power_floor", dict(floor=0.0)), ("power_floor", dict(floor=-1e-7)),
    ("power_floor", dict(floor=float("inf"))), ("power_floor", dict(floor=float("nan"))),
    ("d_sums", dict(null=("sums",))), ("d_counts", dict(null=("counts",))), ("d_x", dict(null=("x",))), ("d_y", dict(null=("y",))),
]


@pytest.mark.parametrize("word,kw", BAD_CALL, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_of_ev_stft_dist_fails_with_a_message_naming_it(small, word, kw):
    z = np.zeros((2, 256), np.float32)
    rc, *_ = raw(small, SMALL, z, z, None, **kw)                          # (a failed call writes nothing: raw checks that)
    msg = err_of(small)
    assert rc != 0 and "ev_stft_dist" in msg and word in msg, msg


_NAN_W = R.hann(24)
_NAN_W[5] = float("nan")
_INF_T = R.twiddle(64)
_INF_T[7, 1] = float("inf")
BAD_LOAD = [
    ("nfft=", dict(nfft=14, W=12)), ("nfft=", dict(nfft=2050)), ("nfft=", dict(nfft=65, W=25)), ("W=", dict(W=2)), ("W=", dict(W=68)), ("W=", dict(W=26)),
    ("nfft - W", dict(nfft=66, W=25)), ("H=", dict(H=0)), ("H=", dict(H=513)), ("window[5]", dict(window=_NAN_W)), ("twiddle[15]", dict(twiddle=_INF_T)),
    ("non-null", dict(null=("window",))), ("non-null", dict(null=("twiddle",))),
]


@pytest.mark.parametrize("word,kw", BAD_LOAD, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_LOAD)])
def test_each_limit_of_ev_load_stft_dist_fails_with_a_message_naming_it(small, word, kw):
    kw = dict(kw)
    null = kw.pop("null", ())
    rc = load(small, SMALL, null=null, **kw)
    msg = err_of(small)
    assert rc != 0 and "ev_load_stft_dist" in msg and word in msg, msg
    x, y, lens = R.rows_for(SMALL)                                        # the basis loaded before is still the one in use
    ref = ref_of(("rows", SMALL), x, y, lens, SMALL)
    rc, *dev = raw(small, SMALL, x[:1], y[:1], lens[:1])
    assert rc == 0 and dev[2][0] == ref[2][0] and R.rel_err(dev[1][0], ref[1][0]) <= R.TOL


def test_ev_stft_dist_before_a_load_fails_and_loading_again_replaces_the_basis():
    e = Engine(0)
    try:
        z = np.zeros((1, 256), np.float32)
        rc, *_ = raw(e, SMALL, z, z, None)
        assert rc != 0 and "ev_load_stft_dist" in err_of(e)
        assert load(e, R.GEOMETRIES[1]) == 0 and load(e, SMALL) == 0, err_of(e)
        x, y, lens = R.rows_for(SMALL)
        rc, *dev = raw(e, SMALL, x, y, lens)
        assert rc == 0, err_of(e)
        check(dev, ref_of(("rows", SMALL), x, y, lens, SMALL), "after loading twice")
    finally:
        e.close()


# ---- 8. audio.stft_distance ---------------------------------------------------------------------------------------------------------------------
def test_audio_stft_distance_on_three_ragged_rows():
    lens = [4000, 2600, 700]                                              # 700 samples: frames at 512 and 1024, none at 2048
    pairs = []
    for i, n in enumerate(lens):
        c = R.speech_like(n, seed=30 + i, fs=R.FS)
        pairs.append((c, R.processed(c, R.SNR_DB, seed=30 + i)))
    x, y, _ = R.padded(pairs)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    out = audio.stft_distance(xd, yd, lengths=lens)
    n0 = [audio._stft_dist_engine(xd.device, r).alloc_count() for r in audio.MSTFT_RESOLUTIONS]
    out2 = audio.stft_distance(xd, yd, lengths=lens)
    torch.cuda.synchronize()
    assert [audio._stft_dist_engine(xd.device, r).alloc_count() for r in audio.MSTFT_RESOLUTIONS] == n0, "a second call at the same shape allocates nothing"
    for k in ("sc", "log_mag", "lsd_db", "mstft"):
        assert out[k].dtype == torch.float64 and out[k].shape == (3,) and torch.equal(out[k].nan_to_num(-9.0), out2[k].nan_to_num(-9.0)), k
    per = []
    for nfft, hop, win in R.RESOLUTIONS:
        fr, sums, counts = R.batch(x, y, lens, (nfft, hop, win))
        frl, sumsl, _ = R.batch(x, y, lens, (nfft, hop, win), dtype=np.longdouble)
        assert max(R.rel_err(fr, frl), R.rel_err(sums, sumsl)) <= R.INPUT_TOL
        per.append(R.figures(sums, counts, nfft) + (counts,))
    assert out["frames"].cpu().tolist() == np.stack([p[3] for p in per], axis=1).tolist() and out["frames"][2].cpu().tolist() == [6, 0, 15]
    worst = 0.0
    for i, k in enumerate(("sc", "log_mag", "lsd_db")):
        for r, p in enumerate(out["per_resolution"]):
            got, want = p[k].cpu().numpy(), per[r][i]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (k, r)
            worst = max(worst, R.rel_err(got[~np.isnan(want)], want[~np.isnan(want)]))
        got, want = out[k].cpu().numpy(), np.mean([p[i] for p in per], axis=0)
        assert np.isnan(got[2]) and np.isnan(want[2]), "a row too short for the 2048 resolution gets NaN"
        worst = max(worst, R.rel_err(got[:2], want[:2]))
    got, want = out["mstft"].cpu().numpy(), np.mean([p[0] + p[1] for p in per], axis=0)
    worst = max(worst, R.rel_err(got[:2], want[:2]))
    print(f"\nSTFT distance audio.stft_distance 4000 / 2600 / 700 samples: worst rel err {worst:.3e} (gate {R.TOL:g})  frames {out['frames'].cpu().tolist()}  "
          f"mstft {out['mstft'].tolist()} sc {out['sc'].tolist()} log_mag {out['log_mag'].tolist()} lsd_db {out['lsd_db'].tolist()}")
    assert np.isnan(got[2]) and worst <= R.TOL
    one = audio.stft_distance(xd[0, :lens[0]], yd[0, :lens[0]])
    assert one["mstft"].shape == (1,) and float(one["mstft"][0]) == float(out["mstft"][0]), "a 1-D input is the same row"


# ---- 9. the CLI -----------------------------------------------------------------------------------------------------------------------------------
def test_vocoder_report_with_spectral_distance(tmp_path):
    from emojivoice_amd import cli

    sr = 22050
    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    for i, (name, spk) in enumerate(names.items()):
        cli.write_wav_pcm16(tmp_path / name, R.speech_like((16000, 19000, 300)[i], seed=20 + i, fs=sr), sr)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    old_file = {"path", "speaker", "seconds", "stoi", "estoi", "mel_l1", "lufs_shift"}
    old_summary = {"files", "unscored", "stoi", "estoi", "mel_l1", "lufs_shift"}
    new = {"mstft", "sc", "log_mag", "lsd_db"}
    rep = cli.cli(["--vocoder_report", str(flist), "--synthetic", "--vocoder_config", "v3", "--batch_size", "2", "--spectral_distance"])
    with open(f"{flist}.vocoder.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep)) and saved["stft_resolutions"] == [list(r) for r in audio.MSTFT_RESOLUTIONS]
    assert [set(f_) for f_ in saved["files"]] == [old_file | new] * 3
    a, b, c = saved["files"]
    print(f"\nSTFT distance --vocoder_report --spectral_distance (random weights): {[[f_[k] for k in sorted(new)] for f_ in saved['files']]}")
    for f_ in (a, b):
        assert all(isinstance(f_[k], float) and np.isfinite(f_[k]) and f_[k] > 0 for k in new)
    assert all(c[k] is None for k in new), "300 samples: nothing to analyse"
    s7 = saved["speakers"]["7"]
    assert set(s7) == old_summary | new
    for k in new:
        assert set(s7[k]) == {"mean", "max"} and abs(s7[k]["mean"] - (a[k] + b[k]) / 2) < 1e-12 and s7[k]["max"] == max(a[k], b[k])
        assert saved["speakers"]["12"][k] == {"mean": None, "max": None} and saved["overall"][k]["max"] == max(a[k], b[k])
    assert set(s7["stoi"]) == {"mean", "min"}
    plain = cli.cli(["--vocoder_report", str(flist), "--synthetic", "--vocoder_config", "v3", "--batch_size", "2"])
    assert [set(f_) for f_ in plain["files"]] == [old_file] * 3 and "stft_resolutions" not in plain
    assert set(plain["speakers"]["7"]) == old_summary and set(plain["overall"]) == old_summary
    assert [f_["seconds"] for f_ in plain["files"]] == [f_["seconds"] for f_ in saved["files"]]
