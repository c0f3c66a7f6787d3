"""The host side of ev_phase_vocoder, on the CPU.  The first part checks the YARDSTICK, tests/phase_vocoder_ref.py, against numpy's FFT and against
mutants of the definition: those tests exercise the restatement only and pass whether or not the library has the feature.  The rest needs it: the header,
the exports and the code object; audio.pitch_ratio, audio.time_stretch and audio.pitch_shift through their ``rows=`` / ``resampler=`` hooks; the CLI's
--augment_dataset with the device call replaced by the restatement.
"""
import argparse
import ctypes
import json
import math
import os
import re
import wave
from fractions import Fraction

import numpy as np
import pytest
import torch

import phase_vocoder_ref as R
from emojivoice_amd import _lib, audio, cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nfft, samples, rate) of the committed inputs: the prototype's range (nfft 64 and 256, 261 .. 1729 samples, the five rates)
COMMITTED = [(64, 261, 0.5), (64, 499, 0.8), (64, 262, 0.8), (64, 481, 1.25), (64, 700, 1.7), (256, 1029, 0.8), (256, 1729, 1.25), (256, 1301, 1.7)]


def row(n, seed=11):
    return R.speech_like(n, seed)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [16, 64, 256])
def test_analysis_is_the_rfft_of_the_windowed_frames(nfft):
    n, H = 5 * nfft + 3, nfft // 4
    x = row(n)
    _, _, re, im = R.analysis(x, n, nfft)
    pad = np.zeros(n + 2 * nfft)
    pad[nfft // 2: nfft // 2 + n] = x
    w = R.window(nfft)
    ref = np.stack([np.fft.rfft(pad[f * H: f * H + nfft] * w) for f in range(R.frames_of(n, nfft))])
    assert re.shape == ref.shape == (1 + n // H, nfft // 2 + 1)
    assert np.abs(re + 1j * im - ref).max() <= 1e-12 * np.abs(ref).max()
    mag, ang, _, _ = R.analysis(x, n, nfft)
    assert not mag[-2:].any() and not ang[-2:].any(), "two all-zero frames stand behind frame nf - 1"
    assert R.analysis(np.zeros(8, np.float32), 8, 16)[1].max() == 0.0, "atan2(0, 0) = 0"


@pytest.mark.parametrize("nfft", [16, 64, 256])
def test_synthesis_is_the_irfft_overlap_added(nfft):
    rng = np.random.default_rng(nfft)
    H, NB, n_out = nfft // 4, nfft // 2 + 1, 9
    yr, yi = rng.standard_normal((n_out, NB)), rng.standard_normal((n_out, NB))
    n = H * (n_out - 1)
    y, out_len = R.synthesis(yr, yi, n, 1.0, nfft, n)
    w = R.window(nfft)
    num, wss = np.zeros(H * (n_out - 1) + nfft), np.zeros(H * (n_out - 1) + nfft)
    for t in range(n_out):
        num[t * H: t * H + nfft] += np.fft.irfft(yr[t] + 1j * yi[t], nfft) * w
        wss[t * H: t * H + nfft] += w * w
    ref = (num / np.where(wss > R.FLT_MIN, wss, 1.0))[nfft // 2: nfft // 2 + n]
    assert out_len == n and np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("nfft,n", [(16, 65), (64, 261), (64, 1), (256, 1729)])
def test_rate_one_reproduces_the_input_edges_included(nfft, n):
    x = row(n)
    r = R.stretch_row(x, n, 1.0, nfft)
    assert r["out_len"] == n and r["n_out"] == r["nf"] == 1 + n // (nfft // 4)
    assert np.abs(r["y"] - x).max() <= 1e-9 * np.abs(x).max()


def test_time_steps_are_float64_products():
    i, a = R.time_steps(40, 1.7)
    s = np.arange(40, dtype=np.float64) * 1.7
    assert np.array_equal(i, np.floor(s).astype(np.int64)) and np.array_equal(a, s - np.floor(s))
    ld = np.floor(np.arange(40, dtype=np.longdouble) * np.longdouble(1.7)).astype(np.int64)
    if np.finfo(np.longdouble).nmant > 52:                               # 10 * 1.7 is 17.0 in float64 and 16.99... in a wider format: another frame
        assert np.any(ld != i), "the steps are part of the definition: a restatement in higher precision takes the float64 product as given"
    i5, a5 = R.time_steps(9, 0.5)
    assert set(a5.tolist()) == {0.0, 0.5} and R.steps_of(31, 0.8) == 39 and R.out_len_of(262, 0.8) == 328 and R.out_len_of(1, 8.0) == 0


@pytest.mark.parametrize("nfft,n,rate", COMMITTED)
def test_float64_and_longdouble_agree_on_the_committed_inputs(nfft, n, rate):
    x = row(n)
    a, b = R.stretch_row(x, n, rate, nfft), R.stretch_row(x, n, rate, nfft, dtype=np.longdouble)
    mags = np.hypot(b["Y"][..., 0], b["Y"][..., 1])
    eY = float(np.hypot(*(np.moveaxis(a["Y"] - b["Y"], -1, 0))).max() / mags.max())
    ey = float(np.abs(a["y"] - b["y"]).max() / np.abs(b["y"]).max())
    print(f"\nnfft {nfft} n {n} rate {rate}: float64 against longdouble Y {eY:.2e} y {ey:.2e}")
    assert (a["nf"], a["n_out"], a["out_len"]) == (b["nf"], b["n_out"], b["out_len"])
    assert eY <= R.INPUT_TOL and ey <= R.INPUT_TOL


# Each mutant on an input where its clause matters: (nfft, n, rate).  262 / 0.8 = 327.5: rint gives 328, floor 327.
MUTANT_CASES = {"a_swapped": (64, 499, 0.8), "round_for_floor": (64, 499, 0.8), "phasor_after_update": (64, 481, 1.25),
                "advance_from_previous": (256, 1029, 0.8), "c_two_at_edges": (64, 700, 1.7), "wss_without_squares": (64, 261, 0.5),
                "out_len_by_floor": (64, 262, 0.8)}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_misses_the_restatement(mutant):
    nfft, n, rate = MUTANT_CASES[mutant]
    assert (nfft, n, rate) in COMMITTED
    x = row(n)
    good = R.stretch_row(x, n, rate, nfft, size=R.out_len_of(n, rate))
    bad = R.stretch_row(x, n, rate, nfft, size=R.out_len_of(n, rate), mutant=mutant)
    miss = float(np.abs(bad["y"] - good["y"]).max() / np.abs(good["y"]).max())
    print(f"\nmutant {mutant}: misses by {miss:.3e} of the peak (at least {100 * R.TOL:g})")
    assert miss >= 100 * R.TOL


def test_the_wrap_is_no_mutant():
    """Dropping d -= 2 pi rint(d / 2 pi) moves phi by multiples of 2 pi only: the output changes by rounding, which is why it is not on the list."""
    n, nfft, rate = 499, 64, 0.8
    x = row(n)
    mag, ang, _, _ = R.analysis(x, n, nfft)
    yr, yi = R.propagate(mag, ang, R.frames_of(n, nfft), rate, nfft)
    unwrapped = ang.copy()
    unwrapped[3] += R.TWO_PI * 5
    ur, ui = R.propagate(mag, unwrapped, R.frames_of(n, nfft), rate, nfft)
    assert np.abs(ur - yr).max() <= 1e-9 * np.abs(yr).max() and np.abs(ui - yi).max() <= 1e-9 * np.abs(yr).max()


def test_batch_rows_and_the_stub():
    lens = [100, 0, 101, 37]
    x = R.batch(lens, 100, "noise", seed=3)
    r = R.stretch(x, lens, 0.8, 64)
    assert r["y"].shape == (4, 125) and r["stretch"].shape == (4, 9, 33, 2) and r["out_len"].tolist() == [125, 0, 0, 46]
    assert r["counts"].tolist() == [[7, 9], [0, 0], [0, 0], [3, 4]] and not r["y"][1:3].any() and not r["y"][3, 46:].any()
    assert R.lens_for(64, 17) == [481, 499, 261] and [1 + n // 16 for n in R.lens_for(64, 20, (12, 0, 1), 13)] == [25, 26, 27]
    y, n = R.rows_stub(torch.from_numpy(x), torch.tensor(lens), 0.8, 64)
    assert y.dtype == torch.float32 and np.array_equal(y.numpy(), r["y"].astype(np.float32)) and n.tolist() == r["out_len"].tolist()


# ---- the C ABI's face -----------------------------------------------------------------------------------------------------------------------------
def test_header_abi_line_and_symbols():
    head = open(os.path.join(REPO, "include", "emojivoice.h")).read()
    line = next(ln for ln in head.splitlines() if ln.startswith("#define EV_ABI_VERSION"))
    assert re.match(r"#define EV_ABI_VERSION 4\b", line) and "ev_load_phase_vocoder, ev_phase_vocoder" in line
    assert "int ev_load_phase_vocoder(ev_handle *h, const double *window /* HOST (nfft) */, const double *twiddle /* HOST (nfft, 2) */, int nfft);" in head
    assert "int ev_phase_vocoder(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L, double rate," in head
    assert {"ev_load_phase_vocoder", "ev_phase_vocoder"} <= set(_lib.EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.ev_abi_version() == 4 and lib.ev_load_phase_vocoder and lib.ev_phase_vocoder


def test_new_kernels_neither_spill_nor_use_scratch():
    """The register census of the four new kernels alone (tests/test_code_object.py holds the whole library to the same rule)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("code_object", os.path.join(REPO, "tools", "code_object.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):                                   # (first: nothing of this test runs without the tool)
        pytest.skip("llvm-readelf of the ROCm toolchain is not installed")
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    ks = {k["demangled"].split("(")[0]: k for k in co.kernels(_lib.LIB_PATH)}
    for name in ("pv_analysis_kernel", "pv_propagate_kernel", "pv_synthesis_kernel", "pv_inv_basis_kernel"):
        assert ks[name]["vgpr_spill_count"] == 0 and ks[name]["private_segment_fixed_size"] == 0, (name, ks[name])
    assert ks["pv_synthesis_kernel"]["group_segment_fixed_size"] <= 160 * 1024


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------------
def test_pitch_ratio_terms_and_cents():
    for s in list(range(-12, 13)) + [0.5, -3.25, 11.9]:
        r = audio.pitch_ratio(s)
        assert isinstance(r, Fraction) and 1 <= r.numerator <= 640 and 1 <= r.denominator <= 320, (s, r)
        # some k / 320 lies within 1 / 640 of any ratio, the best fraction is no worse, and the ratio is at least 1 / 2: under 1 / 320 relative
        assert abs(audio.pitch_cents(r) - 100.0 * s) <= 1200.0 * math.log2(1.0 + 1.0 / 320.0), (s, r)
    assert audio.pitch_ratio(12) == 2 and audio.pitch_ratio(-12) == Fraction(1, 2) and audio.pitch_ratio(0) == 1
    assert audio.pitch_ratio(1) == Fraction(196, 185) and audio.pitch_ratio(-1) == Fraction(185, 196)
    for bad in (12.5, -13, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="n_steps"):
            audio.pitch_ratio(bad)


def test_time_stretch_through_rows():
    lens = [481, 0, 261]
    x = torch.from_numpy(R.batch(lens, 502, "speech", seed=5))
    calls = []

    def rows(xb, ln, rate, n_fft):
        calls.append((tuple(xb.shape), None if ln is None else ln.tolist(), rate, n_fft))
        return R.rows_stub(xb, ln, rate, n_fft)
    y, out = audio.time_stretch(x, 0.8, lens, n_fft=64, rows=rows)
    ref = R.stretch(x.numpy(), lens, 0.8, 64)
    assert y.shape == (3, 628) and y.dtype == torch.float32 and np.array_equal(y.numpy(), ref["y"].astype(np.float32))
    assert out.dtype == torch.int64 and out.tolist() == [601, 0, 326] and calls == [((3, 502), lens, 0.8, 64)]
    y1, out1 = audio.time_stretch(x[0, :481], 0.8, n_fft=64, rows=rows)                         # 1-D: B = 1, no lengths
    assert y1.shape == (1, 601) and out1.tolist() == [601] and calls[-1] == ((1, 481), None, 0.8, 64)
    assert np.array_equal(y1[0].numpy(), y[0, :601].numpy()), "a row alone equals the row in a batch"
    y0, out0 = audio.time_stretch(torch.ones(2, 3), 8.0, rows=rows)                             # rint(3 / 8) = 0 samples
    assert y0.shape == (2, 0) and out0.tolist() == [0, 0]


def test_time_stretch_splits_by_the_scratch_limit(monkeypatch):
    x = torch.from_numpy(R.batch([300] * 5, 300, "noise", seed=6))
    groups = []

    def rows(xb, ln, rate, n_fft):
        groups.append(xb.shape[0])
        return R.rows_stub(xb, ln, rate, n_fft)
    assert audio.phase_vocoder_scratch_bytes(1, 300, 0.8, 64) == 8 * 33 * (2 * 19 + 2 * 24)
    monkeypatch.setattr(audio, "PHASE_VOCODER_SCRATCH_BYTES", 2 * audio.phase_vocoder_scratch_bytes(1, 300, 0.8, 64) + 1)
    y, out = audio.time_stretch(x, 0.8, n_fft=64, rows=rows)
    assert groups == [2, 2, 1] and y.shape == (5, 375) and out.tolist() == [375] * 5
    monkeypatch.setattr(audio, "PHASE_VOCODER_SCRATCH_BYTES", 100)
    with pytest.raises(ValueError, match="4 GiB"):
        audio.time_stretch(x, 0.8, n_fft=64, rows=rows)


def test_argument_errors_of_the_python_layer():
    x = torch.zeros(2, 100)
    for rate in (0.1, 8.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="rate"):
            audio.time_stretch(x, rate, rows=R.rows_stub)
    for n_fft in (8, 24, 4096, 100, 64.5):
        with pytest.raises(ValueError, match="n_fft"):
            audio.time_stretch(x, 0.8, n_fft=n_fft, rows=R.rows_stub)
    with pytest.raises(ValueError, match="1-D or"):
        audio.time_stretch(torch.zeros(2, 3, 4), 0.8, rows=R.rows_stub)
    with pytest.raises(ValueError, match="empty"):
        audio.time_stretch(torch.zeros(2, 0), 0.8, rows=R.rows_stub)
    with pytest.raises(ValueError, match="2 lengths expected"):
        audio.time_stretch(x, 0.8, [100], rows=R.rows_stub)
    with pytest.raises(audio.EvLibraryError, match="GPU"):
        audio.time_stretch(x, 0.8)
    with pytest.raises(ValueError, match="n_steps"):
        audio.pitch_shift(x, 13, rows=R.rows_stub)
    with pytest.raises(ValueError, match="sr"):
        audio.pitch_shift(x, 1, sr=0, rows=R.rows_stub)
    with pytest.raises(ValueError, match="2 lengths expected"):
        audio.pitch_shift(x, 1, lengths=[1, 2, 3], rows=R.rows_stub)
    with pytest.raises(ValueError, match="n_fft"):
        audio.pitch_shift(x, 1, n_fft=100, rows=R.rows_stub)


def linear_resampler(y, up, down, lengths):
    """A stand-in for the device resampler: linear interpolation to ceil(L up / down) samples, zeros past ceil(len up / down)."""
    B, L = y.shape
    n_out = -(-L * up // down)
    pos = np.arange(n_out) * (down / up)
    out = np.stack([np.interp(pos, np.arange(L), r.numpy(), right=0.0) for r in y]).astype(np.float32)
    for b, n in enumerate(lengths.tolist()):
        out[b, -(-n * up // down):] = 0.0
    return torch.from_numpy(out)


def test_pitch_shift_lengths_and_the_realised_shift():
    sr, n = 8000, 4000
    t = np.arange(n) / sr
    tone = (0.5 * np.sin(2 * np.pi * 200.0 * t)).astype(np.float32)
    x = torch.from_numpy(np.stack([tone, tone]))
    seen = []

    def rows(xb, ln, rate, n_fft):
        seen.append((rate, n_fft, ln.tolist()))
        return R.rows_stub(xb, ln, rate, n_fft)
    y, cents = audio.pitch_shift(x, 2, sr, [n, 3000], n_fft=256, rows=rows, resampler=linear_resampler)
    assert y.shape == x.shape and y.dtype == torch.float32 and cents == pytest.approx(200.0, abs=0.05)
    assert seen == [(49 / 55, 256, [n, 3000])], "time_stretch runs at q / p"
    assert not y[1, 3000:].any() and y[1, 2000:3000].abs().max() > 0.3 and y[0, 3000:].abs().max() > 0.3
    seg = y[0, 1024:3072].numpy().astype(np.float64) * np.hanning(2048)
    peak_hz = np.argmax(np.abs(np.fft.rfft(seg, 1 << 16))) * sr / (1 << 16)
    assert abs(1200 * math.log2(peak_hz / 200.0) - cents) <= 20.0, peak_hz
    same, zero = audio.pitch_shift(x, 0, sr, rows=rows, resampler=linear_resampler)
    assert zero == 0.0 and torch.equal(same, x) and same.data_ptr() != x.data_ptr() and len(seen) == 1
    low, c = audio.pitch_shift(x[0], -12, sr, n_fft=256, rows=rows, resampler=linear_resampler)   # 1-D: B = 1
    assert low.shape == (1, n) and c == -1200.0 and seen[-1][0] == 2.0


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------------
def ns(**over):
    a = dict(augment_dataset=None, out_dir=None, rates=None, semitones=None, batch_size=2, sample_rate=None, prepare_dataset=None, peak=0.95)
    a.update(over)
    return argparse.Namespace(**a)


def test_augment_arguments():
    with pytest.raises(AssertionError, match="--out_dir"):
        cli.validate_args(ns(augment_dataset="x.txt", rates="0.9"))
    with pytest.raises(AssertionError, match="at least one"):
        cli.validate_args(ns(augment_dataset="x.txt", out_dir="d"))
    for bad in (dict(rates="0.9,1.0"), dict(rates="9"), dict(rates="fast"), dict(semitones="0"), dict(semitones="13"), dict(rates="nan")):
        with pytest.raises(AssertionError):
            cli.validate_args(ns(augment_dataset="x.txt", out_dir="d", **bad))
    a = cli.validate_args(ns(augment_dataset="x.txt", out_dir="d", rates="0.9, 1.1", semitones="-1,1"))
    assert a.rates == [0.9, 1.1] and a.semitones == [-1.0, 1.0]
    p = cli.cli.__doc__ or ""
    assert "--augment_dataset clean/filelist.txt --out_dir aug --rates 0.9,1.1 --semitones -1,1" in cli.__doc__, p


def read_pcm16(path):
    with wave.open(str(path), "rb") as f:
        assert f.getnchannels() == 1 and f.getsampwidth() == 2
        return f.getframerate(), np.frombuffer(f.readframes(f.getnframes()), "<i2")


def test_augment_dataset_with_the_restatement_behind_it(tmp_path, monkeypatch):
    sr = 8000
    wavs = {"a.wav": R.speech_like(1600, 1), "b.wav": R.speech_like(1201, 2), "c.wav": R.speech_like(900, 3)}
    for name in wavs:
        (tmp_path / name).write_bytes(b"")
    flist = tmp_path / "filelist.txt"
    flist.write_text(f"{tmp_path / 'a.wav'}|7|first\nb.wav|7|second\nc.wav|12|third take\n", encoding="utf-8")
    monkeypatch.setattr(audio, "load_audio", lambda path, sr=22050, device="cuda": torch.from_numpy(wavs[os.path.basename(str(path))]).unsqueeze(0))
    time_stretch = audio.time_stretch
    monkeypatch.setattr(audio, "time_stretch", lambda y, rate, lengths=None, n_fft=1024, rows=None: time_stretch(y, rate, lengths, 256, rows))
    args = cli.validate_args(ns(augment_dataset=str(flist), out_dir=str(tmp_path / "aug"), rates="0.9,1.25", semitones="+1", sample_rate=sr))
    rep = cli.augment_dataset(args, "cpu", rows=R.rows_stub, resampler=linear_resampler)
    out = tmp_path / "aug"
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted(["filelist.txt"] + [f"{b}{t}.wav" for b in "abc" for t in ("_r0.90", "_r1.25", "_p+1.00")])
    lines = (out / "filelist.txt").read_text(encoding="utf-8").splitlines()
    assert len(lines) == 3 + 9 and lines[0] == f"{tmp_path / 'a.wav'}|7|first" and lines[2].endswith("c.wav|12|third take")
    assert [ln.split("|", 1)[1] for ln in lines[3:]] == ["7|first", "7|second"] * 3 + ["12|third take"] * 3
    assert os.path.basename(lines[3].split("|")[0]) == "a_r0.90.wav" and os.path.basename(lines[-1].split("|")[0]) == "c_p+1.00.wav"
    rate, pcm = read_pcm16(out / "b_r0.90.wav")
    ref = R.stretch(wavs["b.wav"][None, :], None, 0.9, 256)
    assert rate == sr and len(pcm) == ref["out_len"][0] == round(1201 / 0.9)
    assert np.array_equal(pcm, np.round(np.clip(ref["y"][0].astype(np.float32).astype(np.float64), -1, 1) * 32767.0).astype("<i2"))
    assert len(read_pcm16(out / "c_p+1.00.wav")[1]) == 900 and len(read_pcm16(out / "a_r1.25.wav")[1]) == 1280
    saved = json.loads((tmp_path / "filelist.txt.augment.json").read_text())
    assert saved == json.loads(json.dumps(rep)) and saved["rates"] == [0.9, 1.25] and saved["semitones"] == [1.0]
    assert saved["realised_cents"] == {"+1.00": pytest.approx(100.0, abs=0.01)}
    s7, s12 = saved["speakers"]["7"], saved["speakers"]["12"]
    assert s7["files"] == 2 and s7["variants"] == 6 and s7["seconds_before"] == pytest.approx(2801 / sr)
    assert s7["seconds_after"] == pytest.approx((2801 * 2 + round(1600 / 0.9) + round(1201 / 0.9) + 1280 + 961) / sr)
    assert s12["seconds_after"] == pytest.approx((900 * 2 + 1000 + 720) / sr) and s7["below_two_minutes"] and saved["below_two_minutes"] == ["12", "7"]
    assert [v["kind"] for v in saved["files"][0]["variants"]] == ["rate", "rate", "semitones"]
