"""The pitch tracker without a GPU: the numpy float64 restatement (tests/pitch_ref.py) on tones whose f0 is known, the lag arithmetic of
``audio.pitch_yin``, ``audio.prosody_statistics`` on hand-made contours, the JSON of ``--prosody_report`` with ``pitch_yin`` stubbed by
the restatement, and the declaration of ``ev_pitch_yin``.

ACCURACY of the restatement at 22050 Hz, W 1024, H 256, lags 36 .. 340, threshold 0.1, over 8192 samples (relative error of f0, measured
here; the tolerances in pitch_ref.py are 2 x the worst case of each column, and tests/test_gpu_pitch.py holds audio.pitch_yin to them):
                      interior frames (26 of 32)     every voiced frame
    sine 110 Hz       5.4e-6                         5.0e-3  (29 voiced)
    sine 220 Hz       4.7e-5                         5.3e-3  (31)
    sine 440 Hz       2.0e-4                         1.5e-3  (32)
    3 harmonics 110   7.2e-6                         6.0e-3  (29)
    3 harmonics 220   5.3e-5                         1.8e-3  (31)
    3 harmonics 440   2.3e-4                         8.4e-4  (32)
Interior frames see the tone over their whole span; the error there is the parabola's, and grows with f0 as the period shrinks to a few
samples.  The frames at the ends of the row see zeros in part of the span, which shifts the minimum of d' by up to half a per cent.
"""
import argparse
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pitch_ref as P
from emojivoice_amd import _lib, audio, cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 22050


@pytest.mark.parametrize("amps", [(1.0,), (1.0, 0.5, 0.25)], ids=["sine", "3-harmonics"])
@pytest.mark.parametrize("f0", [110.0, 220.0, 440.0])
def test_restatement_recovers_f0(f0, amps):
    y = P.harmonic_tone(f0, 8192, SR, amps=amps)
    r = P.pitch_yin(y, None, 1024, 256, 36, 340, 0.1)
    f = P.f0_from_period(r["period"], SR)[0]
    v, it = r["lag"][0] > 0, P.interior_frames(32, 8192)
    e_in, e_all = float(np.max(np.abs(f[it] / f0 - 1))), float(np.max(np.abs(f[v] / f0 - 1)))
    print(f"\nPITCH restatement {f0} Hz {len(amps)} harmonics: voiced {int(v.sum())}/32, rel err interior {e_in:.3e} all voiced {e_all:.3e}")
    assert it.sum() == 26 and v[it].all(), "every interior frame is voiced"
    assert e_in <= P.F0_TOL_INTERIOR and e_all <= P.F0_TOL_ALL
    assert np.all(r["cmnd"][0][v] < 0.1) and np.all(r["period"][0][~v] == 0)
    assert np.all(np.abs(r["period"][0][v] - r["lag"][0][v]) <= 1.0), "the parabola moves the lag by at most one sample"


def test_silence_and_a_one_sample_row_are_unvoiced():
    x = np.zeros((2, 2048), np.float32)
    x[1, 0] = 0.7
    r = P.pitch_yin(x, [2048, 1], 1024, 256, 36, 340, 0.1)
    assert not r["lag"].any() and not r["period"].any()
    assert np.all(r["cmnd"][0] == 1.0), "a silent frame has d' = 1 at every lag"
    assert r["cmnd"][1, 0] > 0.1 and not r["cmnd"][1, 1:].any(), "one frame, aperiodic; the rest of the row is past its length"
    assert np.all(r["margin"][0] == 0.9), "nothing but the threshold is near a silent frame's decision"
    bad = P.pitch_yin(x, [0, 2049], 1024, 256, 36, 340, 0.1)
    assert not bad["lag"].any() and not bad["cmnd"].any()


def test_parity_rows_of_the_gpu_test_leave_out_no_frame():
    x, lens = P.parity_rows()
    r = P.pitch_yin(x, lens, **P.STD)
    print(f"\nPITCH parity rows: least margin per row {[float(r['margin'][b].min()) for b in range(4)]}")
    assert int((r["margin"] < 1e-9).sum()) == 0
    assert r["lag"].shape == (4, 32) and (r["lag"][2, :20] > 0).sum() >= 4 and not r["lag"][2, 20:].any()
    assert [g[:4] for g in P.GEOMETRIES] == [(64, 64, 1, 1), (4096, 4096, 1, 2048), (1024, 64, 36, 340), (1024, 256, 100, 100)]


def test_framing_is_centred_on_the_mel_frame():
    # frame f of ev_mel_spectrogram at hop H (center=False, reflect padding (1024 - H) / 2) covers samples [f H - 384, f H + 640): centre f H + 128
    W, H, tau_max = 1024, 256, 340
    x = np.arange(1, 20001, dtype=np.float32)
    span = P.frame_span(x, 10, W, H, tau_max)
    first = int(span[0]) - 1
    assert first == 10 * H + H // 2 - (W + tau_max) // 2 and len(span) == W + tau_max + 1
    assert abs((first + len(span) / 2.0) - (10 * H + H / 2.0)) <= 0.5
    assert np.all(P.frame_span(x, 0, W, H, tau_max)[: (W + tau_max) // 2 - H // 2] == 0), "samples left of the row enter as zeros"


def test_lag_range_of_audio_pitch_yin():
    assert audio.pitch_lag_range(22050, 65.0, 600.0) == (36, 340)
    assert audio.pitch_lag_range(22050, 50.0, 441.0) == (50, 441)
    assert audio.pitch_lag_range(16000, 80.0, 400.0) == (40, 200)
    assert audio.pitch_lag_range(44100, 65.0, 600.0) == (73, 679)
    with pytest.raises(ValueError):
        audio.pitch_lag_range(22050, 600.0, 65.0)
    with pytest.raises(ValueError):
        audio.pitch_lag_range(22050, 0.0, 65.0)
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.pitch_yin(torch.zeros(4000))
    with pytest.raises(ValueError):
        audio.pitch_yin(torch.zeros(1, 2, 3))


def test_prosody_statistics_on_hand_made_contours():
    f0 = torch.tensor([[100.0, 0.0, 200.0, 400.0, 0.0, 999.0],
                       [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                       [150.0, 150.0, 150.0, 150.0, 150.0, 150.0]])
    voiced = f0 > 0
    st = audio.prosody_statistics(f0, voiced, lengths=[5, 6, 6])            # row 0: its sixth frame is past the row
    assert set(st) == {"voiced_fraction", "f0_median", "f0_p05", "f0_p95", "f0_range_semitones"}
    assert all(v.shape == (3,) and v.dtype == torch.float32 for v in st.values())
    assert st["voiced_fraction"].tolist() == pytest.approx([3 / 5, 0.0, 1.0])
    want = np.percentile([100.0, 200.0, 400.0], [5, 50, 95])
    assert [float(st[k][0]) for k in ("f0_p05", "f0_median", "f0_p95")] == pytest.approx(want.tolist(), rel=1e-6)
    assert float(st["f0_range_semitones"][0]) == pytest.approx(12 * math.log2(want[2] / want[0]), rel=1e-5)
    for k in ("f0_median", "f0_p05", "f0_p95", "f0_range_semitones"):
        assert math.isnan(float(st[k][1])), "no voiced frame: NaN"
    assert float(st["f0_median"][2]) == 150.0 and float(st["f0_range_semitones"][2]) == 0.0
    one = audio.prosody_statistics(f0[0], voiced[0])                        # 1-D, every frame counted
    assert one["voiced_fraction"].tolist() == pytest.approx([4 / 6])


def test_prosody_report_json_shape(tmp_path, monkeypatch):
    tones = {"a.wav": (110.0, 8192), "b.wav": (220.0, 6000), "c.wav": (0.0, 3000), "d.wav": (330.0, 8192)}
    for name in tones:
        (tmp_path / name).write_bytes(b"")                                  # (the stubs below never open them)
    flist = tmp_path / "filelist.txt"
    flist.write_text(f"{tmp_path / 'a.wav'}|7|first\nb.wav|7|second\nc.wav|12|silent take\nd.wav|12|fourth\n", encoding="utf-8")
    loads, calls = [], []

    def fake_load(path, sr=22050, device="cuda"):
        f0, n = tones[os.path.basename(str(path))]
        loads.append((os.path.basename(str(path)), sr))
        y = P.harmonic_tone(f0, n) if f0 else np.zeros(n, np.float32)
        return torch.from_numpy(y).unsqueeze(0)

    def fake_pitch_yin(y, sr=22050, fmin=65.0, fmax=600.0, frame_length=1024, hop_length=256, threshold=0.1, lengths=None):
        calls.append((tuple(y.shape), list(lengths)))
        t0, t1 = audio.pitch_lag_range(sr, fmin, fmax)
        r = P.pitch_yin(y.numpy(), lengths, frame_length, hop_length, t0, t1, threshold)
        return {"f0": torch.from_numpy(P.f0_from_period(r["period"], sr)).float(), "voiced": torch.from_numpy(r["lag"] > 0),
                "aperiodicity": torch.from_numpy(r["cmnd"]).float()}

    monkeypatch.setattr(audio, "load_audio", fake_load)
    monkeypatch.setattr(audio, "pitch_yin", fake_pitch_yin)
    args = cli.validate_args(argparse.Namespace(prosody_report=str(flist), batch_size=3, sample_rate=None, prepare_dataset=None))
    rep = cli.prosody_report(args, "cpu")
    assert loads == [("a.wav", 22050), ("b.wav", 22050), ("c.wav", 22050), ("d.wav", 22050)]
    assert calls == [((3, 8192), [8192, 6000, 3000]), ((1, 8192), [8192])], "padded batches of --batch_size files, each row with its length"
    with open(f"{flist}.prosody.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert set(saved) == {"sample_rate", "hop_length", "files", "speakers"} and saved["sample_rate"] == 22050 and saved["hop_length"] == 256
    keys = {"path", "speaker", "seconds", "frames", "voiced_fraction", "f0_median", "f0_p05", "f0_p95", "f0_range_semitones"}
    assert [set(f) for f in saved["files"]] == [keys] * 4
    assert [(os.path.basename(f["path"]), f["speaker"], f["frames"]) for f in saved["files"]] == [("a.wav", "7", 32), ("b.wav", "7", 24), ("c.wav", "12", 12),
                                                                                                    ("d.wav", "12", 32)]
    a, b, c, d = saved["files"]
    assert a["f0_median"] == pytest.approx(110.0, rel=P.F0_TOL_INTERIOR) and b["f0_median"] == pytest.approx(220.0, rel=P.F0_TOL_INTERIOR)
    assert a["voiced_fraction"] >= 26 / 32 and a["seconds"] == 8192 / 22050
    assert c["voiced_fraction"] == 0.0 and all(c[k] is None for k in ("f0_median", "f0_p05", "f0_p95", "f0_range_semitones")), "NaN is written as null"
    assert set(saved["speakers"]) == {"7", "12"}
    s7, s12 = saved["speakers"]["7"], saved["speakers"]["12"]
    assert set(s7) == {"files", "voiced_fraction", "f0_median", "f0_p05", "f0_p95", "f0_range_semitones"}
    assert s7["files"] == 2 and s12["files"] == 2
    # pooled over the speaker's voiced frames: an octave between the 5th and the 95th percentile of speaker 7, none inside a file
    assert s7["f0_p05"] == pytest.approx(110.0, rel=P.F0_TOL_ALL) and s7["f0_p95"] == pytest.approx(220.0, rel=P.F0_TOL_ALL)
    assert s7["f0_range_semitones"] == pytest.approx(12.0, abs=0.3) and a["f0_range_semitones"] < 0.3
    assert s12["f0_median"] == pytest.approx(330.0, rel=P.F0_TOL_ALL), "the silent take adds frames, not pitch"
    assert s12["voiced_fraction"] == pytest.approx(d["voiced_fraction"] * 32 / 44)

    empty = tmp_path / "empty.txt"
    empty.write_text("\n", encoding="utf-8")
    with pytest.raises(SystemExit, match="no files"):
        cli.prosody_report(argparse.Namespace(prosody_report=str(empty), batch_size=4), "cpu")
    with pytest.raises(AssertionError, match="Batch size"):
        cli.validate_args(argparse.Namespace(prosody_report=str(flist), batch_size=0, sample_rate=None, prepare_dataset=None))


def test_header_declares_and_library_exports_ev_pitch_yin():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+ev_pitch_yin\s*\(([^;]*)\)\s*;", header)
    assert m, "ev_pitch_yin is not declared in include/emojivoice.h"
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ["ev_handle *h", "const float *d_x", "const int32_t *d_len", "int B", "int L", "int frame_length", "int hop_length", "int tau_min",
                    "int tau_max", "float threshold", "int32_t *d_lag", "float *d_period", "float *d_cmnd", "void *stream"]
    assert re.search(r"\*\s+ev_pitch_yin\s+<-\s+no counterpart: the reference never measures pitch; librosa\.yin is the model", header)
    assert re.search(r"#define\s+EV_ABI_VERSION\s+4\b.*ev_pitch_yin", header), "the ABI line's additions list"
    assert "ev_pitch_yin" in _lib.EXPORTS and hasattr(_lib.Engine, "pitch_yin")
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, "ev_pitch_yin"), "ev_pitch_yin is not exported by the built library"
    assert len(lib.ev_pitch_yin.argtypes) == 14
    nm = "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        syms = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\sT\s+ev_pitch_yin\b", syms)


def test_the_kernel_has_no_scratch():
    import importlib.util

    spec = importlib.util.spec_from_file_location("code_object", os.path.join(REPO, "tools", "code_object.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain is not installed")
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    ks = [k for k in co.kernels(_lib.LIB_PATH) if k["demangled"].startswith("pitch_yin_kernel")]
    assert len(ks) == 1, "one kernel, one launch"
    k = ks[0]
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 64, k
