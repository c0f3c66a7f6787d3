"""Silence trimming without a GPU: the numpy restatement (tests/trim_ref.py) against hand-computed cases, the inputs of the GPU test
(their distance from the threshold), the C ABI's declarations and exports, and the parse / JSON shape of --prepare_dataset with the
device calls stubbed."""
import argparse
import json
import os
import re
import subprocess
import wave

import numpy as np
import pytest
import torch

import trim_ref as T
from emojivoice_amd import _lib, audio, cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ev_trim_bounds", "ev_trim_apply"]


def _impulse(n, at):
    x = np.zeros(n, np.float32)
    x[at] = 1.0
    return x


def test_row_shorter_than_half_a_frame():
    x = np.ones(100, np.float32)
    ms = T.frame_ms(x, 2048, 512)                    # one frame, [-1024, 1024): all 100 samples
    assert ms.tolist() == [100.0 / 2048.0]
    assert T.bounds(x, 60, 2048, 512) == (0, 100)    # (f_last + 1) H = 512 is clipped to len
    assert T.bounds(x, 60, 2048, 512, clip_end=False) == (0, 512)


def test_length_an_exact_multiple_of_the_hop():
    x = _impulse(1024, 700)                          # F = 1024, H = 512: frames [-512, 512), [0, 1024), [512, 1536)
    ms = T.frame_ms(x, 1024, 512)
    assert ms.tolist() == [0.0, 1.0 / 1024.0, 1.0 / 1024.0]
    assert T.non_silent(ms, 60).tolist() == [False, True, True]      # 1e-10 against (1 / 1024) * 1e-6 = 9.8e-10
    assert T.bounds(x, 60, 1024, 512) == (512, 1024)
    assert T.frame_ms(x, 1024, 512, centred=False).tolist() == [1.0 / 1024.0, 1.0 / 1024.0, 0.0]     # the mutant: [0, 1024), [512, 1536), [1024, 2048)
    assert T.bounds(x, 60, 1024, 512, centred=False) == (0, 1024)


def test_length_one_past_a_multiple_of_the_hop_and_the_clipped_end():
    x = _impulse(1025, 1024)                         # still 3 frames; only [512, 1536) holds the impulse
    assert T.frame_ms(x, 1024, 512).tolist() == [0.0, 0.0, 1.0 / 1024.0]
    assert T.bounds(x, 60, 1024, 512) == (1024, 1025)                # end = min(1025, 1536)
    assert T.bounds(x, 60, 1024, 512, clip_end=False) == (1024, 1536)
    y = _impulse(2000, 100)                          # frames 0 and 1 hold it: the end is NOT clipped here
    assert T.bounds(y, 60, 1024, 512) == (0, 1024)


def test_all_zero_row_and_no_frame_at_all():
    z = np.zeros(1500, np.float32)
    assert T.bounds(z, 60, 2048, 512) == (0, 1500)   # max(0, 1e-10) > 1e-10 * 1e-6 in every frame
    assert T.bounds(np.ones(1500, np.float32), 0.0, 2048, 512) == (0, 0)      # top_db = 0: not even the loudest frame passes
    assert T.peak(z) == 0.0 and T.peak(np.array([0.25, -0.5], np.float32)) == 0.5


def test_odd_frames_per_hop_are_centred_on_the_hop():
    x = _impulse(1024, 255)                          # F = H = 512: frames [-256, 256), [256, 768), [768, 1280)
    assert T.frame_ms(x, 512, 512).tolist() == [1.0 / 512.0, 0.0, 0.0]
    assert T.bounds(x, 60, 512, 512) == (0, 512)
    assert T.bounds(_impulse(1024, 256), 60, 512, 512) == (512, 1024)


def test_apply_restatement():
    x = np.arange(1, 11, dtype=np.float32) / 16
    y, n = T.apply(x, 2, 7, peak_value=0.625, target_peak=0.95, out_len=8)
    g = np.float32(0.95) / np.float32(0.625)
    assert n == 5 and np.array_equal(y[:5], x[2:7] * g) and not y[5:].any() and y.dtype == np.float32
    y, n = T.apply(x, 2, 7, peak_value=0.625, target_peak=0.0, out_len=3)
    assert n == 3 and np.array_equal(y, x[2:5])
    y, n = T.apply(x, 7, 2)
    assert n == 0 and not y.any()


LENGTHS = [1, 63, 1023, 1024, 1025, 5000, 5120, 3 * 2048 + 511]
CONFIGS = [(2048, 512), (1024, 256), (512, 512)]


def test_the_gpu_test_rows_keep_their_distance_from_the_threshold():
    """The rows tests/test_gpu_trim.py compares exactly: every frame at least 1 dB from the threshold, the -50 dB parts kept, and each
    mutant expectation wrong on at least one of them."""
    wrong = {"uncentred": 0, "unclipped": 0}
    for F, H in CONFIGS:
        for n in LENGTHS:
            x, lens = T.three_level_row(n, seed=n)
            assert len(x) == n and sum(lens) == n
            assert T.margin_db(T.frame_ms(x, F, H), 60) >= 1.0, (F, H, n)
            s, e = T.bounds(x, 60, F, H)
            if n >= 4096:                                # (shorter rows: start = f_first H is coarser than their segments)
                assert s <= lens[0] and e >= n - lens[4], "the -50 dB parts are kept"
                assert s > 0, "-80 dB samples are dropped"
            wrong["uncentred"] += T.bounds(x, 60, F, H, centred=False) != (s, e)
            wrong["unclipped"] += T.bounds(x, 60, F, H, clip_end=False) != (s, e)
    assert wrong["uncentred"] > 0 and wrong["unclipped"] > 0


def test_header_declares_and_library_exports_the_new_calls():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    for n in NAMES:
        assert re.search(rf"\bint\s+{n}\s*\(\s*ev_handle\s*\*", header), f"{n} is not declared in include/emojivoice.h"
        assert re.search(rf"\*\s+{n}\s+<-", header), f"{n} is missing from the table of reference counterparts"
        assert n in _lib.EXPORTS
    assert re.search(r"#define\s+EV_ABI_VERSION\s+4\b", header)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported by the built library"
    nm = "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        syms = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for n in NAMES:
            assert re.search(rf"\sT\s+{n}\b", syms), n


def test_python_entry_points_refuse_the_cpu():
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.trim_silence(torch.zeros(4000))
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.peak_normalize(torch.zeros(2, 4000))
    with pytest.raises(ValueError):
        audio.trim_silence(torch.zeros(1, 2, 3))


def test_pcm16_writer_round_trips(tmp_path):
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 1e-5], np.float32)
    cli.write_wav_pcm16(tmp_path / "a.wav", x, 16000)
    with wave.open(str(tmp_path / "a.wav"), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 16000, len(x))
        q = np.frombuffer(f.readframes(len(x)), "<i2")
    assert q.tolist() == [0, 16384, -16384, 32767, -32767, 32767, 0]


def test_prepare_dataset_parse_and_json_shape(tmp_path, monkeypatch):
    raw = tmp_path / "raw"
    raw.mkdir()
    for name in ("a.wav", "b.wav", "c.wav"):
        (raw / name).write_bytes(b"")                 # (the stub below never opens them)
    flist = tmp_path / "raw.txt"
    flist.write_text(f"{raw / 'a.wav'}|7|first, text\nraw/b.wav|7|second\n\nraw/c.wav|12|third | with a bar\n", encoding="utf-8")
    entries = cli.parse_filelist(flist)
    assert [(os.path.basename(w), s) for w, s, _ in entries] == [("a.wav", "7"), ("b.wav", "7"), ("c.wav", "12")]
    assert all(os.path.exists(w) for w, _, _ in entries), "relative paths are taken from the filelist's folder"
    two = tmp_path / "two.txt"
    two.write_text("raw/a.wav|only text\n", encoding="utf-8")
    assert cli.parse_filelist(two)[0][1] is None

    seconds = {"a.wav": (100.0, 90.0), "b.wav": (50.0, 40.0), "c.wav": (30.0, 20.5)}
    calls = []

    def fake_prepare(path, sr=22050, top_db=60, peak=0.95, device="cuda"):
        calls.append((os.path.basename(str(path)), sr, top_db, peak))
        s_in, s_out = seconds[os.path.basename(str(path))]
        return torch.full((16,), 0.5), {"start": 3, "end": 19, "seconds_in": s_in, "seconds_out": s_out}

    monkeypatch.setattr(audio, "prepare_recording", fake_prepare)
    out_dir = tmp_path / "clean"
    args = argparse.Namespace(prepare_dataset=str(flist), out_dir=str(out_dir), top_db=40.0, peak=0.9, sample_rate=None)
    rep = cli.prepare_dataset(cli.validate_args(args), None)
    assert calls == [("a.wav", 22050, 40.0, 0.9), ("b.wav", 22050, 40.0, 0.9), ("c.wav", 22050, 40.0, 0.9)]
    with open(f"{flist}.durations.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert set(saved) == {"sample_rate", "top_db", "peak", "files", "speakers", "below_two_minutes", "total_minutes_in", "total_minutes_out"}
    assert [os.path.basename(f["path"]) for f in saved["files"]] == ["a.wav", "b.wav", "c.wav"]
    assert [(f["speaker"], f["seconds_in"], f["seconds_out"]) for f in saved["files"]] == [("7", 100.0, 90.0), ("7", 50.0, 40.0), ("12", 30.0, 20.5)]
    assert saved["speakers"]["7"] == {"files": 2, "minutes": 130.0 / 60.0, "below_two_minutes": False}
    assert saved["speakers"]["12"] == {"files": 1, "minutes": 20.5 / 60.0, "below_two_minutes": True}
    assert saved["below_two_minutes"] == ["12"]
    assert saved["total_minutes_in"] == 3.0 and abs(saved["total_minutes_out"] - 150.5 / 60.0) < 1e-12
    lines = (out_dir / "filelist.txt").read_text(encoding="utf-8").splitlines()
    assert [ln.split("|", 1)[1] for ln in lines] == ["7|first, text", "7|second", "12|third | with a bar"]
    for ln, f in zip(lines, saved["files"]):
        p = ln.split("|")[0]
        assert p == f["out"] and os.path.isabs(p) and os.path.dirname(p) == str(out_dir.resolve())
        with wave.open(p, "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 22050, 16)
            assert set(np.frombuffer(w.readframes(16), "<i2").tolist()) == {16384}

    dup = tmp_path / "dup.txt"
    (tmp_path / "other").mkdir()
    (tmp_path / "other" / "a.wav").write_bytes(b"")
    dup.write_text("raw/a.wav|1|x\nother/a.wav|1|y\n", encoding="utf-8")
    with pytest.raises(SystemExit, match="base name"):
        cli.prepare_dataset(argparse.Namespace(prepare_dataset=str(dup), out_dir=str(out_dir), top_db=60.0, peak=0.95, sample_rate=None), None)
    with pytest.raises(AssertionError, match="out_dir"):
        cli.validate_args(argparse.Namespace(prepare_dataset=str(flist), out_dir=None, top_db=60.0, peak=0.95, sample_rate=None))
