"""CPU-side checks of the loudness path: ``audio.k_weighting`` against the BS.1770-4 table, the standard's 997 Hz tone through the numpy
restatement (tests/loudness_ref.py) with those coefficients, the gate margins and known figures of the rows tests/test_gpu_loudness.py runs on
the device, ``audio.loudness_gain`` / ``loudness_normalize`` arithmetic, the JSON of ``--loudness_report`` with the device calls stubbed, the
argument checks, and the C ABI's declaration and export.
"""
import argparse
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import loudness_ref as R
from emojivoice_amd import _lib, audio, cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_weighting_at_48k_is_the_standards_table():
    k = audio.k_weighting(48000)
    assert k.dtype == np.float64 and k.shape == (10,)
    err = float(np.max(np.abs(k - R.TABLE_48K)))
    print(f"\nLOUDNESS k_weighting(48000) against the table: max abs diff {err:.3e}")
    assert err <= 1e-12
    for sr in (8000, 16000, 22050, 44100, 48000, 96000):
        c = audio.k_weighting(sr)
        for st in (0, 1):
            a1, a2 = c[5 * st + 3], c[5 * st + 4]
            assert abs(a2) < 1 and abs(a1) < 1 + a2, f"stage {st + 1} at {sr} Hz must be stable"
    assert audio.ABSOLUTE_GATE == R.ABS_GATE


def test_the_standards_tone_reads_minus_3_01_lufs():
    """A 997 Hz full-scale sine: -3.01 LUFS at 48 kHz (the standard's own check), and -2.98 at 22.05 kHz, the bilinear design's known offset
    there (the shelf's warped response at 997 Hz) — asserted so that a silent change of design shows."""
    l48 = float(R.loudness(R.sine(997.0, 5.0, 48000), None, 4800, audio.k_weighting(48000))["integrated"][0])
    l22 = float(R.loudness(R.sine(997.0, 5.0, 22050), None, 2205, audio.k_weighting(22050))["integrated"][0])
    print(f"\nLOUDNESS 997 Hz full scale: {l48:.4f} LUFS at 48 kHz, {l22:.4f} LUFS at 22.05 kHz")
    assert abs(l48 - (-3.01)) <= 0.01
    assert abs(l22 - (-2.98)) <= 0.01


def test_device_cases_have_their_known_figures_and_margins():
    k = audio.k_weighting(22050)
    for S in R.GATING_S:
        r = R.loudness(R.gating_row(S), None, S, k)
        assert tuple(r["counts"][0]) == R.GATING_COUNTS[S], S
        assert r["margin"][0] >= 3.0 and abs(r["integrated"][0] - R.GATING_LUFS[S]) <= 0.01, (S, r["margin"][0], r["integrated"][0])
        assert r["sub"][0].min() < 1e-8 * r["sub"][0].max(), "the near-silent segment"
    x, lens = R.edge_rows()
    r = R.loudness(x, lens, R.EDGE_S, k)
    assert r["counts"][:, 0].tolist() == [0, 1, 1, 1, 0, 12, 13, 13, 30, 0, 0]
    assert np.all(r["margin"] >= 1e-3)
    x, lens = R.realistic_rows()
    r = R.loudness(x, lens, 2205, k)
    assert r["counts"].tolist() == [[7, 7, 7], [19, 15, 15], [27, 27, 15]] and np.all(r["margin"] >= 1e-3)
    z = R.loudness(np.zeros(8 * 64, np.float32), None, 64, k)
    assert z["counts"].tolist() == [[5, 0, 0]] and not z["gated"].any() and z["integrated"][0] == -np.inf


def test_restatement_pads_bad_rows_and_block_formula_matches():
    k = audio.k_weighting(22050)
    x, lens = R.edge_rows()
    r = R.loudness(x, lens, R.EDGE_S, k)
    assert not r["sub"][9].any() and not r["sub"][10].any() and not r["counts"][9:].any()
    assert np.array_equal(R.block_formula(r["sub"], r["counts"], R.EDGE_S), r["block"])
    alone = R.loudness(x[8, :lens[8]], None, R.EDGE_S, k)
    assert np.array_equal(alone["sub"][0], r["sub"][8, :alone["sub"].shape[1]]), "the garbage behind a row does not enter"


def test_loudness_gain_and_cap_arithmetic():
    loud = torch.tensor([-20.0, -30.0, float("-inf"), -23.0, -26.0], dtype=torch.float64)
    peak = torch.tensor([0.5, 0.5, 0.0, 0.2, 0.95])
    gain, gain_db, capped = audio.loudness_gain(loud, peak, -23.0, 0.95)
    assert capped.tolist() == [False, True, False, False, True]
    want = [10 ** (-3 / 20), 0.95 / 0.5, 1.0, 1.0, 1.0]
    assert np.allclose(gain.numpy(), want, rtol=1e-7, atol=0)               # (the peaks are float32)
    assert np.allclose(gain_db.numpy(), [-3.0, 20 * math.log10(1.9), 0.0, 0.0, 0.0], atol=1e-6)
    g2, _, c2 = audio.loudness_gain(loud, peak, -23.0, None)
    assert not c2.any() and abs(float(g2[1]) - 10 ** (7 / 20)) < 1e-12, "no ceiling, no cap"


def test_loudness_normalize_applies_the_gain(monkeypatch):
    y = torch.tensor([[0.5, -0.25, 0.1, 9.0], [0.0, 0.0, 0.0, 0.0], [0.25, -0.5, 0.5, 0.5]])
    monkeypatch.setattr(audio, "loudness", lambda y, sr=22050, lengths=None: {"integrated": torch.tensor([-17.0, float("-inf"), -43.0], dtype=torch.float64)})
    monkeypatch.setattr(audio, "peak_level", lambda y, lengths=None: torch.tensor([0.5, 0.0, 0.5]))
    out, gain_db, capped = audio.loudness_normalize(y, -23.0, 22050, lengths=[3, 4, 4], peak_ceiling=0.95)
    assert capped.tolist() == [False, False, True] and out.dtype == torch.float32
    assert np.allclose(gain_db.numpy(), [-6.0, 0.0, 20 * math.log10(1.9)], atol=1e-6)
    g0 = np.float32(10 ** (-6 / 20))
    assert np.array_equal(out[0].numpy(), (y[0].numpy() * g0) * np.array([1, 1, 1, 0], np.float32)), "zeros past the row's length"
    assert np.array_equal(out[1].numpy(), y[1].numpy()) and abs(float(out[2].abs().max()) - 0.95) < 1e-6


def test_loudness_report_json_shape(tmp_path, monkeypatch):
    folder = tmp_path / "clean"
    folder.mkdir()
    for name in ("a.wav", "b.wav", "c.wav", "d.wav", "e.wav"):
        (folder / name).write_bytes(b"")                 # (the stubs below never open them)
    flist = tmp_path / "clean" / "filelist.txt"
    flist.write_text("a.wav|7|one\nb.wav|7|two\nc.wav|7|three\n\nd.wav|12|four\ne.wav|12|five\n", encoding="utf-8")
    lufs = {"a.wav": -20.0, "b.wav": -21.0, "c.wav": -28.0, "d.wav": -23.0, "e.wav": float("-inf")}
    samples = {"a.wav": 22050, "b.wav": 44100, "c.wav": 11025, "d.wav": 33075, "e.wav": 4000}
    order = []

    def fake_load(path, sr=22050, device="cuda"):
        name = os.path.basename(str(path))
        order.append(name)
        y = torch.zeros(1, samples[name])
        y[0, 0] = float(list(samples).index(name))        # tags the row
        return y

    def fake_loudness(y, sr=22050, lengths=None):
        names = [list(samples)[int(v)] for v in y[:, 0]]
        assert sr == 22050 and list(lengths) == [samples[n] for n in names] and y.shape[1] == max(lengths)
        nb = max(y.shape[1] // 2205 - 3, 0)
        mom = torch.full((len(names), nb), float("-inf"), dtype=torch.float64)
        for r, n in enumerate(names):
            if math.isfinite(lufs[n]):
                mom[r, 0], mom[r, 1] = lufs[n] - 1.0, lufs[n] + 2.0
        return {"integrated": torch.tensor([lufs[n] for n in names], dtype=torch.float64), "momentary": mom,
                "blocks": torch.tensor([max(samples[n] // 2205 - 3, 0) for n in names], dtype=torch.int32),
                "gated_blocks": torch.zeros(len(names), dtype=torch.int32), "sub_energy": None}

    def fake_peak(y, lengths=None):
        return torch.tensor([0.0 if list(samples)[int(v)] == "e.wav" else 0.5 for v in y[:, 0]])

    monkeypatch.setattr(audio, "load_audio", fake_load)
    monkeypatch.setattr(audio, "loudness", fake_loudness)
    monkeypatch.setattr(audio, "peak_level", fake_peak)
    args = cli.validate_args(argparse.Namespace(loudness_report=str(flist), batch_size=3, sample_rate=None, prepare_dataset=None))
    rep = cli.loudness_report(args, "cpu")
    assert order == ["a.wav", "b.wav", "c.wav", "d.wav", "e.wav"]
    with open(f"{flist}.loudness.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert set(saved) == {"sample_rate", "outlier_lu", "files", "speakers"} and saved["sample_rate"] == 22050 and saved["outlier_lu"] == 3.0
    assert [set(f) for f in saved["files"]] == [{"path", "speaker", "seconds", "integrated_lufs", "max_momentary_lufs", "peak_dbfs"}] * 5
    a, b, c, d, e = saved["files"]
    assert (a["speaker"], a["seconds"], a["integrated_lufs"], a["max_momentary_lufs"]) == ("7", 1.0, -20.0, -18.0)
    assert abs(a["peak_dbfs"] - 20 * math.log10(0.5)) < 1e-12 and b["seconds"] == 2.0 and c["max_momentary_lufs"] == -26.0
    assert (e["integrated_lufs"], e["max_momentary_lufs"], e["peak_dbfs"]) == (None, None, None), "no block, silence: nulls, not -Infinity"
    s7, s12 = saved["speakers"]["7"], saved["speakers"]["12"]
    assert set(s7) == {"files", "measured", "mean", "std", "min", "max", "outliers"}
    assert (s7["files"], s7["measured"], s7["mean"], s7["min"], s7["max"]) == (3, 3, -23.0, -28.0, -20.0)
    assert abs(s7["std"] - math.sqrt((9 + 4 + 25) / 3)) < 1e-12
    assert [os.path.basename(p) for p in s7["outliers"]] == ["c.wav"], "c is 5 LU under the mean, a exactly 3 LU over it (not MORE than 3)"
    assert (s12["files"], s12["measured"], s12["mean"], s12["std"], s12["outliers"]) == (2, 1, -23.0, 0.0, [])
    assert "Infinity" not in open(f"{flist}.loudness.json").read() and "NaN" not in open(f"{flist}.loudness.json").read()

    empty = tmp_path / "empty.txt"
    empty.write_text("\n", encoding="utf-8")
    with pytest.raises(SystemExit, match="no files"):
        cli.loudness_report(argparse.Namespace(loudness_report=str(empty), batch_size=4), "cpu")
    with pytest.raises(AssertionError, match="Batch size"):
        cli.validate_args(argparse.Namespace(loudness_report=str(flist), batch_size=0, sample_rate=None, prepare_dataset=None))


def test_target_lufs_is_validated():
    ns = lambda **kw: argparse.Namespace(**{**dict(prepare_dataset="raw.txt", out_dir="clean", top_db=60.0, peak=0.95, sample_rate=None), **kw})
    assert cli.validate_args(ns(target_lufs=-23.0)).target_lufs == -23.0
    assert cli.validate_args(ns()) is not None, "without the flag nothing new is asked"
    with pytest.raises(AssertionError, match="target_lufs"):
        cli.validate_args(ns(target_lufs=float("nan")))
    with pytest.raises(AssertionError, match="peak"):
        cli.validate_args(ns(target_lufs=-23.0, peak=0.0))
    with pytest.raises(AssertionError, match="sample_rate"):
        cli.validate_args(ns(target_lufs=-23.0, sample_rate=11025))


def test_argument_checks():
    for sr in (22051, 7990, 4000, 0, -48000, 22050.5):
        with pytest.raises(ValueError, match="k_weighting"):
            audio.k_weighting(sr)
    with pytest.raises(ValueError, match="k_weighting"):
        audio.loudness(torch.zeros(2, 4000), sr=22055)
    with pytest.raises(ValueError):
        audio.loudness(torch.zeros(1, 2, 3))
    with pytest.raises(ValueError):
        audio.loudness(np.zeros(4000, np.float32))
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.loudness(torch.zeros(2, 4000))
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.loudness_normalize(torch.zeros(4000))
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.peak_level(torch.zeros(4000))


def test_header_declares_and_library_exports_ev_loudness():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+ev_loudness\s*\(\s*ev_handle\s*\*", header)
    assert re.search(r"\*\s+ev_loudness\s+<-\s+no counterpart; ITU-R BS\.1770-4 is the model", header)
    assert re.search(r"#define\s+EV_ABI_VERSION\s+4\b[^\n]*\bev_loudness\b", header), "the additions list of the ABI comment"
    assert "ev_loudness" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    assert hasattr(_lib.load_library(), "ev_loudness")
