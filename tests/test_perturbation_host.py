"""The perturbation measures on the CPU: what the restatement (tests/perturbation_ref.py) itself recovers from synthetic pulses, the input
conditions of every case tests/test_gpu_perturbation.py runs on the device, the mutants, and the host side (audio.hnr_db,
audio.perturbation_statistics, the --perturbation key sets).  Needs no GPU and, but for the export test, no library.

Measured on the restatement at 22050 Hz, H 256, W 1024, n_cycles 3, lags from tests/pitch_ref.py, 12000 samples, medians over the voiced frames with
a counted pair (``MEASURED``; DESIGN section 3.21 records them):
    pulses(120 Hz, 0, 0)            local jitter 0.00561 %    local shimmer 0.0454 %    HNR 44.7 dB
    pulses(120 Hz, sigma 1 %, 0)    local jitter 0.711 %      (the mean to expect of |N(0, s) - N(0, s)| is 2 sigma / sqrt(pi) = 1.128 %)
    pulses(120 Hz, 0, sigma 5 %)    local shimmer 5.05 %      (the mean to expect is 5.64 %)
    harmonic_tone(147)              jitter 0.000 %, shimmer 0.000 %, HNR 90 dB (the clip) on the interior frames
The gates: the clean row at ten times the measured medians; the jittered and the shimmered row within +-40 % of their own measured medians.  They are
derived from the restatement, never from the device.
"""
import os
import re

import numpy as np
import pytest
import torch

import perturbation_ref as R
import pitch_ref
import stoi_ref
import voice_stubs
from emojivoice_amd import _lib, audio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = {"clean_jitter": 5.61e-5, "clean_shimmer": 4.54e-4, "jitter_row": 7.107e-3, "shimmer_row": 5.047e-2}
_ROWS = {}


def measured(key, y):
    """(frame (F, 8), count (F, 4), voiced (F,)) of one row at the audio geometry, at the restatement of YIN's lags; computed once."""
    if key not in _ROWS:
        y = np.asarray(y, np.float32)[None]
        lag = pitch_ref.pitch_yin(y, None, **pitch_ref.STD)["lag"]
        r = R.batch(y, None, lag, R.AUDIO_GEO)
        _ROWS[key] = (r["frame"][0], r["count"][0], lag[0] > 0)
    return _ROWS[key]


def medians(key, y):
    fr, ct, v = measured(key, y)
    jit, shim = fr[v & (ct[:, 1] > 0), 0], fr[v & (ct[:, 2] > 0), 2]
    return float(np.median(jit)), float(np.median(shim)), float(np.median(R.hnr_db(fr[v, 4]))), int(v.sum()), int((ct[v, 0] == 6).sum())


# ---- what the restatement recovers ----------------------------------------------------------------------------------------------------------------
def test_clean_pulses_have_almost_no_jitter_or_shimmer():
    jit, shim, hnr, nv, six = medians("clean", R.perturbed_pulses(12000, 120.0, 0.0, 0.0, seed=1))
    print(f"\nperturbation pulses(120 Hz, 0, 0): local jitter {100 * jit:.5f} %  local shimmer {100 * shim:.5f} %  HNR {hnr:.2f} dB  voiced {nv}  all six periods {six}")
    assert nv >= 40 and six == nv
    assert jit <= 10 * MEASURED["clean_jitter"] and shim <= 10 * MEASURED["clean_shimmer"] and hnr > 30.0


def test_jittered_pulses():
    jit, shim, hnr, nv, six = medians("jitter", R.perturbed_pulses(12000, 120.0, 0.01, 0.0, seed=1))
    print(f"\nperturbation pulses(120 Hz, sigma 1 %, 0): local jitter {100 * jit:.5f} % (2 sigma / sqrt(pi) = 1.128 %)  local shimmer {100 * shim:.5f} %  "
          f"HNR {hnr:.2f} dB  voiced {nv}  all six periods {six}")
    assert nv >= 30 and 0.6 * MEASURED["jitter_row"] <= jit <= 1.4 * MEASURED["jitter_row"]
    assert 0.4 * 0.01128 <= jit <= 1.2 * 0.01128, "a median of |differences| over a handful of pairs lies under the mean 2 sigma / sqrt(pi), not far"


def test_shimmered_pulses():
    jit, shim, hnr, nv, six = medians("shimmer", R.perturbed_pulses(12000, 120.0, 0.0, 0.05, seed=1))
    print(f"\nperturbation pulses(120 Hz, 0, sigma 5 %): local shimmer {100 * shim:.5f} % (2 sigma / sqrt(pi) = 5.64 %)  local jitter {100 * jit:.5f} %  "
          f"HNR {hnr:.2f} dB  voiced {nv}  all six periods {six}")
    assert nv >= 40 and 0.6 * MEASURED["shimmer_row"] <= shim <= 1.4 * MEASURED["shimmer_row"]
    assert 0.6 * 0.0564 <= shim <= 1.4 * 0.0564


def test_a_harmonic_tone_is_perfectly_regular():
    fr, ct, v = measured("tone", pitch_ref.harmonic_tone(147.0, 12000))
    it = pitch_ref.interior_frames(len(v), 12000)
    assert v[it].all() and (ct[it, 0] == 6).all()
    jit, shim, hnr = np.median(fr[it, 0]), np.median(fr[it, 2]), np.median(R.hnr_db(fr[it, 4]))
    print(f"\nperturbation harmonic_tone(147): local jitter {100 * jit:.6f} %  local shimmer {100 * shim:.6f} %  HNR {hnr:.1f} dB over {int(it.sum())} interior frames")
    assert round(100 * jit, 3) == 0 and round(100 * shim, 3) == 0 and hnr > 60.0


def test_speech_like_row_finds_its_periods():
    fr, ct, v = measured("speech", stoi_ref.speech_like(12000, 1, fs=22050))
    six = int((ct[v, 0] == 6).sum())
    print(f"\nperturbation speech_like(12000, 1): {six} of {int(v.sum())} voiced frames found all six periods; median local jitter "
          f"{100 * np.median(fr[v & (ct[:, 1] > 0), 0]):.3f} %, HNR {np.median(R.hnr_db(fr[v, 4])):.1f} dB")
    assert v.sum() >= 20 and six >= 0.8 * v.sum(), "a glide of +-20 % at 0.7 Hz moves the period by under 1 % per cycle: the +-1/8 window holds it"


# ---- the cases of the device test ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    out = dict(R.cases())
    x, lens = R.audio_rows()
    out["audio"] = (x, lens, pitch_ref.pitch_yin(x, lens, **pitch_ref.STD)["lag"], R.AUDIO_GEO)
    return out


def test_float64_and_longdouble_take_equal_decisions_on_every_frame_of_the_device_cases(cases):
    for name, (x, lens, lag, g) in cases.items():
        a, b = R.batch(x, lens, lag, g), R.batch(x, lens, lag, g, dtype=np.longdouble)
        R.input_conditions(a, b, name)
        e = R.err(a["frame"], b["frame"].astype(np.float64))
        print(f"perturbation {name}: float64 against longdouble {e:.3e}; least pair margin {a['pair_margin']:.2e}, floor margin {a['floor_margin']:.2e}, "
              f"ties {a['ties']}, periods {int(a['count'][..., 0].sum())}")
        assert e <= 1e-11, "the restatement's own float64 error is far inside the device's margin of 1e-9"
        assert (a["count"][..., 0] > 0).any() or name == "one"
    assert cases["plateau"][0].shape[0] == 2 and R.batch(*cases["plateau"])["ties"] >= 1
    x, lens, lag, g = cases["small-nc3"]
    assert [R.frames(n, g.H) % 4 for n in lens] == [3, 0, 1]
    assert (x[0, lens[0]:] == R.GARBAGE).all()


def test_each_mutant_moves_some_output(cases):
    names = ("small-nc3", "hand", "plateau")
    base = {n: R.batch(*cases[n]) for n in names}
    for m in R.MUTANTS:
        moved = {n: R.err(R.batch(*cases[n], mutant=m)["frame"], base[n]["frame"]) for n in names}
        print(f"perturbation mutant {m}: moves d_frame by {', '.join(f'{n} {v:.3e}' for n, v in moved.items())} (relative to max(|ref|, 1))")
        assert max(moved.values()) >= 1e-4, m


def test_lane_sum_is_the_documented_order():
    g = np.random.default_rng(3)
    for W in (8, 64, 70, 128, 1000):
        v = g.standard_normal(W)
        lanes = [0.0] * 64
        for j in range(W):
            lanes[j % 64] = lanes[j % 64] + v[j]
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[i] + lanes[i ^ o] for i in range(64)]
        assert R.lane_sum(v, np.float64) == lanes[0] and len(set(lanes)) == 1


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------
def test_hnr_db():
    r = torch.tensor([0.5, 0.99, 0.0, 1.0, -0.3, 1.7, 0.9090909090909091], dtype=torch.float64)
    got = audio.hnr_db(r)
    want = [0.0, 10 * np.log10(99.0), 10 * np.log10(1e-6 / (1 - 1e-6)), 10 * np.log10((1 - 1e-9) / 1e-9), 10 * np.log10(1e-6 / (1 - 1e-6)),
            10 * np.log10((1 - 1e-9) / 1e-9), 10.0]
    assert got.dtype == torch.float64 and np.allclose(got.numpy(), want, rtol=0, atol=1e-6)
    assert abs(float(got[2]) + 60.0) < 1e-4 and abs(float(got[3]) - 90.0) < 1e-6
    assert np.allclose(R.hnr_db(r.numpy()), got.numpy(), rtol=0, atol=1e-6)


def test_perturbation_statistics_against_hand_made_tensors():
    g = np.random.default_rng(5)
    B, F = 3, 40
    vals = {k: g.uniform(0.0, 0.2, (B, F)) for k in ("jitter", "rap", "shimmer", "shimmer_db")}
    vals["r"] = g.uniform(-0.1, 1.1, (B, F))
    count = g.integers(0, 3, (B, F, 4)).astype(np.int32)
    voiced = g.random((B, F)) < 0.7
    voiced[2] = False
    lens = [40, 23, 40]
    pt = {k: torch.from_numpy(v) for k, v in vals.items()}
    pt["count"] = torch.from_numpy(count)
    st = audio.perturbation_statistics(pt, torch.from_numpy(voiced), lengths=lens)
    use = voiced & (np.arange(F)[None, :] < np.array(lens)[:, None])
    assert st["frames"].tolist() == use.sum(axis=1).tolist() and st["frames"].dtype == torch.int64 and st["frames"][2] == 0
    for name, v, k in (("jitter_pct", 100 * vals["jitter"], 1), ("rap_pct", 100 * vals["rap"], 3), ("shimmer_pct", 100 * vals["shimmer"], 2),
                       ("shimmer_db", vals["shimmer_db"], 2), ("hnr_db", R.hnr_db(vals["r"]), None)):
        ok = use & (count[..., k] > 0) if k is not None else use
        assert st["used"][name].tolist() == ok.sum(axis=1).tolist()
        assert st[name].dtype == torch.float64 and torch.isnan(st[name][2]) and float(st["sums"][name][2]) == 0.0
        for b in range(2):
            assert abs(float(st[name][b]) - v[b][ok[b]].mean()) < 1e-9 and abs(float(st["sums"][name][b]) - v[b][ok[b]].sum()) < 1e-8
        if k is not None:
            assert (ok.sum(axis=1) < use.sum(axis=1))[:2].all(), "frames without a counted pair are left out"
    one = audio.perturbation_statistics({k: v[0] for k, v in pt.items()}, torch.from_numpy(voiced[0]))
    assert one["frames"].tolist() == [int(voiced[0].sum())]
    assert tuple(audio.PERTURBATION_FIGURES) == ("jitter_pct", "rap_pct", "shimmer_pct", "shimmer_db", "hnr_db")
    with pytest.raises(ValueError, match="perturbation_statistics"):
        audio.perturbation_statistics(pt, torch.from_numpy(voiced[:, :5]))
    with pytest.raises(ValueError, match="perturbation_statistics"):
        audio.perturbation_statistics(pt, torch.from_numpy(voiced), lengths=[1, 2])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_ev_perturbation():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    assert re.search(r"\bint ev_perturbation\(ev_handle \*h,", header) and "ev_perturbation" in _lib.EXPORTS
    assert "ev_perturbation" in re.search(r"#define EV_ABI_VERSION 4 .*", header).group(0), "the additions list of the ABI line"
    for word in ("UNVOICED", "period_factor", "amplitude_factor", "lowest index", "tau0 / 8", "power_floor^2"):
        assert word in header
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, "ev_perturbation") and lib.ev_abi_version() == 4


# ---- the CLI, with the device calls stubbed by the restatements ------------------------------------------------------------------------------------------
def test_voice_report_perturbation_json_shape_and_validate_args(tmp_path, monkeypatch):
    import argparse
    import json

    from emojivoice_amd import cli

    wavs = {"a.wav": R.perturbed_pulses(6000, 120.0, 0.01, 0.05, seed=20), "b.wav": R.perturbed_pulses(5000, 150.0, 0.005, 0.1, seed=21),
            "c.wav": np.zeros(3000, np.float32)}
    flist = voice_stubs.filelist(tmp_path, wavs)
    fake_yin, fake_pt = voice_stubs.base(monkeypatch, wavs), voice_stubs.perturbation(monkeypatch)
    ns = lambda **kw: argparse.Namespace(voice_report=str(flist), batch_size=2, sample_rate=None, prepare_dataset=None, **kw)
    plain = cli.voice_report(cli.validate_args(ns()), "cpu")
    rep = cli.voice_report(cli.validate_args(ns(perturbation=True)), "cpu")
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    figs = set(audio.PERTURBATION_FIGURES)
    extra = figs | {"perturbation_frames"}
    assert extra == {"jitter_pct", "rap_pct", "shimmer_pct", "shimmer_db", "hnr_db", "perturbation_frames"}
    assert saved == json.loads(json.dumps(rep)) and set(saved) == set(plain) == {"sample_rate", "hop_length", "files", "speakers", "overall"}
    old = {"path", "speaker", "seconds", "frames", "voiced_frames"} | set(audio.VOICE_QUALITY_FIGURES)
    assert [set(f_) for f_ in plain["files"]] == [old] * 3 and [set(f_) for f_ in saved["files"]] == [old | extra] * 3
    assert set(plain["overall"]) | extra == set(saved["overall"]) == set(saved["speakers"]["7"]) and not extra & set(plain["overall"])
    assert all(saved["files"][i][k] == plain["files"][i][k] for i in range(3) for k in old), "the flag changes none of the other figures"
    a, b, c = saved["files"]
    assert c["perturbation_frames"] == 0 and all(c[k] is None for k in figs) and a["perturbation_frames"] > 3 and b["perturbation_frames"] > 3
    stats = {}
    for name in ("a.wav", "b.wav"):
        y = torch.from_numpy(wavs[name])[None]
        n = len(wavs[name])
        stats[name] = audio.perturbation_statistics(fake_pt(y, lengths=[n]), fake_yin(y, lengths=[n])["voiced"], [R.frames(n, 256)])
    assert a["perturbation_frames"] == int(stats["a.wav"]["frames"][0])
    for k in figs:
        assert abs(a[k] - float(stats["a.wav"][k][0])) < 1e-9
        na, nb = int(stats["a.wav"]["used"][k][0]), int(stats["b.wav"]["used"][k][0])
        pooled = (a[k] * na + b[k] * nb) / (na + nb)
        assert abs(saved["speakers"]["7"][k] - pooled) < 1e-9 and saved["overall"][k] == saved["speakers"]["7"][k] and saved["speakers"]["12"][k] is None
    assert saved["speakers"]["7"]["perturbation_frames"] == a["perturbation_frames"] + b["perturbation_frames"] == saved["overall"]["perturbation_frames"]
    with pytest.raises(AssertionError, match="--perturbation"):
        cli.validate_args(argparse.Namespace(perturbation=True, evaluate_pairs=None, voice_report=None, sample_rate=None, prepare_dataset=None))
    cli.validate_args(argparse.Namespace(perturbation=True, evaluate_pairs="pairs.txt", voice_report=None, batch_size=2, sample_rate=None, prepare_dataset=None))
