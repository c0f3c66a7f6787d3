"""The host side of speech rate and pauses, on the CPU: the restatement (tests/speech_rate_ref.py) against its plain form, the ground truth of the
burst generator, every mutant against the restatement on its named case, the header's ABI line and the library's symbols and code object, the
``audio`` functions through ``rows=``, the JSON of ``--prosody_report --rhythm`` and ``--evaluate_pairs --rhythm`` with the device calls replaced,
and the argument errors of the Python layer.

Ground truth: bursts of 9-13 frames, gaps of 12-19 frames, a 1e-4 noise floor, H = 64, W in {128, 192, 256}, 25 dB / 2 dB, min_pause 8,
min_sound 3, rank_fraction 0.01, four seeds: restatement and plain form count exactly the 14 bursts as nuclei and the 3 interior gaps as pauses;
the least decision margin over the twelve rows is 2.5e-5 (this module's margin also holds every frame's power against ref, not its rank
neighbours alone); the plain form's power stands within 1.1e-15 of the restatement's.
"""
import argparse
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import speech_rate_ref as R
import voice_stubs
from emojivoice_amd import _lib, audio, cli
from emojivoice_amd._lib import EvLibraryError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = R.H0


def rows_ref(x, lengths, voiced, W, Hh, power_floor, rank_fraction, silence_ratio, dip_ratio, min_pause, min_sound):
    """The per-batch measurement ``audio.speech_rate`` takes as ``rows=``, from the restatement."""
    par = dict(power_floor=power_floor, rank_fraction=rank_fraction, silence_db=-10.0 * math.log10(silence_ratio), dip_db=10.0 * math.log10(dip_ratio),
               min_pause=min_pause, min_sound=min_sound)
    r = R.speech_rate(x.numpy(), None if lengths is None else [int(v) for v in lengths], audio.intensity_window(W), Hh, par,
                      voiced=None if voiced is None else voiced.numpy())
    return tuple(torch.from_numpy(r[k]) for k in ("power", "mark", "stat", "count"))


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_restatement_against_its_plain_form(name):
    a, b = R.case_ref(name), R.case_ref(name, plain=True)
    e = R.rel_err(a["power"], b["power"])
    print(f"\nspeech rate host {name}: power of the restatement against np.sum {e:.3e}  least margin {a['margin'].min():.3e}")
    assert e <= 1e-12 and a["margin"].min() >= 1e-6
    assert np.array_equal(a["mark"], b["mark"]) and np.array_equal(a["count"], b["count"]), "selection on bits = np.sort; the same decisions"
    assert R.rel_err(a["stat"], b["stat"]) <= 1e-12


@pytest.mark.parametrize("W", [128, 192, 256])
def test_the_generator_counts_its_bursts_and_gaps(W):
    worst = 1.0
    for seed in range(4):
        x, nb, ng = R.bursts(H, seed=seed)
        for plain in (False, True):
            r = R.speech_rate(x[None], None, np.kaiser(W, 20.24), H, plain=plain)
            assert (nb, ng) == (14, 3) and r["count"][0, 5] == nb and r["count"][0, 2] == ng, (W, seed, plain, r["count"].tolist())
        worst = min(worst, float(r["margin"][0]))
    print(f"\nspeech rate ground truth W = {W}: 14 nuclei and 3 pauses on four seeds, least margin {worst:.3e}")
    assert worst >= 1e-6


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_differs_on_its_named_case(mutant):
    name = R.MUTANT_CASE[mutant]
    far, differ = R.mutant_distance(R.case_ref(name), R.case_ref(name, mutant=mutant))
    print(f"\nspeech rate mutant {mutant} on {name}: {far:.3e} from the restatement; marks or counts differ: {differ}")
    assert far > 1e-9 or differ


def test_selection_steps_and_statistics_on_hand_made_contours():
    P = np.array([5.0, 1.0, 4.0, 4.0, 0.0, 2.0, 3.0])
    for k in range(7):
        assert R.select(P, k, False) == R.select(P, k, True) == sorted(P, reverse=True)[k]
    f = np.array([1, 0, 0, 1, 0, 0, 0, 1, 1, 0], dtype=bool)
    assert R.step_a(f, 3).tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1, 0], "a run of 2 < 3 is filled, one of 3 and the trailing one are not"
    assert R.step_b(R.step_a(f, 3), 3).tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0], "then the sounding run of 2 < 3 goes"
    par = dict(R.PAR, rank_fraction=0.0, min_pause=1, min_sound=1)
    r = R.decide(np.array([0.0, 9.0, 9.0, 0.0, 0.0, 0.0, 8.0, 1.0, 9.0, 0.0, 7.0, 0.0]), par)
    assert r["count"].tolist() == [12, 6, 2, 4, 4, 4, 1, 1], "pauses of 3 and 1 frames; the plateau's first frame is the candidate, its second is none"
    assert r["cand"] == [1, 6, 8, 10] and r["stat"][2] == 2.0 and r["stat"][3] == math.sqrt(2 * 10 - 16) / 2
    v = np.ones(12, np.uint8)
    v[8] = 0
    assert R.decide(np.array([0.0, 9.0, 9.0, 0.0, 0.0, 0.0, 8.0, 1.0, 9.0, 0.0, 7.0, 0.0]), par, voiced=v)["count"][4:6].tolist() == [4, 3]


# ---- 2. the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_abi_line_symbols_and_code_object():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        head = f.read()
    line = next(l for l in head.splitlines() if l.startswith("#define EV_ABI_VERSION"))
    assert re.match(r"#define EV_ABI_VERSION 4\b", line) and "ev_load_speech_rate, ev_speech_rate" in line
    assert "int ev_load_speech_rate(ev_handle *h, const double *window /* HOST (W) */, int W, int H);" in head and "int ev_speech_rate(" in head
    assert {"ev_load_speech_rate", "ev_speech_rate"} <= set(_lib.EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert lib.ev_abi_version() == 4 and lib.ev_load_speech_rate and lib.ev_speech_rate
    spec = importlib.util.spec_from_file_location("code_object", os.path.join(REPO, "tools", "code_object.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain is not installed")
    ks = {k["demangled"].split("(")[0]: k for k in co.kernels(_lib.LIB_PATH)}
    for name in ("speech_power_kernel", "speech_rate_rows_kernel"):
        k = ks[name]
        print(f"\n{name}: {k['vgpr_count']} VGPR, {k['sgpr_count']} SGPR")
        assert (k["sgpr_spill_count"], k["vgpr_spill_count"], k["private_segment_fixed_size"]) == (0, 0, 0), k


# ---- 3. audio ----------------------------------------------------------------------------------------------------------------------------------
def test_window_and_geometry():
    assert np.array_equal(audio.intensity_window(128), np.kaiser(128, 20.24)) and audio.intensity_window(128).dtype == np.float64
    assert audio.speech_rate_geometry(22050) == (1412, 256), "3.2 / 50 s = 1411.2 samples, to the nearest even number"
    assert audio.speech_rate_geometry(16000, 128, 100.0) == (512, 128) and audio.speech_rate_geometry(8000, 64, 75.0) == (342, 64)
    for bad in (dict(sr=0), dict(sr=22050, min_pitch=0.0), dict(sr=22050, min_pitch=10.0), dict(sr=22050, hop_length=100), dict(sr=22050, hop_length=2048)):
        with pytest.raises(ValueError, match="speech_rate_geometry"):
            audio.speech_rate_geometry(**bad)


def _takes():
    """Two takes of the same material at 8 kHz (hop 64): b speaks the same bursts with shorter gaps; c is silence."""
    a = R.bursts(H, seed=1)[0]
    b = R.bursts(H, groups=(4, 3, 4, 3), seed=1, lead=2, trail=2)[0]
    return a, b, np.zeros(40 * H, np.float32)


def test_audio_speech_rate_through_rows():
    a, b, c = _takes()
    x, lens = R.padded([a, b, c], fill=0.0)
    kw = dict(sr=8000, hop_length=H, min_pause_s=0.064, min_sound_s=0.024, rows=rows_ref)     # 8 and 3 frames of 8 ms
    out = audio.speech_rate(torch.from_numpy(x), lengths=lens, **kw)
    assert set(out) == {"nuclei", "pauses", "frames", "sounding", "leading", "trailing", "speech_rate", "articulation_rate", "phonation_ratio",
                        "pause_mean_s", "pause_sd_s", "pause_s", "intensity_db", "mark"}
    W = audio.speech_rate_geometry(8000, H)[0]
    ref = R.speech_rate(x, lens, audio.intensity_window(W), H, dict(R.PAR, min_pause=8, min_sound=3))
    assert W == 512 and np.array_equal(out["mark"].numpy(), ref["mark"]) and out["nuclei"].tolist() == ref["count"][:, 5].tolist()
    assert out["nuclei"].tolist()[:2] == [14, 14] and out["pauses"].tolist() == [3, 3, 0] and out["frames"].tolist() == [len(r) // H for r in (a, b, c)]
    fs = H / 8000.0
    assert float(out["speech_rate"][0]) == 14 / (out["frames"][0].item() * fs) and float(out["articulation_rate"][0]) == 14 / (out["sounding"][0].item() * fs)
    assert float(out["phonation_ratio"][0]) == out["sounding"][0].item() / out["frames"][0].item()
    assert float(out["pause_mean_s"][0]) == ref["stat"][0, 2] * fs and float(out["pause_sd_s"][0]) == ref["stat"][0, 3] * fs
    assert float(out["speech_rate"][2]) == 0.0 and math.isnan(float(out["articulation_rate"][2])), "silence: no nucleus per second; nothing sounds"
    assert float(out["phonation_ratio"][2]) == 0.0
    with np.errstate(divide="ignore"):
        assert np.array_equal(out["intensity_db"].numpy(), 10.0 * np.log10(ref["power"]))
    bad = audio.speech_rate(torch.from_numpy(x), lengths=[0, lens[1], x.shape[1] + 1], **kw)
    assert bad["frames"].tolist()[::2] == [0, 0] and math.isnan(float(bad["speech_rate"][0])) and math.isnan(float(bad["phonation_ratio"][2]))
    one = audio.speech_rate(torch.from_numpy(a), **kw)
    assert one["nuclei"].shape == (1,) and float(one["speech_rate"][0]) == float(out["speech_rate"][0]), "a 1-D input is the same row"
    v = torch.ones(3, x.shape[1] // H, dtype=torch.bool)
    f0 = int(np.flatnonzero(ref["mark"][0] & R.NUC)[3])
    v[0, f0] = False
    cut = audio.speech_rate(torch.from_numpy(x), lengths=lens, voiced=v, **kw)
    assert cut["nuclei"].tolist() == [13, 14, 0] and not cut["mark"][0, f0] & R.NUC
    d = audio.speech_rate_difference({k: v[:1] for k, v in out.items()}, {k: v[1:2] for k, v in out.items()})
    assert set(d) == {"rate_ratio", "articulation_ratio", "pauses_delta", "pause_s_delta"}
    assert float(d["rate_ratio"][0]) == float(out["speech_rate"][1] / out["speech_rate"][0] - 1.0) > 0, "the same bursts in less time: faster"
    assert d["pauses_delta"].tolist() == [0] and float(d["pause_s_delta"][0]) == float(out["pause_s"][1] - out["pause_s"][0])
    assert math.isnan(float(audio.speech_rate_difference({k: v[2:] for k, v in out.items()}, {k: v[:1] for k, v in out.items()})["rate_ratio"][0]))


def test_argument_errors_of_the_python_layer():
    y = torch.zeros(2, 4096)
    for bad, kw in ((y[None], {}), (torch.zeros(2, 0), {}), (y, dict(lengths=[1, 2, 3])), (y, dict(silence_db=0.0)), (y, dict(dip_db=-1.0)),
                    (y, dict(min_pause_s=0.0)), (y, dict(min_sound_s=-1.0)), (y, dict(rank_fraction=1.0)), (y, dict(voiced=torch.ones(2, 3))),
                    (y, dict(hop_length=100)), (torch.zeros(1, 16385 * 64), dict(hop_length=64))):
        with pytest.raises(ValueError, match="speech_rate"):
            audio.speech_rate(bad, **{**dict(sr=8000, rows=rows_ref), **kw})
    with pytest.raises(EvLibraryError, match="no CPU fallback"):
        audio.speech_rate(y, 8000)
    ns = lambda **kw: argparse.Namespace(sample_rate=None, prepare_dataset=None, batch_size=2, **kw)
    with pytest.raises(AssertionError, match="--rhythm is an option of --prosody_report and of --evaluate_pairs"):
        cli.validate_args(ns(rhythm=True, voice_report="x.txt"))
    assert cli.validate_args(ns(rhythm=True, prosody_report="x.txt")).rhythm and cli.validate_args(ns(rhythm=True, evaluate_pairs="x.txt")).rhythm
    assert "--prosody_report clean/filelist.txt --rhythm" in cli.__doc__ and "--evaluate_pairs pairs.txt --rhythm" in cli.__doc__


# ---- 4. the reports ----------------------------------------------------------------------------------------------------------------------------
def _wavs():
    """22.05 kHz at hop 256: a and b of speaker 7 (three bursts, a silence of 0.46 s / 0.35 s, two bursts; b with less silence around them), c of
    speaker 12 (silence)."""
    def take(edge, gap):
        one = R.bursts(256, groups=(3,), seed=1, lead=edge, trail=0, sr=22050.0)[0]
        two = R.bursts(256, groups=(2,), seed=2, lead=0, trail=edge, sr=22050.0)[0]
        return np.concatenate([one, np.zeros(gap * 256, np.float32), two])
    return {"a.wav": take(30, 40), "b.wav": take(12, 30), "c.wav": np.zeros(60 * 256, np.float32)}


def test_prosody_report_with_and_without_rhythm(tmp_path, monkeypatch):
    wavs = _wavs()
    voice_stubs.base(monkeypatch, wavs)
    flist = voice_stubs.filelist(tmp_path, wavs)
    ns = lambda **kw: argparse.Namespace(prosody_report=str(flist), batch_size=2, sample_rate=None, prepare_dataset=None, **kw)
    plain = cli.prosody_report(cli.validate_args(ns()), "cpu")
    plain_bytes = open(f"{flist}.prosody.json", "rb").read()
    assert cli.prosody_report(cli.validate_args(ns(rhythm=False, speech_rate_rows=rows_ref)), "cpu") == plain
    assert open(f"{flist}.prosody.json", "rb").read() == plain_bytes, "without the flag the report keeps every byte"
    rep = cli.prosody_report(cli.validate_args(ns(rhythm=True, speech_rate_rows=rows_ref)), "cpu")
    with open(f"{flist}.prosody.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep)) and "NaN" not in open(f"{flist}.prosody.json").read()
    assert [{k: v for k, v in f.items() if k != "rhythm"} for f in saved["files"]] == plain["files"], "the flag changes no other figure"
    keys = set(cli.RHYTHM_REPORT_KEYS) | {"nuclei", "pause_s"}
    assert cli.RHYTHM_REPORT_KEYS == ("speech_rate", "articulation_rate", "pauses", "pause_mean_s", "phonation_ratio")
    assert all(set(f["rhythm"]) == keys for f in saved["files"])
    a, b, c = (f["rhythm"] for f in saved["files"])
    y = torch.from_numpy(wavs["a.wav"])
    voiced = audio.pitch_yin(y[None], 22050, hop_length=256)["voiced"]
    want = audio.speech_rate(y, 22050, voiced=voiced, rows=rows_ref)
    assert a["speech_rate"] == float(want["speech_rate"][0]) and a["nuclei"] == int(want["nuclei"][0]) and a["pauses"] == 1
    free = audio.speech_rate(y, 22050, rows=rows_ref)
    assert int(free["nuclei"][0]) == 5 and a["nuclei"] <= 5, "five bursts; the tracker's voicing can only remove nuclei"
    assert b["speech_rate"] > a["speech_rate"] and b["phonation_ratio"] > a["phonation_ratio"], "the same bursts with less silence around them"
    assert (c["speech_rate"], c["articulation_rate"], c["pauses"], c["phonation_ratio"], c["nuclei"]) == (0.0, None, 0, 0.0, 0)
    s7, s12 = saved["speakers"]["7"]["rhythm"], saved["speakers"]["12"]["rhythm"]
    assert set(s7) == set(cli.RHYTHM_REPORT_KEYS) | {"pooled_speech_rate"}
    assert abs(s7["speech_rate"] - (a["speech_rate"] + b["speech_rate"]) / 2) < 1e-12 and s7["pauses"] == (a["pauses"] + b["pauses"]) / 2
    secs = sum(f["frames"] for f in saved["files"][:2]) * 256 / 22050.0
    assert abs(s7["pooled_speech_rate"] - (a["nuclei"] + b["nuclei"]) / secs) < 1e-12
    assert s12["articulation_rate"] is None and s12["pooled_speech_rate"] == 0.0
    assert {k: v for k, v in saved["speakers"]["7"].items() if k != "rhythm"} == plain["speakers"]["7"]


def test_evaluate_pairs_with_and_without_rhythm(tmp_path, monkeypatch):
    wavs = _wavs()
    voice_stubs.base(monkeypatch, wavs)
    whole = lambda w: w[: len(w) // 256 * 256]                            # (wav_at_rate hands out whole hops)
    monkeypatch.setattr(cli, "wav_at_rate", lambda path, sr, device: torch.from_numpy(whole(wavs[os.path.basename(str(path))])).unsqueeze(0))
    monkeypatch.setattr(audio, "mel_spectrogram", lambda w, *a, **k: torch.zeros(1, 80, w.shape[1] // 256))
    monkeypatch.setattr(audio, "mel_cepstrum", lambda mel, n=13: torch.zeros(1, n, mel.shape[2]))
    monkeypatch.setattr(audio, "dtw", lambda a, b, fa, fb, metric: {"cost": torch.zeros(a.shape[0], dtype=torch.float64),
                                                                     "steps": torch.ones(a.shape[0], dtype=torch.int32),
                                                                     "path": torch.zeros(a.shape[0], 1, 2, dtype=torch.int32)})
    monkeypatch.setattr(audio, "f0_errors", lambda *a: {"rmse_cents": [None] * a[0].shape[0], "voicing_error": torch.zeros(a[0].shape[0]),
                                                        "voiced_pairs": torch.zeros(a[0].shape[0], dtype=torch.int64)})
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("a.wav|b.wav|7\nb.wav|a.wav|7\nc.wav|a.wav|12\n", encoding="utf-8")
    ns = lambda **kw: argparse.Namespace(evaluate_pairs=str(pairs), batch_size=2, sample_rate=None, prepare_dataset=None, voice_report=None, **kw)
    plain = cli.evaluate_pairs(cli.validate_args(ns()), "cpu")
    plain_bytes = open(f"{pairs}.eval.json", "rb").read()
    assert cli.evaluate_pairs(cli.validate_args(ns(rhythm=False, speech_rate_rows=rows_ref)), "cpu") == plain
    assert open(f"{pairs}.eval.json", "rb").read() == plain_bytes, "without the flag the report keeps every byte"
    rep = cli.evaluate_pairs(cli.validate_args(ns(rhythm=True, speech_rate_rows=rows_ref)), "cpu")
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep)) and "NaN" not in open(f"{pairs}.eval.json").read()
    assert [{k: v for k, v in p.items() if k != "rhythm"} for p in saved["pairs"]] == plain["pairs"], "the flag changes no other figure"
    assert set(saved["overall"]) - {"rhythm"} == set(plain["overall"]) and set(saved) == set(plain)
    p0, p1, p2 = saved["pairs"]
    assert all(set(p["rhythm"]) == {"recorded", "synthesised", "delta"} for p in saved["pairs"])
    assert all(set(p["rhythm"]["delta"]) == {"rate_ratio", "pauses_delta", "pause_s_delta"} for p in saved["pairs"])
    ra, rb = p0["rhythm"]["recorded"], p0["rhythm"]["synthesised"]
    assert p1["rhythm"]["recorded"] == rb and p1["rhythm"]["synthesised"] == ra
    assert p0["rhythm"]["delta"]["rate_ratio"] == rb["speech_rate"] / ra["speech_rate"] - 1.0 > 0, "b says the same in less time"
    assert abs((1 + p0["rhythm"]["delta"]["rate_ratio"]) * (1 + p1["rhythm"]["delta"]["rate_ratio"]) - 1) < 1e-12
    assert p0["rhythm"]["delta"]["pauses_delta"] == -p1["rhythm"]["delta"]["pauses_delta"]
    assert p2["rhythm"]["delta"]["rate_ratio"] is None, "a recording without a nucleus has no rate to compare with"
    o = saved["speakers"]["7"]["rhythm"]
    assert set(o) == {"rate_ratio", "pauses_delta", "pause_s_delta"} and abs(o["pause_s_delta"]) < 1e-12
    assert saved["speakers"]["12"]["rhythm"]["rate_ratio"] is None
