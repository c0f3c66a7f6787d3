"""The host side of SRMR, on the CPU: the restatement (tests/srmr_ref.py) against a plain sequential form of itself in longdouble, the table
design of ``audio.srmr_tables``, the K* rule on hand-made energies, two physical properties of the measure, the limits of ``audio.srmr`` and
the JSON of ``--reverb_report`` and ``--evaluate_pairs --srmr`` with the device calls replaced through ``rows=``.

Restatement against longdouble, per GPU case (``R.host_error``; the GPU gate of a case is max(1e-9, 16 x this)): 8.5e-13 at worst on the
H = 64 cases; 1.8e-10 on "big" (H = 1024 at 16 kHz, 1.6 s), whose gate is therefore 2.9e-9: the two lowest bands' poles lie within 4e-4 of
the unit circle there.
Reverberation property: the dry source reads 5.155, the same source under a T60 = 0.8 s tail 3.821 (both K* = 8); the test asks for half that
margin, 0.667.  (Under T60 = 0.3 s it reads 3.891; no order against the dry value is asserted there.)
"""
import argparse
import json
import math
import os

import numpy as np
import pytest
import torch

import srmr_ref as R
import voice_stubs
from emojivoice_amd import audio, cli
from emojivoice_amd._lib import EvLibraryError

TAB16 = audio.srmr_tables()


def rows_of(tab):
    """The per-batch measurement ``audio.srmr`` takes as ``rows=``, from the restatement."""
    def rows(x, lengths, want_frame):
        r = R.srmr(x.numpy(), None if lengths is None else [int(v) for v in lengths], tab)
        return (torch.from_numpy(r["frame"]) if want_frame else None, torch.from_numpy(r["mean"]), torch.from_numpy(r["srmr"]),
                torch.from_numpy(r["counts"]))
    return rows


def fake_resample(y, orig_sr, new_sr, lengths=None, zeros=10, beta=5.0):
    """scipy's polyphase resampler in the place of the device's (what ``audio.resample`` restates), zeros past every row's own length."""
    from scipy.signal import resample_poly

    up, down = audio.resample_ratio(orig_sr, new_sr)
    out = torch.from_numpy(resample_poly(y.numpy().astype(np.float64), up, down, axis=-1).astype(np.float32))
    if lengths is not None:
        for b, n in enumerate(lengths):
            out[b, -(-int(n) * up // down):] = 0
    return out


# ---- 1. the restatement against its plain longdouble form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_restatement_against_the_plain_longdouble_form(name):
    e = R.host_error(name)
    print(f"\nSRMR host {name}: restatement against longdouble {e:.3e}  ->  GPU gate {R.gpu_gate(name):.3e}")
    assert np.finfo(np.longdouble).eps < 1e-18, "longdouble is no wider than double here: the comparison would show nothing"
    assert e <= 1e-9, "the chunked float64 restatement is within the project's gate of the exact value"


def test_transitions_carry_the_state_exactly_enough():
    """A row run as chunks with the carries equals the row run as one chunk-free recurrence in float64 to rounding: the carry is the definition's
    only structural step, so it gets its own check at the restatement's precision."""
    x, lens, tab = R.case("shape-3-3-8")
    a, b = R.srmr(x, lens, tab), R.srmr_plain(x, lens, tab, dt=np.float64)
    assert np.array_equal(a["counts"], b["counts"]) and max(R.rel_err(a[k], b[k]) for k in R.FLOAT_OUTPUTS) < 1e-11
    Mr, Mi, Mb = R.transitions(tab)
    assert not np.triu(Mr[0], 1).any() and not np.triu(Mi[0], 1).any(), "lower triangular: a stage feeds only the stages behind it"
    lam = np.hypot(tab["chan"][:, 0], tab["chan"][:, 1])
    assert np.allclose(np.hypot(Mr[:, 0, 0], Mi[:, 0, 0]), lam ** tab["hop"], rtol=1e-12), "the diagonal is a^H"


# ---- 2. the table design -------------------------------------------------------------------------------------------------------------------------
def test_table_design():
    t = TAB16
    N, K = 23, 8
    assert t["hop"] == 1024 and t["window"].shape == (4096,) and t["chan"].shape == (N, 3) and t["mod"].shape == (K, 5)
    c = t["centres"]
    assert abs(c[0] - 125.0) < 1e-9 and np.all(np.diff(c) > 0) and c[-1] < 8000.0
    e = (c + 9.26449 * 24.7) / 9.26449
    assert np.allclose(t["erb"], e, rtol=1e-14) and np.allclose(np.diff(np.log(c + 9.26449 * 24.7)), np.log((8000 + 228.83) / (125 + 228.83)) / N, rtol=1e-3)
    lam = np.hypot(t["chan"][:, 0], t["chan"][:, 1])
    assert np.all(lam < 1) and np.allclose(np.arctan2(t["chan"][:, 1], t["chan"][:, 0]), 2 * np.pi * c / 16000, rtol=1e-12)
    assert np.allclose(lam, np.exp(-2 * np.pi * (t["erb"] / (np.pi * 0.3125)) / 16000), rtol=1e-14), "a_4 = pi 6! / (2^6 (3!)^2) = 0.3125 pi"
    assert np.allclose(t["chan"][:, 2], 2 * (1 - lam) ** 4, rtol=1e-14)
    f = t["mod_centres"]
    assert abs(f[0] - 4.0) < 1e-12 and abs(f[-1] - 128.0) < 1e-9 and np.allclose(f[1:] / f[:-1], 32.0 ** (1 / 7), rtol=1e-12)
    W0 = np.tan(np.pi * f / 16000)
    B0 = W0 / 2.0
    a0 = 1 + B0 + W0 ** 2
    assert np.allclose(t["mod"], np.stack([B0 / a0, 0 * f, -B0 / a0, (2 * W0 ** 2 - 2) / a0, (1 - B0 + W0 ** 2) / a0], 1), rtol=1e-14)
    assert np.all(np.abs(t["mod"][:, 4]) < 1) and np.all(np.abs(t["mod"][:, 3]) < 1 + t["mod"][:, 4]), "ev_loudness's stability rule"
    assert np.allclose(t["cutoff"], f - B0 * 16000 / (2 * np.pi), rtol=1e-14) and np.allclose(t["cutoff"], 0.75 * f, rtol=1e-3)
    pole = np.abs(np.roots([1.0, t["mod"][0, 3], t["mod"][0, 4]]))
    assert np.all(1 - pole < 4e-4), "the 4 Hz band's poles at 16 kHz lie within 4e-4 of the unit circle"
    w = t["window"]
    assert np.array_equal(w, w[::-1]) and abs(w[0] - 0.08) < 1e-12 and np.allclose(w, 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(4096) / 4095), atol=1e-15)
    small = audio.srmr_tables(sr=1000, n_channels=32, n_bands=5)
    assert small["hop"] == 64 and small["chan"].shape == (32, 3) and small["centres"][-1] < 500 and small["mod"].shape == (5, 5)
    assert audio.srmr_tables(n_bands=1)["mod_centres"].tolist() == [4.0]
    for kw in (dict(sr=22050), dict(hop_ms=32, sr=1000), dict(frame_ms=128), dict(n_channels=33), dict(n_bands=0), dict(n_bands=9), dict(low_freq=9000.0),
               dict(mod_hi=9000.0), dict(q=0.0), dict(hop_ms=128, frame_ms=512)):
        with pytest.raises(ValueError, match="srmr_tables"):
            audio.srmr_tables(**kw)


# ---- 3. the K* rule on hand-made energies --------------------------------------------------------------------------------------------------------
def test_k_star_rule_on_hand_made_energies():
    tab = {"erb": np.array([10.0, 50.0, 100.0]), "cutoff": np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0])}
    m = np.zeros((3, 8))
    m[0, :] = [8, 4, 2, 1, 1, 1, 1, 1]                                   # 19 of 19.1: the first channel closes 90 %
    m[2, 0] = 0.1
    ratio, bw, j90, ks, cum = R.close_row(m, tab)
    assert (bw, j90, ks) == (10.0, 0, 5) and abs(ratio - 15.1 / 1.0) < 1e-12, "four edges under 10 Hz: clamped up to five bands; the denominator is band 4"
    m2 = m.copy()
    m2[1, :] = m[0] * 2
    ratio, bw, j90, ks, cum = R.close_row(m2, tab)
    assert (bw, j90, ks) == (50.0, 1, 6) and abs(ratio - (45.1 / 6.0)) < 1e-12, "six edges under 50 Hz"
    m3 = np.zeros((3, 8))
    m3[2, :] = 1.0
    ratio, bw, j90, ks, cum = R.close_row(m3, tab)
    assert (bw, j90, ks) == (100.0, 2, 7) and abs(ratio - 4.0 / 3.0) < 1e-12 and cum.tolist() == [0.0, 0.0, 1.0], "seven edges under 100 Hz: not all eight"
    tab["erb"][2] = 1000.0
    assert R.close_row(m3, tab)[3] == 8, "never more than K"
    few = {"erb": tab["erb"], "cutoff": tab["cutoff"][:4]}
    assert R.close_row(m3[:, :4], few)[0] == 0.0 and R.close_row(m3[:, :4], few)[3] == 4, "K <= 4: no high band, ratio 0, K* = K"
    lo = m3.copy()
    lo[:, 4:] = 0.0
    assert R.close_row(lo, tab)[0] == 0.0, "no energy in the high bands: ratio 0 (the caller's NaN)"
    assert R.close_row(np.zeros((3, 8)), tab)[2] == 2, "silence: no share exceeds 0.9, the last channel stands"
    x, lens, t4 = R.tie_case()
    r = R.srmr(x, lens, t4)
    assert r["counts"].tolist() == [[3, 3, 1]] and r["mean"][0, :, 0].tolist() == [256.0, 1024.0, 1024.0, 256.0], "a share of exactly 0.9 does not exceed it"
    assert R.srmr(x, lens, t4, "share_ge")["counts"][0, 1] == 2


# ---- 4. two physical properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j,k", [(10, 3), (4, 1), (18, 5)])
def test_a_modulated_tone_lands_in_its_channel_and_band(j, k):
    t = np.arange(16000) / 16000.0
    x = (0.3 * np.sin(2 * np.pi * TAB16["centres"][j] * t) * (1 + np.cos(2 * np.pi * TAB16["mod_centres"][k] * t)) / 2).astype(np.float32)
    mean = R.srmr(x[None], None, TAB16)["mean"][0]
    assert np.unravel_index(np.argmax(mean), mean.shape) == (j, k)


def test_reverberation_lowers_the_ratio():
    sr, n, t60 = 16000, 25600, 0.8
    src = R.voice(n, sr, seed=2, f0=120.0, noise=0.0).astype(np.float64)  # 1.6 s, a harmonic source gated at 4 Hz
    g = np.random.default_rng(1)
    tt = np.arange(int(1.2 * t60 * sr)) / sr
    tail = g.standard_normal(len(tt)) * 10.0 ** (-3.0 * tt / t60)        # exponentially decaying noise: -60 dB at T60
    tail[0] = 1.0
    level = lambda y: (0.3 * y / np.abs(y).max()).astype(np.float32)
    r = R.srmr(np.stack([level(src), level(np.convolve(src, tail)[:n])]), None, TAB16)
    dry, wet = r["srmr"][:, 0]
    print(f"\nSRMR dry {dry:.3f} under T60 = 0.8 s {wet:.3f}  K* {r['counts'][:, 2].tolist()}")
    assert r["counts"][:, 2].tolist() == [8, 8]
    assert dry - wet > 0.667, "half the margin the restatement shows (5.155 against 3.821)"


# ---- 5. the limits of audio.srmr -----------------------------------------------------------------------------------------------------------------
def test_audio_srmr_limits_and_shapes(monkeypatch):
    rows = rows_of(TAB16)
    y = torch.from_numpy(np.stack([R.voice(8192, 16000, seed=1), R.voice(8192, 16000, seed=2)]))
    out = audio.srmr(y, 16000, lengths=[8192, 3000], rows=rows, energies=True)
    assert set(out) == {"srmr", "bw", "k_star", "frames", "mean", "energies"} and out["srmr"].dtype == torch.float64
    assert out["frames"].tolist() == [5, 0] and math.isnan(float(out["srmr"][1])) and float(out["srmr"][0]) > 0 and out["energies"].shape == (2, 5, 23, 8)
    assert out["k_star"].tolist()[1] == 0 and float(out["bw"][1]) == 0.0
    one = audio.srmr(y[0], 16000, rows=rows)
    assert "energies" not in one and one["srmr"].shape == (1,) and float(one["srmr"][0]) == float(out["srmr"][0])
    seen = {}

    def spy(x, lengths, want_frame):
        seen["shape"], seen["lengths"] = tuple(x.shape), None if lengths is None else lengths.tolist()
        return rows(x, lengths, want_frame)
    monkeypatch.setattr(audio, "resample", fake_resample)
    audio.srmr(torch.from_numpy(np.stack([R.voice(11025, 22050, seed=1)] * 2)), 22050, lengths=[11025, 441 * 5 + 1], rows=spy)
    assert seen == {"shape": (2, 8000), "lengths": [8000, 1601]}, "22050 -> 16000 is up 320, down 441; lengths round up"
    for bad, kw in ((y, dict(sr=16000.5)), (y, dict(sr=0)), (y[None], {}), (torch.zeros(2, 0), {}), (y, dict(lengths=[1, 2, 3]))):
        with pytest.raises(ValueError, match="srmr"):
            audio.srmr(bad, **{**dict(sr=16000, rows=rows), **kw})
    with pytest.raises(EvLibraryError, match="no CPU fallback"):
        audio.srmr(y, 16000)


# ---- 6. the reports ------------------------------------------------------------------------------------------------------------------------------
def _wavs():
    """a, b: half a second of voice at 22.05 kHz; c: 100 ms, under a frame."""
    return {"a.wav": R.voice(11025, 22050, seed=1, f0=110.0), "b.wav": R.voice(11025, 22050, seed=2, f0=190.0), "c.wav": R.voice(2205, 22050, seed=3)}


def test_reverb_report_json_shape(tmp_path, monkeypatch):
    wavs = _wavs()
    monkeypatch.setattr(audio, "load_audio", lambda path, sr=22050, device="cuda": torch.from_numpy(wavs[os.path.basename(str(path))]).unsqueeze(0))
    monkeypatch.setattr(audio, "resample", fake_resample)
    flist = voice_stubs.filelist(tmp_path, wavs)
    args = cli.validate_args(argparse.Namespace(reverb_report=str(flist), batch_size=2, sample_rate=None, prepare_dataset=None, srmr_rows=rows_of(TAB16)))
    rep = cli.reverb_report(args, "cpu")
    with open(f"{flist}.srmr.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep)) and set(saved) == {"sample_rate", "srmr_sample_rate", "files", "speakers", "overall"}
    assert saved["sample_rate"] == 22050 and saved["srmr_sample_rate"] == 16000
    assert [set(f) for f in saved["files"]] == [{"path", "speaker", "seconds", "srmr", "frames", "k_star"}] * 3
    a, b, c = saved["files"]
    want = audio.srmr(torch.from_numpy(wavs["a.wav"]), 22050, rows=rows_of(TAB16))
    assert (a["speaker"], a["seconds"], a["frames"]) == ("7", 0.5, 4) and a["srmr"] == float(want["srmr"][0]) and a["k_star"] == int(want["k_star"][0])
    assert (c["speaker"], c["srmr"], c["frames"], c["k_star"]) == ("12", None, 0, 0), "under a frame: null, not NaN"
    s7, s12 = saved["speakers"]["7"], saved["speakers"]["12"]
    assert set(s7) == {"files", "measured", "mean", "std", "min"} and (s7["files"], s7["measured"]) == (2, 2)
    assert abs(s7["mean"] - (a["srmr"] + b["srmr"]) / 2) < 1e-12 and abs(s7["std"] - abs(a["srmr"] - b["srmr"]) / 2) < 1e-12 and s7["min"] == min(a["srmr"], b["srmr"])
    assert s12 == {"files": 1, "measured": 0, "mean": None, "std": None, "min": None}
    assert saved["overall"] == {"files": 3, **{k: s7[k] for k in ("measured", "mean", "std", "min")}}
    assert "NaN" not in open(f"{flist}.srmr.json").read()
    empty = tmp_path / "empty.txt"
    empty.write_text("\n", encoding="utf-8")
    with pytest.raises(SystemExit, match="no files"):
        cli.reverb_report(argparse.Namespace(reverb_report=str(empty), batch_size=4), "cpu")
    with pytest.raises(AssertionError, match="Batch size"):
        cli.validate_args(argparse.Namespace(reverb_report=str(flist), batch_size=0, sample_rate=None, prepare_dataset=None))


def test_evaluate_pairs_srmr_key_sets(tmp_path, monkeypatch):
    wavs = _wavs()
    voice_stubs.base(monkeypatch, wavs)
    monkeypatch.setattr(audio, "resample", fake_resample)
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
    pairs.write_text("a.wav|b.wav|7\nb.wav|a.wav|7\na.wav|c.wav|12\n", encoding="utf-8")
    ns = lambda **kw: argparse.Namespace(evaluate_pairs=str(pairs), batch_size=2, sample_rate=None, prepare_dataset=None, voice_report=None, **kw)
    plain = cli.evaluate_pairs(cli.validate_args(ns()), "cpu")
    plain_bytes = open(f"{pairs}.eval.json", "rb").read()
    assert cli.evaluate_pairs(cli.validate_args(ns(srmr=False, srmr_rows=rows_of(TAB16))), "cpu") == plain
    assert open(f"{pairs}.eval.json", "rb").read() == plain_bytes, "without the flag the report keeps every byte"
    rep = cli.evaluate_pairs(cli.validate_args(ns(srmr=True, srmr_rows=rows_of(TAB16))), "cpu")
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert all("srmr" not in p for p in plain["pairs"]) and "srmr" not in plain["overall"]
    assert [{k: v for k, v in p.items() if k != "srmr"} for p in saved["pairs"]] == plain["pairs"], "the flag changes no other figure"
    assert set(saved["overall"]) - {"srmr"} == set(plain["overall"]) and set(saved) == set(plain)
    p0, p1, p2 = saved["pairs"]
    assert all(set(p["srmr"]) == {"recorded", "synthesised", "delta"} for p in saved["pairs"])
    va = float(audio.srmr(torch.from_numpy(whole(wavs["a.wav"])), 22050, rows=rows_of(TAB16))["srmr"][0])
    assert p0["srmr"]["recorded"] == va == p1["srmr"]["synthesised"] and abs(p0["srmr"]["delta"] - (p0["srmr"]["synthesised"] - va)) < 1e-12
    assert abs(p0["srmr"]["delta"] + p1["srmr"]["delta"]) < 1e-12, "the swapped pair has the opposite delta"
    assert p2["srmr"]["synthesised"] is None and p2["srmr"]["delta"] is None and p2["srmr"]["recorded"] == va
    s7, s12 = saved["speakers"]["7"]["srmr"], saved["speakers"]["12"]["srmr"]
    assert set(s7) == {"recorded", "synthesised", "delta"} and abs(s7["delta"]) < 1e-12 and abs(s7["recorded"] - s7["synthesised"]) < 1e-12
    assert s12 == {"recorded": va, "synthesised": None, "delta": None}
