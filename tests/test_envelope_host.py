"""The host side of the spectral envelope and its mel-cepstrum, on the CPU: ``audio.freq_warp_matrix`` against what a frequency warping must do,
the properties of the restatement (tests/envelope_ref.py) that make it CheapTrick, every mutant against it, the header and the library's symbols
and code object, the ``audio`` functions through ``rows=``, the JSON of ``--evaluate_pairs --envelope_mcd`` with the device calls replaced, and
the argument errors of the Python layer.

Measured here (printed by the tests; the bounds are the issue's): the round trip of a decaying 41-term cepstrum through alpha and -alpha at order
400 returns it within 1e-15 and the warped cosine series stands within 1e-15 of the original on the warped axis (bound 1e-12); a band-limited
pulse train at 64.9, 100, 220.5, 333.3 and 600 Hz (22050 / 1024) has an envelope that is flat between f0 and 8 kHz within 0.077 dB over frequency
and 0.051 dB over the place of the frame centre inside a period (bound 0.2 dB).
"""
import argparse
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import envelope_ref as R
import voice_stubs
from emojivoice_amd import _lib, audio, cli
from emojivoice_amd._lib import EvLibraryError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = 10.0 / np.log(10.0)


def rows_ref(x, lengths, period, sr, n_fft, hop, order, alpha, want_envelope):
    """The per-batch measurement ``audio.spectral_envelope`` takes as ``rows=``, from the restatement."""
    r = R.envelope(x.numpy(), None if lengths is None else [int(v) for v in lengths], period.numpy().astype(np.float32), hop, n_fft,
                   audio.freq_warp_matrix(n_fft // 2 + 1, order, alpha), sr / 500.0)
    return (torch.from_numpy(r["env"]) if want_envelope else None), torch.from_numpy(r["mcep"]), torch.from_numpy(r["class"])


# ---- 1. the warp matrix ------------------------------------------------------------------------------------------------------------------------
def test_warp_matrix_is_the_identity_at_alpha_zero():
    A = audio.freq_warp_matrix(65, 24, 0.0)
    assert A.shape == (25, 65) and A.dtype == np.float64 and np.array_equal(A, np.eye(25, 65))
    assert np.array_equal(audio.freq_warp_matrix(3, 5, 0.0), np.eye(6, 3)), "more outputs than inputs: zeros behind"


def test_warp_matrix_round_trip_and_the_warped_axis():
    c = 0.8 ** np.arange(41) * np.cos(0.7 * np.arange(41))
    a = 0.455
    fwd = audio.freq_warp_matrix(41, 400, a) @ c
    back = audio.freq_warp_matrix(401, 40, -a) @ fwd
    e_rt = float(np.abs(back - c).max())
    w = np.linspace(0.0, np.pi, 257)
    ww = w + 2.0 * np.arctan(a * np.sin(w) / (1.0 - a * np.cos(w)))
    series = lambda cc, om: (cc[None, :] * np.cos(np.arange(len(cc))[None, :] * om[:, None])).sum(1)
    e_ax = float(np.abs(series(fwd, ww) - series(c, w)).max())
    print(f"\nfreq_warp_matrix: round trip {e_rt:.3e}, the warped cosine series against the original {e_ax:.3e} (bound 1e-12)")
    assert e_rt <= 1e-12 and e_ax <= 1e-12
    assert abs(fwd[400]) < 1e-30 or abs(fwd[400]) < 1e-12 * abs(fwd).max(), "order 400 holds the whole warped cepstrum"


def test_warp_matrix_is_freqt_on_a_vector():
    """The recursion run on a vector, as SPTK writes it, equals the matrix built from unit vectors."""
    rng = np.random.default_rng(0)
    c, a, m2 = rng.standard_normal(30), 0.35, 12
    g = np.zeros(m2 + 1)
    for i in range(len(c) - 1, -1, -1):
        d = g.copy()
        g[0] = c[i] + a * d[0]
        g[1] = (1.0 - a * a) * d[0] + a * d[1]
        for m in range(2, m2 + 1):
            g[m] = d[m - 1] + a * (d[m] - g[m - 1])
    assert np.abs(audio.freq_warp_matrix(30, m2, a) @ c - g).max() <= 1e-13


# ---- 2. the restatement ------------------------------------------------------------------------------------------------------------------------
def _frame(x, T, nfft=128, c=None, mutant=None, A=None):
    A = audio.freq_warp_matrix(nfft // 2 + 1, 4, 0.455) if A is None else A
    return R.frame_envelope(x, len(x), len(x) // 2 if c is None else c, T, nfft, A, R.cos_table(nfft), mutant=mutant)


def test_scaling_the_signal_moves_the_level_only():
    x = R.harmonic_row(600, 20.0, seed=1).astype(np.float64)
    g = 3.7
    Le, mc, half, kd, _ = _frame(x, 20.0)
    Lg, mg, half_g, kd_g, _ = _frame(g * x, 20.0)
    assert (half, kd) == (half_g, kd_g) == (30, 6)
    assert np.abs(Lg - (Le + 2.0 * np.log(g))).max() <= 1e-10, "the power envelope in nepers gains 2 ln g"   # (the floor is far below)
    assert abs(mg[0] - (mc[0] + np.log(g))) <= 1e-10 and np.abs(mg[1:] - mc[1:]).max() <= 1e-10, "mc[0] is the log AMPLITUDE level"


@pytest.mark.parametrize("T", [2.0, 2.6, 8.0, 20.0, 41.6])
def test_the_direct_smoothing_is_the_cumulative_sum_form(T):
    rng = np.random.default_rng(2)
    P = rng.uniform(0.1, 5.0, 65)
    a, b = R.smooth_direct(P, T, 128), R.smooth_cumulative(P, T, 128)
    e = float(np.abs(a / b - 1.0).max())
    print(f"\nsmoothing at T = {T}: direct against cumulative {e:.3e}")
    assert e <= 1e-12
    assert np.abs(R.smooth_direct(np.ones(65), T, 128) - 1.0).max() <= 1e-13, "a flat spectrum stays flat: the cells' weights add up to wd"


@pytest.mark.parametrize("f0", [64.9, 100.0, 220.5, 333.3, 600.0])
def test_a_pulse_train_has_a_flat_time_invariant_envelope(f0):
    sr, nfft = 22050.0, 1024
    T = float(np.float32(sr / f0))
    x = R.pulse_train(6000, T, 0.5)
    A = audio.freq_warp_matrix(nfft // 2 + 1, 24, 0.455)
    tab = R.cos_table(nfft)
    k = np.arange(nfft // 2 + 1) * sr / nfft
    band = (k >= f0) & (k <= 8000.0)
    Ls = np.stack([R.frame_envelope(x, len(x), 3000 + int(round(T * s / 8.0)), T, nfft, A, tab)[0] for s in range(8)]) * DB
    over_f = float((Ls[:, band].max(1) - Ls[:, band].min(1)).max())
    over_t = float((Ls[:, band].max(0) - Ls[:, band].min(0)).max())
    print(f"\npulse train at {f0} Hz (T = {T:.3f}): ripple over frequency {over_f:.3f} dB, over the frame's place in the period {over_t:.3f} dB (bound 0.2)")
    assert over_f <= 0.2 and over_t <= 0.2


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_differs(mutant):
    x = R.harmonic_row(600, 20.0, seed=3)
    Le, mc, *_ = _frame(x, 13.37)
    Lm, mm, *_ = _frame(x, 13.37, mutant=mutant)
    far = max(float(np.abs(Le - Lm).max()), float(np.abs(mc - mm).max()))
    print(f"\nenvelope mutant {mutant}: {far:.3e} from the restatement (the GPU tests' gate: 1e-9)")
    assert far > 1e-9, "a mutant the gate of the GPU tests could not tell from the definition"


def test_periods_classes_and_edges():
    assert R.period_of(np.float32(0.0), 128, 8.0) == (8.0, 1) and R.period_of(np.float32(np.nan), 128, 8.0) == (8.0, 1)
    assert R.period_of(np.float32(2.0), 128, 8.0) == (2.0, 0) and R.period_of(np.nextafter(np.float32(2.0), np.float32(0)), 128, 8.0)[1] == 1
    assert R.period_of(np.float32(41.7), 128, 8.0)[1] == 1 and abs(R.t_max(1024) - 22050.0 / 64.79) < 0.01, "CheapTrick's floor: 64.8 Hz at 22050 / 1024"
    x = R.harmonic_row(5 * 32 - 7, 11.5, seed=3)
    r = R.envelope(x[None], None, np.full((1, 5), 11.5, np.float32), 32, 128, np.eye(3, 65), 8.0)
    assert r["class"][0].tolist() == [[0, 17, 11]] * 5 and r["env"].shape == (1, 5, 65) and r["mcep"].shape == (1, 5, 3)
    z = R.envelope(np.zeros((1, 64), np.float32), None, np.zeros((1, 2), np.float32), 32, 128, np.eye(3, 65), 8.0)
    assert z["class"][0].tolist() == [[2, 12, 16]] * 2 and not z["env"].any() and not z["mcep"].any(), "digital silence: silent frames, zeros"
    e = R.envelope(np.ones((2, 64), np.float32), [0, 65], np.zeros((2, 2), np.float32), 32, 128, np.eye(3, 65), 8.0)
    assert (e["class"] == [3, 0, 0]).all(), "len < 1 and len > L are empty rows"


# ---- 3. the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_code_object():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        head = f.read()
    line = next(l for l in head.splitlines() if l.startswith("#define EV_ABI_VERSION"))
    assert re.match(r"#define EV_ABI_VERSION 4\b", line) and "ev_load_envelope, ev_envelope" in line
    assert "int ev_load_envelope(ev_handle *h, const double *twiddle" in head and "int ev_envelope(ev_handle *h, const float *d_x" in head
    assert {"ev_load_envelope", "ev_envelope"} <= set(_lib.EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert lib.ev_abi_version() == 4 and lib.ev_load_envelope and lib.ev_envelope
    spec = importlib.util.spec_from_file_location("code_object", os.path.join(REPO, "tools", "code_object.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain is not installed")
    ks = {k["demangled"].split("(")[0]: k for k in co.kernels(_lib.LIB_PATH)}
    for name in ("envelope_power_kernel", "envelope_cepstrum_kernel"):
        k = ks[name]
        print(f"\n{name}: {k['vgpr_count']} VGPR, {k['sgpr_count']} SGPR")
        assert (k["sgpr_spill_count"], k["vgpr_spill_count"], k["private_segment_fixed_size"]) == (0, 0, 0), k


# ---- 4. audio ----------------------------------------------------------------------------------------------------------------------------------
def _rows(sr=4000):
    a, b = R.harmonic_row(400, 20.0, seed=5), R.harmonic_row(333, 16.0, seed=6)
    b[88:170] = 0.0                                                      # frames 3 and 4 at T = 16 (half = 24) see zeros only
    x, lens = R.padded([a, b, np.zeros(64, np.float32)], fill=0.0)
    p = np.zeros((3, 13), np.float32)
    p[0], p[1] = 20.0, 16.0
    return x, lens, p


def test_audio_spectral_envelope_through_rows():
    x, lens, p = _rows()
    kw = dict(sr=4000, n_fft=128, hop_length=32, order=6, alpha=0.31, rows=rows_ref)
    out = audio.spectral_envelope(torch.from_numpy(x), torch.from_numpy(p), lengths=lens, envelope=True, **kw)
    assert set(out) == {"mcep", "class", "log_envelope"} and out["mcep"].shape == (3, 13, 7) and out["log_envelope"].shape == (3, 13, 65)
    ref = R.envelope(x, lens, p, 32, 128, audio.freq_warp_matrix(65, 6, 0.31), 8.0)
    assert np.array_equal(out["class"].numpy(), ref["class"][..., 0]) and np.array_equal(out["mcep"].numpy(), ref["mcep"])
    assert out["class"][1].tolist() == [0, 0, 0, 2, 2, 0, 0, 0, 0, 0, 0, 3, 3] and out["class"][2].tolist() == [2, 2] + [3] * 11
    assert audio.ENVELOPE_CLASSES[2] == "silent" and audio.spectral_envelope(torch.from_numpy(x), torch.from_numpy(p), lengths=lens, **kw)["log_envelope"] is None
    one = audio.spectral_envelope(torch.from_numpy(x[0]), torch.from_numpy(p[0]), **kw)
    assert one["mcep"].shape == (1, 13, 7) and np.array_equal(one["mcep"][0, :11].numpy(), ref["mcep"][0, :11]), "a 1-D input is the same row"
    cep, n = audio.envelope_cepstra(torch.from_numpy(x), torch.from_numpy(p), lengths=lens, **kw)
    assert cep.shape == (3, 6, 13) and cep.dtype == torch.float32 and n.tolist() == [13, 9, 0]
    keep = ref["class"][1, :, 0] < 2
    assert np.array_equal(cep[1, :, :9].numpy(), ref["mcep"][1, keep, 1:].T.astype(np.float32)), "the kept frames first, in order, without c0"
    pt = audio.period_from_pitch({"f0": torch.tensor([[100.0, 0.0, 200.0]]), "voiced": torch.tensor([[True, True, False]])}, 4000)
    assert pt.tolist() == [[40.0, 0.0, 0.0]] and pt.dtype == torch.float32


def test_envelope_mcd_composes_pitch_envelope_dtw(monkeypatch):
    x, lens, p = _rows()
    seen = {}

    def fake_dtw(a, b, na, nb, metric):
        seen.update(a=a, b=b, na=na, nb=nb, metric=metric)
        cost = torch.stack([(a[r, :, 0] - b[r, :, 0]).double().norm() for r in range(a.shape[0])])
        return {"cost": cost, "steps": torch.ones(a.shape[0], dtype=torch.int32), "path": None}

    monkeypatch.setattr(audio, "dtw", fake_dtw)
    pitch_of = lambda q: {"f0": torch.from_numpy(np.where(q > 0, 4000.0 / np.maximum(q, 1), 0).astype(np.float32)), "voiced": torch.from_numpy(q > 0)}
    track = lambda y, sr, hop_length, lengths: pitch_of(p if np.array_equal(y[0].numpy(), x[0]) else p[[1, 0, 2]])
    kw = dict(pitch=track, n_fft=128, hop_length=32, order=6, alpha=0.31, rows=rows_ref)
    mcd = audio.envelope_mcd(torch.from_numpy(x), torch.from_numpy(x[[1, 0, 2]]), 4000, lens, [lens[1], lens[0], lens[2]], **kw)
    assert seen["metric"] == "euclidean" and seen["a"].shape == (3, 6, 13) and seen["na"].tolist() == [13, 9, 1] and seen["nb"].tolist() == [9, 13, 1]
    assert mcd.dtype == torch.float64 and mcd[0] > 0 and float(mcd[0]) == float(mcd[1]) and torch.isnan(mcd[2]), "a side without a frame: NaN"
    assert abs(float(mcd[0]) - audio.MCD_DB * float((seen["a"][0, :, 0] - seen["b"][0, :, 0]).double().norm())) < 1e-12


def test_argument_errors_of_the_python_layer():
    y, p = torch.zeros(2, 256), torch.zeros(2, 8)
    kw = dict(sr=4000, n_fft=128, hop_length=32, rows=rows_ref)
    for bad_y, bad_p, over in ((y[None], p, {}), (torch.zeros(2, 0), p, {}), (y, torch.zeros(2, 7), {}), (y, torch.zeros(3, 8), {}), (y, p, dict(order=64)),
                               (y, p, dict(order=-1)), (y, p, dict(alpha=1.0)), (y, p, dict(n_fft=127)), (y, p, dict(n_fft=2048)),
                               (y, p, dict(hop_length=0)), (y, p, dict(hop_length=513)), (y, p, dict(sr=500)), (y, p, dict(sr=22050))):
        with pytest.raises(ValueError, match="spectral_envelope"):
            audio.spectral_envelope(bad_y, bad_p, **{**kw, **over})
    with pytest.raises(EvLibraryError, match="no CPU fallback"):
        audio.spectral_envelope(y, p, 4000, 128, 32)
    with pytest.raises(ValueError, match="envelope_cepstra"):
        audio.envelope_cepstra(y, p, order=0, **kw)
    for bad in (dict(n_in=0, order=3, alpha=0.1), dict(n_in=4, order=-1, alpha=0.1), dict(n_in=4, order=3, alpha=1.0)):
        with pytest.raises(ValueError, match="freq_warp_matrix"):
            audio.freq_warp_matrix(**bad)
    ns = lambda **k: argparse.Namespace(sample_rate=None, prepare_dataset=None, batch_size=2, **k)
    with pytest.raises(AssertionError, match="--envelope_mcd is an option of --evaluate_pairs"):
        cli.validate_args(ns(envelope_mcd=True, voice_report="x.txt"))
    assert cli.validate_args(ns(envelope_mcd=True, evaluate_pairs="x.txt")).envelope_mcd
    assert "--evaluate_pairs pairs.txt --envelope_mcd" in cli.__doc__


# ---- 5. the report -----------------------------------------------------------------------------------------------------------------------------
def test_evaluate_pairs_with_and_without_envelope_mcd(tmp_path, monkeypatch):
    wavs = {"a.wav": R.harmonic_row(16 * 256, 147.0, seed=7), "b.wav": R.harmonic_row(14 * 256, 140.0, seed=8), "c.wav": np.zeros(12 * 256, np.float32)}
    voice_stubs.base(monkeypatch, wavs)
    calls = []

    def fake_dtw(a, b, fa, fb, metric):
        calls.append((tuple(a.shape), [int(v) for v in fa], [int(v) for v in fb]))
        cost = torch.stack([(a[r, :, 0] - b[r, :, 0]).double().norm() for r in range(a.shape[0])])
        return {"cost": cost, "steps": torch.ones(a.shape[0], dtype=torch.int32), "path": torch.zeros(a.shape[0], 1, 2, dtype=torch.int32)}

    monkeypatch.setattr(cli, "wav_at_rate", lambda path, sr, device: torch.from_numpy(wavs[os.path.basename(str(path))]).unsqueeze(0))
    monkeypatch.setattr(audio, "mel_spectrogram", lambda w, *a, **k: torch.zeros(1, 80, w.shape[1] // 256))
    monkeypatch.setattr(audio, "mel_cepstrum", lambda mel, n=13: torch.zeros(1, n, mel.shape[2]))
    monkeypatch.setattr(audio, "dtw", fake_dtw)
    monkeypatch.setattr(audio, "f0_errors", lambda *a: {"rmse_cents": [None] * a[0].shape[0], "voicing_error": torch.zeros(a[0].shape[0]),
                                                        "voiced_pairs": torch.zeros(a[0].shape[0], dtype=torch.int64)})
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("a.wav|b.wav|7\nc.wav|a.wav|12\n", encoding="utf-8")
    ns = lambda **kw: argparse.Namespace(evaluate_pairs=str(pairs), batch_size=2, sample_rate=None, prepare_dataset=None, voice_report=None, **kw)
    plain = cli.evaluate_pairs(cli.validate_args(ns()), "cpu")
    plain_bytes = open(f"{pairs}.eval.json", "rb").read()
    assert cli.evaluate_pairs(cli.validate_args(ns(envelope_mcd=False, envelope_rows=rows_ref)), "cpu") == plain
    assert open(f"{pairs}.eval.json", "rb").read() == plain_bytes, "without the flag the report keeps every byte"
    calls.clear()
    rep = cli.evaluate_pairs(cli.validate_args(ns(envelope_mcd=True, envelope_rows=rows_ref)), "cpu")
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep)) and "NaN" not in open(f"{pairs}.eval.json").read()
    assert [{k: v for k, v in p.items() if k != "mcd_env_db"} for p in saved["pairs"]] == plain["pairs"], "the flag changes no other figure"
    assert set(saved["overall"]) - {"mcd_env_db"} == set(plain["overall"]) and set(saved) == set(plain)
    assert calls == [((2, 13, 16), [16, 12], [14, 16]), ((2, 24, 16), [16, 1], [14, 16])], "the mel alignment, then the envelope's own: 24 coefficients"
    p0, p1 = saved["pairs"]
    assert p0["mcd_env_db"] > 0 and p1["mcd_env_db"] is None, "a silent recording has no frame to align"
    assert saved["speakers"]["7"]["mcd_env_db"] == p0["mcd_env_db"] == saved["overall"]["mcd_env_db"] and saved["speakers"]["12"]["mcd_env_db"] is None
