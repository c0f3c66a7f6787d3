"""The device calls behind --voice_report and --evaluate_pairs replaced by the numpy restatements, for the host tests of the report layer (no GPU).
A plain module, imported the way pitch_ref is.  ``base`` patches what every report needs (load_audio, pitch_yin, voice_quality); the others patch one
analysis each and hand back the stand-in, so a test can call it on its own.
"""
import os

import numpy as np
import torch

import pitch_ref
import voice_quality_ref as V
from emojivoice_amd import audio


def filelist(tmp_path, wavs):
    """The three-file list of the JSON-shape tests: a.wav (absolute) and b.wav (relative) of speaker 7, c.wav of speaker 12; the files are empty."""
    for name in wavs:
        (tmp_path / name).write_bytes(b"")                                 # (the stubs never open them)
    flist = tmp_path / "filelist.txt"
    flist.write_text(f"{tmp_path / 'a.wav'}|7|first\nb.wav|7|second\nc.wav|12|silent take\n", encoding="utf-8")
    return flist


def base(monkeypatch, wavs):
    """audio.load_audio from ``wavs`` {base name: float32 row}, audio.pitch_yin and audio.voice_quality from their restatements -> fake_yin."""
    t = audio.voice_quality_tables(22050, 1024)
    gv = V.Geometry(1024, 256, 1024, t["q_fit"], t["q_min"], t["q_max"], V.GEOMETRIES[3].bands, 22050)

    def fake_yin(y, sr=22050, fmin=65.0, fmax=600.0, frame_length=1024, hop_length=256, threshold=0.1, lengths=None):
        r = pitch_ref.pitch_yin(y.numpy(), lengths, frame_length, hop_length, 36, 340, threshold)
        return {"f0": torch.from_numpy(pitch_ref.f0_from_period(r["period"], sr)).float(), "voiced": torch.from_numpy(r["lag"] > 0)}

    def fake_vq(y, sr=22050, fmin=65.0, fmax=600.0, frame_length=1024, hop_length=256, lengths=None, power_floor=1e-7):
        fr, pk, _, _ = V.batch(y.numpy(), lengths, gv, floor=power_floor)
        out = {k: torch.from_numpy(fr[..., i].copy()) for i, k in enumerate(audio.VOICE_QUALITY_FIGURES + ("power",))}
        out["peak_quefrency"] = torch.from_numpy(pk)
        return out

    monkeypatch.setattr(audio, "load_audio", lambda path, sr=22050, device="cuda": torch.from_numpy(wavs[os.path.basename(str(path))]).unsqueeze(0))
    monkeypatch.setattr(audio, "pitch_yin", fake_yin)
    monkeypatch.setattr(audio, "voice_quality", fake_vq)
    return fake_yin


def formants(monkeypatch):
    """audio.formants from its restatement at 11025 Hz -> fake_formants."""
    import formants_ref as R

    gf = R.geometry(11025.0, 512, 128, 13)

    def fake_formants(y, sr=22050, max_formant=5500.0, n_formants=4, order=None, frame_length=1024, hop_length=256, f_lo=50.0, lengths=None):
        x = y.numpy()[:, ::2]                                              # (a plain decimation stands in for the device's resampler)
        lpc, fm, ct, _, _ = R.batch(x, None if lengths is None else [-(-n // 2) for n in lengths], gf)
        return {"frequency": torch.from_numpy(fm[..., 0].copy()), "bandwidth": torch.from_numpy(fm[..., 1].copy()), "count": torch.from_numpy(ct),
                "gain": torch.from_numpy(lpc[..., 13].copy())}

    monkeypatch.setattr(audio, "formants", fake_formants)
    return fake_formants


def flat_formants(monkeypatch):
    """audio.formants as the same four formants on every frame, F2 too wide on every fifth -> (fake_formants, calls): calls["formants"] counts its runs."""
    calls = {"formants": 0}

    def fake_formants(y, sr=22050, max_formant=5500.0, n_formants=4, order=None, frame_length=1024, hop_length=256, f_lo=50.0, lengths=None,
                      power_floor=1e-10):
        calls["formants"] += 1
        B, F = y.shape[0], -(-y.shape[1] // hop_length)
        freq = torch.tensor([520.0, 1480.0, 2530.0, 3600.0], dtype=torch.float64).expand(B, F, 4).clone()
        band = torch.full((B, F, 4), 120.0, dtype=torch.float64)
        band[:, ::5, 1] = 900.0                                           # F2 too wide on every fifth frame
        return {"frequency": freq, "bandwidth": band, "count": torch.full((B, F), 4, dtype=torch.int32)}

    monkeypatch.setattr(audio, "formants", fake_formants)
    return fake_formants, calls


def perturbation(monkeypatch):
    """audio.perturbation from its restatement at the restated YIN's lags -> fake_perturbation."""
    import perturbation_ref as R

    def fake_perturbation(y, sr=22050, fmin=65.0, fmax=600.0, frame_length=1024, hop_length=256, lengths=None, lag=None, n_cycles=3,
                          period_factor=1.3, amplitude_factor=1.6, power_floor=1e-10):
        x = y.numpy()
        lag = pitch_ref.pitch_yin(x, lengths, frame_length, hop_length, 36, 340, 0.1)["lag"]
        r = R.batch(x, lengths, lag, R.geo(hop_length, frame_length, n_cycles, period_factor, amplitude_factor, power_floor))
        out = {k: torch.from_numpy(r["frame"][..., i].copy()) for i, k in enumerate(audio._PERTURBATION_FRAME)}
        out.update(count=torch.from_numpy(r["count"]), marks=torch.from_numpy(r["marks"]), lag=torch.from_numpy(lag))
        return out

    monkeypatch.setattr(audio, "perturbation", fake_perturbation)
    return fake_perturbation


def harmonics(monkeypatch):
    """audio.harmonics from its restatement at the restated YIN's periods and the formants it is handed -> fake_harmonics."""
    import harmonics_ref as R

    def fake_harmonics(y, sr=22050, fmin=65.0, fmax=600.0, frame_length=1024, hop_length=256, lengths=None, period=None, formants=None, n_harm=48,
                       search=0.25, min_spacing=4.0, a3_range=0.1, power_floor=1e-7):
        assert formants is not None and formants is not False, "the CLI hands the formants over"
        x = y.numpy()
        g = R.Geometry(frame_length, hop_length, frame_length, sr, n_harm, search, min_spacing, a3_range)
        fm = np.stack([formants["frequency"].numpy(), formants["bandwidth"].numpy()], axis=-1)
        period = pitch_ref.pitch_yin(x, lengths, frame_length, hop_length, 36, 340, 0.1)["period"]
        r = R.batch(x, lengths, period, g, fm, formants["count"].numpy(), floor=power_floor)
        out = {k: torch.from_numpy(r["frame"][..., i].copy()) for i, k in enumerate(audio._HARMONIC_FRAME)}
        out.update(n_harmonics=torch.from_numpy(r["count"][..., 0].copy()), flags=torch.from_numpy(r["count"][..., 1].copy()),
                   harmonic_hz=torch.from_numpy(r["harm"][..., 0].copy()), harmonic_db=torch.from_numpy(r["harm"][..., 1].copy()))
        return out

    monkeypatch.setattr(audio, "harmonics", fake_harmonics)
    return fake_harmonics


def ref_functionals(values, mask=None, lengths=None, percentiles=(0.2, 0.5, 0.8)):
    """audio.functionals on the host, from the restatement: the same dict, the same dtypes."""
    import functionals_ref as R

    (B, K, F), q = audio.functional_arguments(values, mask, lengths, percentiles)
    m = None if mask is None else (torch.as_tensor(mask) != 0).expand(values.shape).reshape(B, K, F).numpy()
    r = R.batch(values.reshape(B, K, F).double().numpy(), m, None if lengths is None else [int(n) for n in torch.as_tensor(lengths)], tuple(q))
    stat, count = torch.from_numpy(r["stat"]), torch.from_numpy(r["count"])
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    out = {k: torch.where(count[..., audio._FUNCTIONAL_BEHIND[k]] > 0, stat[..., i], nan) for i, k in enumerate(audio.FUNCTIONAL_STATISTICS)}
    out["percentiles"] = torch.where(count[..., :1] > 0, stat[..., 12:], nan)
    out["range"] = out["percentiles"][..., -1] - out["percentiles"][..., 0]
    out.update({k: count[..., i] for i, k in enumerate(audio.FUNCTIONAL_COUNTS)})
    return out
