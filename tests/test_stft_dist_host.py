"""CPU-side checks of the STFT-distance path: the numpy restatement (tests/stft_dist_ref.py) against ``torch.stft`` in float64, the input
condition of the device tests (float64 against longdouble), the folds the reflection test must tell apart, ``audio.stft_distance`` with a
stand-in for the device call, the argument checks, ``vocoder_summary`` / ``validate_args`` with the new keys, and the C ABI's declaration
and export.
"""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import stft_dist_ref as R
from emojivoice_amd import _lib, audio, cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_and_tables():
    assert audio.MSTFT_RESOLUTIONS == R.RESOLUTIONS and audio.MSTFT_POWER_FLOOR == R.POWER_FLOOR
    for W in (24, 240, 600, 1200):
        w = audio.stft_dist_window(W)
        assert w.dtype == np.float64 and w.shape == (W,) and np.array_equal(w, R.hann(W)) and w[0] == 0.0
        # (two ways of writing the same window: a few roundings of 2^-52 each on values up to 1)
        assert np.abs(w - torch.hann_window(W, periodic=True, dtype=torch.float64).numpy()).max() <= 1e-15
    assert np.array_equal(audio.stoi_twiddle(64), R.twiddle(64))
    assert [R.frames(n, 64, 10) for n in (1, 32, 33, 39, 40, 2560)] == [0, 0, 4, 4, 5, 257]
    for H in (10, 50, 120, 240):
        lens = R.ragged_lens(H)
        assert [(1 + n // H) % 16 for n in lens] == [15, 0, 1] and min(lens) >= 2500 and max(lens) <= 6000, (H, lens)


@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=[f"{g[0]}-{g[1]}-{g[2]}" for g in R.GEOMETRIES])
def test_restatement_magnitudes_equal_torch_stft(geom):
    """sqrt(max(|X|^2, floor)) of the restatement against torch.stft(x.double(), n_fft, hop, win, window=hann, center=True,
    pad_mode="reflect"), clamped and rooted the same way: every entry within 1e-12 of the frame's largest magnitude.  The scale of a
    DFT's rounding error is the frame, not the bin (an FFT's is eps log2(n_fft) times the frame's norm), so a bin that cancels down to the
    floor carries the same absolute error as the loudest one: relative to itself it differs by up to 7e-12 here, relative to the frame by
    1.4e-15 (the worst of the four geometries)."""
    nfft, H, W = geom
    x, _, lens = R.rows_for(geom)
    worst = 0.0
    for b, n in enumerate(lens):
        m = np.sqrt(R.spectra(x[b, :n], geom))
        z = torch.stft(torch.from_numpy(x[b, :n]).double(), nfft, hop_length=H, win_length=W, window=torch.hann_window(W, dtype=torch.float64),
                       center=True, pad_mode="reflect", return_complex=True)
        t = torch.sqrt(torch.clamp(z.real ** 2 + z.imag ** 2, min=R.POWER_FLOOR)).numpy().T
        assert t.shape == m.shape == (R.frames(n, nfft, H), nfft // 2 + 1)
        worst = max(worst, float(np.max(np.abs(m - t) / t.max(axis=1, keepdims=True))))
    print(f"\nSTFT distance restatement against torch.stft {geom}: worst difference of a magnitude relative to its frame's largest {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=[f"{g[0]}-{g[1]}-{g[2]}" for g in R.GEOMETRIES])
def test_device_cases_hold_the_input_condition(geom):
    """float64 and longdouble restatements agree to 1e-11 relative on every entry for the rows the device tests run."""
    x, y, lens = R.rows_for(geom)
    fr, sums, counts = R.batch(x, y, lens, geom)
    frl, sumsl, _ = R.batch(x, y, lens, geom, dtype=np.longdouble)
    e = max(R.rel_err(fr, frl), R.rel_err(sums, sumsl))
    nz = fr[fr != 0]
    print(f"\nSTFT distance input condition {geom}: float64 against longdouble {e:.3e}; smallest per-frame sum {nz.min():.3e}; counts {counts.tolist()}")
    assert [c % 16 for c in counts.tolist()] == [15, 0, 1]
    assert e <= R.INPUT_TOL
    alone = R.row(x[1, :lens[1]], y[1, :lens[1]], geom)
    assert np.array_equal(alone[0], fr[1, :alone[2]]) and np.array_equal(alone[1], sums[1]), "the garbage behind a row does not enter"
    assert not fr[0, counts[0]:].any()


def test_wrong_folds_show_in_the_first_and_last_frames_only():
    geom = (512, 50, 240)
    x = R.edge_signal(3000, geom[2])
    y = (x + 1e-3 * np.random.default_rng(1).standard_normal(len(x))).astype(np.float32)
    good = R.row(x, y, geom)[0]
    for fold in ("edge", "reflect_even"):
        bad = R.row(x, y, geom, fold=fold)[0]
        moved = np.abs(bad - good).max(axis=1) / np.abs(good).max(axis=1)
        where = np.nonzero(moved > 1e-6)[0]
        print(f"\nSTFT distance fold {fold}: frames moved {where.tolist()} of {len(good)}, by up to {moved.max():.3e}")
        assert len(where) and set(where.tolist()) <= {0, 1, 2, len(good) - 3, len(good) - 2, len(good) - 1}
        assert moved[0] > 1e-6 and moved[-1] > 1e-6


def _stand_in(x, y, lengths, resolution):
    nfft, hop, win = resolution
    _, sums, counts = R.batch(x.numpy(), y.numpy(), None if lengths is None else lengths.tolist(), (nfft, hop, win))
    return torch.from_numpy(sums), torch.from_numpy(counts)


def test_audio_stft_distance_with_a_stand_in_for_the_device_call():
    lens = [4000, 2600, 700]                                              # 700 samples: frames at 512 and 1024, none at 2048
    pairs = []
    for i, n in enumerate(lens):
        c = R.speech_like(n, seed=30 + i, fs=R.FS)
        pairs.append((c, R.processed(c, R.SNR_DB, seed=30 + i)))
    x, y, _ = R.padded(pairs)
    out = audio.stft_distance(torch.from_numpy(x), torch.from_numpy(y), lengths=lens, rows=_stand_in)
    assert set(out) == {"sc", "log_mag", "lsd_db", "mstft", "per_resolution", "frames"}
    assert all(out[k].dtype == torch.float64 and out[k].shape == (3,) for k in ("sc", "log_mag", "lsd_db", "mstft"))
    per = []
    for nfft, hop, win in R.RESOLUTIONS:
        _, sums, counts = R.batch(x, y, lens, (nfft, hop, win))
        per.append(R.figures(sums, counts, nfft) + (counts,))
    assert out["frames"].tolist() == np.stack([p[3] for p in per], axis=1).tolist() and out["frames"][2].tolist() == [1 + 700 // 120, 0, 1 + 700 // 50]
    for r, p in enumerate(out["per_resolution"]):
        assert (p["n_fft"], p["hop"], p["win"]) == R.RESOLUTIONS[r]
        for k, v in zip(("sc", "log_mag", "lsd_db"), per[r][:3]):
            assert np.allclose(p[k].numpy(), v, rtol=1e-14, atol=0, equal_nan=True), (r, k)
    for i, k in enumerate(("sc", "log_mag", "lsd_db")):
        want = np.mean([p[i] for p in per], axis=0)
        assert np.allclose(out[k][:2].numpy(), want[:2], rtol=1e-14, atol=0) and torch.isnan(out[k][2]), k
    want = np.mean([p[0] + p[1] for p in per], axis=0)
    assert np.allclose(out["mstft"][:2].numpy(), want[:2], rtol=1e-14, atol=0) and torch.isnan(out["mstft"][2])
    assert not torch.isnan(out["per_resolution"][0]["sc"][2]) and torch.isnan(out["per_resolution"][1]["sc"][2]), "NaN only where no frame"
    assert (out["sc"][:2] > 0).all() and (out["lsd_db"][:2] > 0).all()
    one = audio.stft_distance(torch.from_numpy(x[0, :lens[0]]), torch.from_numpy(y[0, :lens[0]]), rows=_stand_in)
    assert one["mstft"].shape == (1,) and float(one["mstft"][0]) == float(out["mstft"][0]), "a 1-D input is the same row"
    small = audio.stft_distance(torch.from_numpy(x), torch.from_numpy(y), lengths=lens, resolutions=[(64, 10, 24)], rows=_stand_in)
    assert small["frames"].tolist() == [[401], [261], [71]] and len(small["per_resolution"]) == 1


def test_argument_checks():
    with pytest.raises(ValueError):
        audio.stft_distance(torch.zeros(2, 4000), torch.zeros(2, 4001))
    with pytest.raises(ValueError):
        audio.stft_distance(np.zeros(4000, np.float32), np.zeros(4000, np.float32))
    with pytest.raises(ValueError):
        audio.stft_distance(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3))
    with pytest.raises(ValueError, match="resolutions"):
        audio.stft_distance(torch.zeros(2, 4000), torch.zeros(2, 4000), resolutions=[], rows=_stand_in)
    with pytest.raises(ValueError, match="lengths"):
        audio.stft_distance(torch.zeros(2, 4000), torch.zeros(2, 4000), lengths=[1, 2, 3], rows=_stand_in)
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.stft_distance(torch.zeros(2, 4000), torch.zeros(2, 4000))
    ns = lambda **kw: argparse.Namespace(**{**dict(vocoder_report="clean/filelist.txt", batch_size=4, sample_rate=None, prepare_dataset=None, synthetic=True,
                                                   vocoder_path=None, spectral_distance=True), **kw})
    assert cli.validate_args(ns()) is not None
    with pytest.raises(AssertionError, match="--spectral_distance"):
        cli.validate_args(ns(vocoder_report=None, ids="0 1 0", file=None, phonemes=None))
    with pytest.raises(AssertionError, match="--spectral_distance"):
        cli.validate_args(ns(vocoder_report=None, prepare_dataset="raw.txt", out_dir="clean", peak=0.95))


def test_vocoder_summary_with_the_distance_keys():
    keys = cli.VOCODER_REPORT_KEYS + cli.VOCODER_DISTANCE_KEYS
    assert cli.VOCODER_DISTANCE_KEYS == ("mstft", "sc", "log_mag", "lsd_db")
    base = {"stoi": 0.9, "estoi": 0.8, "mel_l1": 0.3, "lufs_shift": -0.5}
    files = [{"path": "a", **base, "mstft": 1.5, "sc": 0.5, "log_mag": 1.0, "lsd_db": 6.0},
             {"path": "b", **base, "mstft": 2.5, "sc": 0.7, "log_mag": 1.8, "lsd_db": 9.0},
             {"path": "c", **{k: None for k in keys}}]
    s = cli.vocoder_summary(files, keys=keys)
    assert s["files"] == 3 and s["unscored"] == ["c"]
    assert s["mstft"] == {"mean": 2.0, "max": 2.5} and s["lsd_db"] == {"mean": 7.5, "max": 9.0} and s["sc"]["max"] == 0.7 and s["log_mag"]["max"] == 1.8
    assert set(s["stoi"]) == {"mean", "min"}, "the scores keep their minimum: higher is better there"
    assert cli.vocoder_summary(files[2:], keys=keys)["mstft"] == {"mean": None, "max": None}
    assert set(cli.vocoder_summary(files)) == {"files", "unscored", "stoi", "estoi", "mel_l1", "lufs_shift"}, "without the keys: the summary as it was"


def test_header_declares_and_library_exports_ev_stft_dist():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    for name in ("ev_load_stft_dist", "ev_stft_dist"):
        assert re.search(rf"\bint\s+{name}\s*\(\s*ev_handle\s*\*", header), name
        assert re.search(rf"\*\s+{name}\s+<-\s+no counterpart; Yamamoto et al\. 2020 \(multi-resolution STFT loss\) is the model", header), name
        assert re.search(rf"#define\s+EV_ABI_VERSION\s+4\b[^\n]*\b{name}\b", header), f"{name}: the additions list of the ABI comment"
        assert name in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, "ev_load_stft_dist") and hasattr(lib, "ev_stft_dist")
