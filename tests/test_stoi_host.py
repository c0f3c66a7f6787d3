"""CPU-side checks of the STOI / ESTOI path: the band table of ``audio.third_octave_bands``, the properties of the numpy restatement
(tests/stoi_ref.py) on the rows tests/test_gpu_stoi.py runs on the device — identical signals, the order of the three SNRs, the frame-count
rule, the input conditions — eight mutants of the restatement that must each show, ``audio.stoi`` with a stand-in for the device call, the
argument checks, and the C ABI's declaration and export.
"""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import stoi_ref as R
from emojivoice_amd import _lib, audio, cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def snr_rows():
    """One clean row of 20000 samples at 10 kHz against itself at +20, 0 and -10 dB SNR, through the restatement: computed once."""
    c = R.speech_like(20000, seed=0)
    return c, [R.processed(c, snr, seed=0) for snr in R.SNRS_DB], [R.stoi_row(c, R.processed(c, snr, seed=0), R.STANDARD) for snr in R.SNRS_DB]


def test_third_octave_bands_are_the_published_table():
    b = audio.third_octave_bands()
    assert b.dtype == np.int32 and b.shape == (15, 2) and b.tolist() == R.BANDS_15
    assert audio.third_octave_bands(10000, 512, 15, 150.0).tolist() == R.BANDS_15
    assert (b[1:, 0] == b[:-1, 1]).all(), "adjacent bands share their edge bin"
    w = audio.stoi_window(256)
    assert w.dtype == np.float64 and w.shape == (256,) and np.array_equal(w, np.hanning(258)[1:-1]) and w.min() > 0
    t = audio.stoi_twiddle(512)
    assert t.shape == (512, 2) and np.array_equal(t, R.STANDARD.twiddle) and t[0].tolist() == [1.0, 0.0]
    assert (audio.STOI_SILENCE_RATIO, audio.STOI_CLIP) == (R.SILENCE_RATIO, R.CLIP) and R.EPS == 2.0 ** -52
    assert (audio.STOI_WINDOW, audio.STOI_HOP, audio.STOI_NFFT, audio.STOI_SEGMENT) == (R.STANDARD.W, R.STANDARD.H, R.STANDARD.nfft, R.STANDARD.N)


def test_identical_signals_score_one_and_scores_fall_with_snr(snr_rows):
    c, _, res = snr_rows
    same = R.stoi_row(c, c, R.STANDARD)
    print(f"\nSTOI identical signals: 1 - STOI {1 - same['score'][0]:.3e}, 1 - ESTOI {1 - same['score'][1]:.3e}")
    assert same["score"][0] >= 1 - 1e-12 and same["score"][1] >= 1 - 1e-12
    for r, snr in zip(res, R.SNRS_DB):
        print(f"STOI {snr:+.0f} dB SNR: counts {r['counts']} margin {r['margin']:.3f} dB conditioning {r['conditioning']:.3f} "
              f"STOI {r['score'][0]:.4f} ESTOI {r['score'][1]:.4f}")
        assert r["counts"] == (155, 115, 85), "20000 samples: 155 frames; the gate removes a third"
        assert r["margin"] >= 1.0 and r["conditioning"] >= 0.05
    s = [r["score"] for r in res]
    assert 1 > s[0][0] > s[1][0] > s[2][0] > 0 and 1 > s[0][1] > s[1][1] > s[2][1] > 0, "both scores fall strictly with the SNR"
    assert s[0][0] > 0.9 and s[2][0] < 0.5 and s[2][1] < 0.15


def test_frame_count_rule():
    """The model frames with range(0, len - W, H): a row of exactly W + k H samples has k frames, not k + 1."""
    for g in (R.STANDARD, R.SMALL):
        W, H = g.W, g.H
        assert [g.frames(n) for n in (1, W - 1, W, W + 1, W + H, W + H + 1, W + 7 * H, W + 7 * H + 1)] == [0, 0, 0, 1, 1, 2, 7, 8]
        assert g.sizes(W + 40 * H) == (40, 39, max(39 - g.N + 1, 0))
    x = R.dense_row(9)[0]
    assert len(x) == R.SMALL.W + 8 * R.SMALL.H + 1
    for n, nf in ((len(x), 9), (len(x) - 1, 8), (R.SMALL.W, 0), (R.SMALL.W + 1, 1)):
        r = R.stoi_row(x[:n], x[:n], R.SMALL)
        assert r["counts"][0] == nf and r["counts"][1] == nf and r["tob"].shape[2] == max(nf - 1, 0), (n, r["counts"])


def test_device_cases_hold_the_input_conditions():
    x, y, lens = R.standard_rows()
    r = R.stoi(x, y, lens, R.STANDARD)
    assert r["counts"][:, 0].tolist() == [155, 103, 69] and (r["counts"][:, 2] > 0).all()
    assert r["margin"].min() >= R.MIN_MARGIN_DB and r["conditioning"].min() >= R.MIN_CONDITIONING
    alone = R.stoi_row(x[1, :lens[1]], y[1, :lens[1]], R.STANDARD)
    assert np.array_equal(alone["seg"], r["seg"][1, :alone["counts"][2]]), "the garbage behind a row does not enter"
    x, y, lens = R.small_rows()
    r = R.stoi(x, y, lens, R.SMALL)
    assert r["counts"].tolist() == R.SMALL_COUNTS
    scored = r["counts"][:, 0] > 0
    assert r["margin"][scored].min() >= R.MIN_MARGIN_DB and r["conditioning"].min() >= R.MIN_CONDITIONING
    z = R.stoi(np.zeros((1, 3000), np.float32), y[:1], None, R.SMALL)
    assert z["counts"].tolist() == [[92, 0, 0]] and not z["score"].any(), "an all-zero clean row keeps no frame"
    bad = R.stoi(x[:2], y[:2], [0, 3001], R.SMALL)
    assert not bad["counts"].any() and not bad["tob"].any()


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_each_mutant_of_the_restatement_shows(snr_rows, variant):
    """Every misreading must move a score of the 0 dB row by more than 1e-6 or change the mask.  The strictness of the mask shows only where a
    frame sits exactly on the threshold, so that one runs with the dynamic range at 0 dB, where the loudest frame itself does: the strict
    rule keeps no frame, the non-strict one keeps it."""
    c, ys, res = snr_rows
    if variant == "nonstrict_mask":
        strict = R.stoi_row(c, ys[1], R.STANDARD, dyn_range_db=0.0)
        loose = R.stoi_row(c, ys[1], R.STANDARD, variant, dyn_range_db=0.0)
        assert strict["counts"][1] == 0 and loose["counts"][1] >= 1
        return
    m = R.stoi_row(c, ys[1], R.STANDARD, variant)
    moved = max(abs(m["score"][0] - res[1]["score"][0]), abs(m["score"][1] - res[1]["score"][1]))
    mask = not np.array_equal(m["keep"], res[1]["keep"])
    print(f"\nSTOI mutant {variant}: scores {m['score'].tolist()} against {res[1]['score'].tolist()} (moved {moved:.3e}), mask changed: {mask}")
    assert moved > 1e-6 or mask


def _stand_in(x, y, lengths):
    r = R.stoi(x.numpy(), y.numpy(), None if lengths is None else lengths.tolist(), R.STANDARD)
    return torch.from_numpy(r["keep"]), torch.from_numpy(r["seg"]), torch.from_numpy(r["score"]), torch.from_numpy(r["counts"])


def test_audio_stoi_with_a_stand_in_for_the_device_call():
    x, y, lens = R.standard_rows()
    x = np.concatenate([x, x[:1]])
    y = np.concatenate([y, y[:1]])
    lens = lens + [3000]                                                  # 22 frames: no segment
    out = audio.stoi(torch.from_numpy(x), torch.from_numpy(y), sr=10000, lengths=lens, rows=_stand_in)
    ref = R.stoi(x, y, lens, R.STANDARD)
    assert set(out) == {"stoi", "estoi", "segments", "counts", "keep"} and out["stoi"].dtype == torch.float64
    assert np.array_equal(out["stoi"][:3].numpy(), ref["score"][:3, 0]) and np.array_equal(out["estoi"][:3].numpy(), ref["score"][:3, 1])
    assert out["counts"][3].tolist() == [22, ref["counts"][3, 1], 0]
    assert torch.isnan(out["stoi"][3]) and torch.isnan(out["estoi"][3]), "no segment: NaN, not a number that looks like a score"
    one = audio.stoi(torch.from_numpy(x[0]), torch.from_numpy(y[0]), sr=10000, rows=_stand_in)
    assert one["stoi"].shape == (1,) and float(one["stoi"][0]) == ref["score"][0, 0]


def test_argument_checks():
    with pytest.raises(ValueError):
        audio.stoi(torch.zeros(2, 4000), torch.zeros(2, 4001))
    with pytest.raises(ValueError):
        audio.stoi(np.zeros(4000, np.float32), np.zeros(4000, np.float32))
    with pytest.raises(ValueError):
        audio.stoi(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3))
    with pytest.raises(ValueError):
        audio.stoi(torch.zeros(2, 4000), torch.zeros(2, 4000), sr=0)
    with pytest.raises(ValueError, match="lengths"):
        audio.stoi(torch.zeros(2, 4000), torch.zeros(2, 4000), sr=10000, lengths=[1, 2, 3], rows=_stand_in)
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.stoi(torch.zeros(2, 4000), torch.zeros(2, 4000))
    ns = lambda **kw: argparse.Namespace(**{**dict(vocoder_report="clean/filelist.txt", batch_size=4, sample_rate=None, prepare_dataset=None, synthetic=True,
                                                   vocoder_path=None), **kw})
    assert cli.validate_args(ns()) is not None
    with pytest.raises(AssertionError, match="Batch size"):
        cli.validate_args(ns(batch_size=0))
    with pytest.raises(AssertionError, match="vocoder_path"):
        cli.validate_args(ns(synthetic=False))


def test_vocoder_summary_means_minima_and_unscored():
    files = [{"path": "a", "stoi": 0.9, "estoi": 0.8, "mel_l1": 0.3, "lufs_shift": -0.5}, {"path": "b", "stoi": 0.7, "estoi": 0.5, "mel_l1": 0.5, "lufs_shift": None},
             {"path": "c", "stoi": None, "estoi": None, "mel_l1": None, "lufs_shift": None}]
    s = cli.vocoder_summary(files)
    assert s["files"] == 3 and s["unscored"] == ["c"]
    assert abs(s["stoi"]["mean"] - 0.8) < 1e-15 and s["stoi"]["min"] == 0.7 and s["estoi"]["min"] == 0.5 and s["mel_l1"]["mean"] == 0.4
    assert s["lufs_shift"] == {"mean": -0.5, "min": -0.5}
    assert cli.vocoder_summary(files[2:])["stoi"] == {"mean": None, "min": None}


def test_header_declares_and_library_exports_ev_stoi():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    for name in ("ev_load_stoi", "ev_stoi"):
        assert re.search(rf"\bint\s+{name}\s*\(\s*ev_handle\s*\*", header), name
        assert re.search(rf"\*\s+{name}\s+<-\s+no counterpart; Taal et al\. 2011 / Jensen and Taal 2016 are the model", header), name
        assert re.search(rf"#define\s+EV_ABI_VERSION\s+4\b[^\n]*\b{name}\b", header), f"{name}: the additions list of the ABI comment"
        assert name in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, "ev_load_stoi") and hasattr(lib, "ev_stoi")
