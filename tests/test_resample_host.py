"""Host side of the resampler and of the dataset statistics: the filter design against scipy's, an fp64 numpy restatement of the
C ABI's formula against ``scipy.signal.resample_poly``, the rate reduction, ``read_wav``, the statistics formula against a float64
restatement of the reference's ``compute_data_statistics``, and the C ABI's declarations and exports.  No GPU.  (The argument
refusals of ev_load_resampler / ev_resample need a handle, hence a device: they are in tests/test_gpu_resample.py.)

Filter: ``audio.resample_filter`` is numpy (np.sinc, np.kaiser) where scipy's firwin goes through scipy.special; in float64 the two agree
to ~1e-15 of the largest tap (bound here: 1e-12).  After the one rounding to float32 the taps are bit-equal for every pair below; the
test allows 1 ulp only for a tap whose float64 value lies within 1e-12 (relative) of a float32 rounding boundary, and on this scipy
(1.15) NO pair needs that allowance (the test prints the count per pair).
"""
import json
import math
import os
import re
import subprocess
import wave

import numpy as np
import pytest
import torch
from scipy import signal as sps

from emojivoice_amd import _lib, audio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ev_load_resampler", "ev_resample", "ev_mel_stats")
PAIRS = [(1, 2), (147, 320), (320, 147), (441, 320), (160, 147)]


def resample_direct(x, taps, up, down):
    """The formula of include/emojivoice.h in float64: y[n] = sum_i x[i] taps[n down - i up + c], c = (n_taps - 1) / 2, for
    0 <= n < ceil(L up / down), x zero outside [0, L)."""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    L, nt = len(x), len(taps)
    c = (nt - 1) // 2
    n_out = -(-L * up // down)
    y = np.zeros(n_out)
    for n in range(n_out):
        q = n * down + c
        lo = max(0, -((nt - 1 - q) // up))          # smallest i with q - i up <= n_taps - 1
        hi = min(L - 1, q // up)                    # largest i with q - i up >= 0
        if hi >= lo:
            i = np.arange(lo, hi + 1)
            y[n] = math.fsum(x[i] * taps[q - i * up])
    return y


@pytest.mark.parametrize("up,down", PAIRS)
def test_filter_is_scipys_default_design(up, down):
    m = max(up, down)
    want = sps.firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    got64 = audio._resample_filter64(up, down)
    assert got64.dtype == np.float64 and got64.shape == (20 * m + 1,)
    err = float(np.abs(got64 - want).max())
    got, w32 = audio.resample_filter(up, down), want.astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, got64.astype(np.float32)), "computed in float64, rounded once"
    differ = np.flatnonzero(got != w32)
    print(f"\nRSFILT {up}/{down}: float64 max |diff| {err:.2e}; float32 taps that differ: {len(differ)} of {len(got)}")
    assert err <= 1e-12
    for k in differ:                                 # allowed only on a rounding boundary, and then by one ulp
        lo, hi = sorted((float(got[k]), float(w32[k])))
        assert np.nextafter(np.float32(lo), np.float32(np.inf)) == np.float32(hi), (up, down, k)
        assert abs(want[k] - 0.5 * (lo + hi)) <= 1e-12 * abs(want[k]), (up, down, k)
    assert abs(float(got64.sum()) - up) <= 1e-12 * up, "unit sum times the gain up"
    assert np.array_equal(got64, got64[::-1]) or float(np.abs(got64 - got64[::-1]).max()) <= 1e-15 * up


def test_filter_parameters():
    h = audio.resample_filter(1, 2, zeros=32, beta=12.0)
    assert h.shape == (2 * 32 * 2 + 1,)
    want = sps.firwin(129, 0.5, window=("kaiser", 12.0))
    assert float(np.abs(h.astype(np.float64) - want).max()) <= 2.0 ** -24
    assert audio.resample_filter(1, 1).shape == (21,)


@pytest.mark.parametrize("up,down,L", [(1, 2, 1025), (147, 320, 700), (320, 147, 301), (441, 320, 250), (160, 147, 333), (3, 7, 50), (3, 7, 1),
                                       (5, 3, 1), (7, 3, 2), (1, 1, 40)])
def test_formula_is_resample_poly(up, down, L):
    """Pins the centring (c = (n_taps - 1) / 2), scipy's trimming of the filter's delay and the output length; (3, 7) has 141 taps."""
    g = np.random.default_rng(100 * up + down + L)
    x = g.standard_normal(L)
    taps = audio._resample_filter64(up, down)
    if (up, down) == (3, 7):
        assert len(taps) == 141
    want = sps.resample_poly(x, up, down, padtype="constant")
    got = resample_direct(x, taps, up, down)
    assert got.shape == want.shape == (-(-L * up // down),)
    assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))
    # ... and with the taps handed over as an array scipy multiplies them by up itself (what the GPU test's yardstick relies on)
    t32 = audio.resample_filter(up, down).astype(np.float64)
    assert float(np.abs(resample_direct(x, t32, up, down) - sps.resample_poly(x, up, down, window=t32 / up, padtype="constant")).max()) <= 1e-12 * max(
        1.0, float(np.abs(want).max()))


def test_rates_are_reduced_and_equal_rates_short_cut():
    assert audio.resample_ratio(44100, 22050) == (1, 2)
    assert audio.resample_ratio(48000, 22050) == (147, 320)
    assert audio.resample_ratio(22050, 48000) == (320, 147)
    assert audio.resample_ratio(32000, 22050) == (441, 640)
    assert audio.resample_ratio(22050, 16000) == (320, 441)
    assert audio.resample_ratio(24000, 22050) == (147, 160)
    y = torch.zeros(2, 100)
    assert audio.resample(y, 22050, 22050) is y, "orig == new returns y itself (no device needed)"
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.resample(y, 44100, 22050)
    with pytest.raises(ValueError):
        audio.resample_ratio(0, 22050)


def _write_wav(path, q, rate, width, channels):
    """q: integer samples (frames, channels)."""
    q = np.asarray(q).reshape(-1, channels)
    if width == 2:
        raw = q.astype("<i2").tobytes()
    else:
        raw = (q.astype(np.int32).reshape(-1) & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw)


@pytest.mark.parametrize("rate,width,channels", [(44100, 2, 1), (48000, 2, 2), (44100, 3, 2), (48000, 3, 1), (22050, 3, 1)])
def test_read_wav(tmp_path, rate, width, channels):
    g = np.random.default_rng(rate + width + channels)
    full = 2 ** (8 * width - 1)
    q = g.integers(-full, full, size=(501, channels))
    q[0], q[1] = -full, full - 1
    p = tmp_path / "a.wav"
    _write_wav(p, q, rate, width, channels)
    y, sr = audio.read_wav(p)
    scale = 32768.0 if width == 2 else float(2 ** 23 - 1)
    want = (q.astype(np.float64) / scale).mean(axis=1).astype(np.float32)
    assert sr == rate and y.dtype == np.float32 and y.shape == (501,)
    assert np.array_equal(y, want), "channels averaged in float64, rounded once"
    if channels == 1 and rate == 22050:
        assert np.array_equal(y, audio.read_wav_pcm(p)), "mono at 22050 Hz: read_wav_pcm's samples"
    if rate != 22050 and channels == 1:
        with pytest.raises(ValueError, match="does not resample"):
            audio.read_wav_pcm(p)


def compute_data_statistics_fp64(batches, out_channels):
    """utils/generate_data_statistics.py:25-47 on zero-padded numpy batches, in float64 (the reference sums the padding too)."""
    total_sum = total_sq = 0.0
    total_len = 0
    for mels, lengths in batches:
        total_len += int(np.sum(lengths))
        total_sum += float(np.sum(mels.astype(np.float64)))
        total_sq += float(np.sum(np.power(mels.astype(np.float64), 2)))
    mean = total_sum / (total_len * out_channels)
    return {"mel_mean": mean, "mel_std": math.sqrt(total_sq / (total_len * out_channels) - mean ** 2)}


def test_data_statistics_formula():
    g = np.random.default_rng(5)
    batches = []
    for B, T in ((5, 37), (3, 64), (1, 9)):
        lengths = g.integers(1, T + 1, size=B)
        lengths[0] = T
        m = (g.standard_normal((B, 80, T)) * 2.1 - 5.5).astype(np.float32)
        for b, n in enumerate(lengths):
            m[b, :, n:] = 0.0
        batches.append((m, lengths))
    want = compute_data_statistics_fp64(batches, 80)

    def row_sums(mel, lengths):                      # what ev_mel_stats returns, in numpy: the valid cells only
        mel = mel.numpy().astype(np.float64)
        return np.stack([[mel[b, :, :n].sum(), (mel[b, :, :n] ** 2).sum()] for b, n in enumerate(np.asarray(lengths))])

    got = audio.data_statistics([(torch.from_numpy(m), torch.from_numpy(n)) for m, n in batches], 80, row_sums=row_sums)
    assert set(got) == {"mel_mean", "mel_std"} and all(isinstance(v, float) for v in got.values())
    assert abs(got["mel_mean"] - want["mel_mean"]) <= 1e-12 and abs(got["mel_std"] - want["mel_std"]) <= 1e-12
    assert abs(got["mel_mean"] + 5.5) < 0.05 and abs(got["mel_std"] - 2.1) < 0.05
    assert json.loads(json.dumps(got)) == got
    with pytest.raises(ValueError, match="channels"):
        audio.data_statistics([(torch.zeros(1, 40, 4), torch.tensor([4]))], 80, row_sums=row_sums)
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.data_statistics([(torch.zeros(1, 80, 4), torch.tensor([4]))], 80)


def test_header_declares_and_library_exports_the_new_calls():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    for n in NAMES:
        assert re.search(rf"\bint\s+{n}\s*\(\s*ev_handle\s*\*", header), f"{n} is not declared in include/emojivoice.h"
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
