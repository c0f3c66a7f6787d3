"""Host side of the analysis path (emojivoice_amd/audio.py), no GPU: the mel filter bank against an independent restatement of
the published definition, the fp64 yardstick of tests/test_gpu_mel.py against the reference's own output (tests/golden/mel_vectors.npz,
written by tests/golden/make_mel_golden.py), the argument checks of ``mel_spectrogram``, the wav reader, the two new C-ABI symbols."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mel_ref as R
from emojivoice_amd import _lib, audio
from emojivoice_amd.cli import write_wav_pcm24

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restated_bank(sr, n_fft, n_mels, fmin, fmax):
    """Slaney-scale, Slaney-normalised triangles, evaluated bin by bin from the two ramps (float64; scalar math only)."""
    f_sp, logstep = 200.0 / 3.0, math.log(6.4) / 27.0

    def to_mel(f):
        return f / f_sp if f < 1000.0 else 15.0 + math.log(f / 1000.0) / logstep

    def to_hz(m):
        return f_sp * m if m < 15.0 else 1000.0 * math.exp(logstep * (m - 15.0))

    lo, hi = to_mel(float(fmin)), to_mel(float(fmax))
    edges = [to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    out = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float64)
    for m in range(n_mels):
        f_lo, f_c, f_hi = edges[m], edges[m + 1], edges[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * sr / n_fft
            up, down = (f - f_lo) / (f_c - f_lo), (f_hi - f) / (f_hi - f_c)
            out[m, k] = max(0.0, min(up, down)) * 2.0 / (f_hi - f_lo)
    return out


def _ulp_close(a32, b64):
    """a32 (float32) within 1 ulp of float32 of the float64 values b64."""
    b32 = b64.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(b32), np.float32(np.finfo(np.float32).tiny)))
    return bool(np.all(np.abs(a32.astype(np.float64) - b32.astype(np.float64)) <= ulp.astype(np.float64)))


@pytest.mark.parametrize("n_mels,fmax", [(80, 8000), (100, 8000), (80, None)])
def test_mel_filterbank_matches_the_definition(n_mels, fmax):
    w = audio.mel_filterbank(22050, 1024, n_mels, 0, fmax)
    assert w.shape == (n_mels, 513) and w.dtype == np.float32
    assert np.all(w >= 0) and np.all(np.isfinite(w))
    peaks = []
    for row in w:
        nz = np.flatnonzero(row)
        assert nz.size >= 1 and np.array_equal(nz, np.arange(nz[0], nz[-1] + 1)), "every filter is one contiguous run of bins"
        peaks.append(int(row.argmax()))
    assert all(b > a for a, b in zip(peaks, peaks[1:])), "peaks strictly increasing in frequency"
    assert np.all(w[:, 0] == 0), "fmin = 0: no weight on the DC bin"
    top = 11025.0 if fmax is None else float(fmax)
    last = int(math.floor(top * 1024 / 22050))
    if last < 512:
        assert np.all(w[:, last + 1:] == 0), "nothing above fmax"
    if fmax == 8000:
        assert last == 371 and np.any(w[:, 371] > 0)                      # bin 371 = 7988 Hz is the last below 8 kHz
    assert _ulp_close(w, _restated_bank(22050, 1024, n_mels, 0, top))
    if fmax is None:
        assert np.array_equal(w, audio.mel_filterbank(22050, 1024, n_mels, 0, 11025.0))


def test_mel_scale_landmarks():
    """The published constants: 1 kHz is mel 15, 6.4 kHz is 27 mels further, the scale is continuous and invertible."""
    assert float(audio.hz_to_mel(1000.0)) == pytest.approx(15.0, abs=1e-12)
    assert float(audio.hz_to_mel(6400.0)) == pytest.approx(42.0, abs=1e-9)
    f = np.array([0.0, 100.0, 999.9, 1000.0, 1000.1, 4000.0, 8000.0, 11025.0])
    assert np.allclose(audio.mel_to_hz(audio.hz_to_mel(f)), f, rtol=1e-12, atol=1e-9)


def test_fp64_yardstick_is_pinned_to_the_reference_function():
    """The reference's float32 output for the committed signal against the fp64 yardstick: 1e-5 in log units on every mel bin."""
    with np.load(os.path.join(REPO, "tests", "golden", "mel_vectors.npz")) as z:
        y, mel = torch.from_numpy(z["y"]), torch.from_numpy(z["mel"])
        args = {k: int(z[k]) for k in ("n_fft", "num_mels", "sampling_rate", "hop_size", "win_size", "fmin", "fmax")}
    assert tuple(y.shape) == (2, 8192) and tuple(mel.shape) == (2, 80, 32) and mel.dtype == torch.float32
    assert (args["n_fft"], args["hop_size"], args["win_size"]) == (R.N_FFT, R.HOP, R.N_FFT)
    basis = audio.mel_filterbank(args["sampling_rate"], args["n_fft"], args["num_mels"], args["fmin"], args["fmax"])
    ref = R.mel_yardstick(y, basis)
    err = float((ref - mel.double()).abs().max())
    print(f"\nMELERR fixture: fp64 yardstick vs the reference's float32 output, max {err:.2e} log units (bound 1e-5)")
    assert err <= 1e-5
    assert float(mel.min()) > math.log(R.CLAMP) + 1.0, "the fixture stays clear of the clamp"
    # the mutants the GPU gate must catch are not equivalent to the yardstick on this signal either
    assert float((R.mel_yardstick(y, basis, periodic=False) - ref).abs().max()) > 1e-3


def test_test_signals_stay_above_the_clamp():
    """Item 4 of the GPU checks: at most 10 % of the mel bins of every signal but the silent one lie at or below the clamp (fp64)."""
    for kind, B, L, n_mels in [("noise1", 3, 768, 80), ("noise1e-2", 1, 512, 80), ("noise1e-4", 3, 768, 80), ("sines", 1, 256 * 40, 80),
                               ("chirp", 3, 256 * 64, 100), ("mixed", 6, 512, 100)]:
        y = R.signal(kind, B, L, seed=B + L)
        e = R.mel_yardstick(y, audio.mel_filterbank(22050, 1024, n_mels, 0, 8000), log=False)
        assert float((e <= R.CLAMP).double().mean()) <= 0.10, kind
    L = 256 * 64
    e = R.mel_yardstick(R.signal("silent", 1, L), audio.mel_filterbank(22050, 1024, 80, 0, 8000))
    fr = R.silent_frames(L)
    assert len(fr) >= 10
    const = R.silent_constant(audio.mel_filterbank(22050, 1024, 80, 0, 8000))
    assert float((e[0][:, fr] - const[:, None]).abs().max()) <= 1e-12
    assert float((const - math.log(R.CLAMP)).abs().max()) == 0.0, "sum w * sqrt(1e-9) is below the clamp for every Slaney filter: exactly log(1e-5)"


@pytest.mark.parametrize("kw,word", [(dict(n_fft=2048), "n_fft"), (dict(win_size=800), "win_size"), (dict(hop_size=128), "hop_size"),
                                     (dict(center=True), "center"), (dict(num_mels=0), "num_mels"), (dict(num_mels=129), "num_mels")])
def test_mel_spectrogram_names_the_unsupported_argument(kw, word):
    args = dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000, center=False)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        audio.mel_spectrogram(torch.zeros(1, 1024), **args)


@pytest.mark.parametrize("shape", [(1, 1000), (1, 256), (2, 0), (1024,)])
def test_mel_spectrogram_rejects_lengths_the_engine_cannot_frame(shape):
    with pytest.raises(ValueError, match="256|\\(B, L\\)"):
        audio.mel_spectrogram(torch.zeros(*shape), 1024, 80, 22050, 256, 1024, 0, 8000)


def test_no_cpu_fallback_for_the_analysis_path():
    with pytest.raises(_lib.EvLibraryError):                          # a host tensor is never computed on the host
        audio.mel_spectrogram(torch.zeros(1, 1024), 1024, 80, 22050, 256, 1024, 0, 8000)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.EvLibraryError):
            audio._engine_for(torch.device("cuda", 0), 22050, 80, 0, 8000)


def test_new_symbols_are_exported_and_declared():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(REPO, "include", "emojivoice.h")).read()
    for name in ("ev_load_mel_basis", "ev_mel_spectrogram"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.EXPORTS and f"int {name}(" in header
    assert hasattr(_lib.Engine, "load_mel_basis") and hasattr(_lib.Engine, "mel_spectrogram")


def test_wav_reader_round_trips_the_24_bit_writer(tmp_path):
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(4096, generator=g) * 2 - 1).numpy().astype(np.float32)
    x[:4] = [1.0, -1.0, 0.0, -2.0 ** -23]
    p = tmp_path / "a.wav"
    write_wav_pcm24(p, x)
    back = audio.read_wav_pcm(p)
    q = np.round(np.clip(x.astype(np.float64), -1, 1) * (2**23 - 1))
    assert back.dtype == np.float32 and np.array_equal(back, (q / (2**23 - 1)).astype(np.float32))
    p2 = tmp_path / "b.wav"
    write_wav_pcm24(p2, back)
    assert open(p, "rb").read() == open(p2, "rb").read(), "write -> read -> write is the identity on the file"
    # 16-bit files
    import wave
    s16 = np.array([0, 1, -1, 32767, -32768, 12345], dtype="<i2")
    with wave.open(str(tmp_path / "c.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(22050); f.writeframes(s16.tobytes())
    assert np.array_equal(audio.read_wav_pcm(tmp_path / "c.wav"), (s16.astype(np.float64) / 32768).astype(np.float32))
    with wave.open(str(tmp_path / "d.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000); f.writeframes(s16.tobytes())
    with pytest.raises(ValueError, match="Hz"):
        audio.read_wav_pcm(tmp_path / "d.wav")
