"""ev_mel_spectrogram on the MI355X, through the C ABI, against the fp64 yardstick of tests/mel_ref.py.

The yardstick is the reference's call sequence (reflect pad 384, torch.stft(center=False), periodic Hann, sqrt(re^2 + im^2 + 1e-9),
filter bank, log(clamp(., 1e-5))) in float64 on the CPU; tests/test_audio_host.py pins it to the reference function's own output.

Gate.  The reference's own arithmetic — the same sequence in float32 on the CPU — was measured against the yardstick on exactly the
CASES below (max and RMS in log units over the mel bins whose fp64 energy is above the 1e-5 clamp):
    noise 1 / 1e-2 / 1e-4, mixed rows      max 4.3e-7 .. 6.8e-6    RMS 1.0e-7 .. 2.9e-7
    48 sines over a 1e-4 floor, 861 frames max 3.3e-4              RMS 7.4e-6
    chirp over a 1e-3 floor                max 6.4e-4              RMS 1.9e-5      <- the worst of both
(log units magnify float32's absolute spectral error in the quiet bins beside a loud component, hence the spread.)  The engine is
gated at 3x the worst figure, as the decoder and vocoder modules gate at ~3x their worst measured value:
    GATE_MAX = 1.92e-3,  GATE_RMS = 5.67e-5   on every case.
Both figures print per case with -s (MELERR lines: the float32 reference measured live, then the engine).  Bins at or below the clamp
are compared after the clamp only (against log(1e-5), same bound); they are at most 10 % of the bins of every signal but `silent`.
Mutants (the 1e-9 outside the root; a symmetric Hann window) exceed the gate on the low-amplitude and sine cases.

Measured on one MI355X (the float32 reference on that host: worst 7.5e-4 / 2.0e-5, the chirp): engine max / RMS
    noise and mixed cases 5.8e-7 .. 3.0e-5 / 1.2e-7 .. 4.5e-7,  sines 861 frames 9.8e-4 / 2.6e-5,  chirp 8.2e-4 / 2.6e-5,
    committed fixture against the reference's own float32 output 1.9e-6 / 2.7e-7;  worst: 0.51 x GATE_MAX, 0.45 x GATE_RMS.
Run time of this module: 6 s.

The round trip (mel -> Generator V1 with synthetic weights -> mel_reconstruction_error) is a consistency check of the plumbing: with
untrained weights the value itself means nothing.
"""
import math
import os

import numpy as np
import pytest
import torch

import mel_ref as R
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, EvLibraryError

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE_MAX, GATE_RMS = 1.92e-3, 5.67e-5          # 3 x (6.40e-4, 1.89e-5): the float32 reference's worst case (module docstring)
CASES = [("noise1", 3, 768, 80), ("noise1e-2", 1, 512, 80), ("noise1e-4", 3, 256 * 516, 80), ("sines", 1, 256 * 861, 80),
         ("sines", 3, 768, 100), ("chirp", 3, 256 * 516, 100), ("silent", 1, 256 * 516, 80), ("mixed", 64, 256 * 516, 80),
         ("mixed", 64, 512, 100), ("noise1e-4", 64, 768, 80)]
MUTANT_CASES = [("noise1e-4", 3, 256 * 516, 80), ("sines", 1, 256 * 861, 80), ("mixed", 64, 512, 100)]
_BASIS = {}


def basis(n_mels):
    if n_mels not in _BASIS:
        _BASIS[n_mels] = audio.mel_filterbank(R.SR, R.N_FFT, n_mels, R.FMIN, R.FMAX)
    return _BASIS[n_mels]


@pytest.fixture(scope="module")
def engines():
    e = {}
    for n in (80, 100):
        e[n] = Engine(0)
        e[n].load_mel_basis(basis(n))
    return e


def _gate(tag, got, y, b, clamp_share_max=0.10):
    mx, rms, share, cmax = R.mel_errors(got, y, b)
    print(f"MELERR {tag}: engine max {mx:.2e} rms {rms:.2e}  clamped share {share:.3f} (max there {cmax:.1e})  gate {GATE_MAX:.2e} / {GATE_RMS:.2e}")
    assert torch.isfinite(torch.as_tensor(got)).all()
    assert share <= clamp_share_max, (tag, share)
    assert mx <= GATE_MAX and rms <= GATE_RMS and cmax <= GATE_MAX, (tag, mx, rms, cmax)


@pytest.mark.parametrize("kind,B,L,n_mels", CASES, ids=[f"{k}-B{b}-L{l}-m{m}" for k, b, l, m in CASES])
def test_parity_with_the_fp64_yardstick(engines, kind, B, L, n_mels):
    y = R.signal(kind, B, L, seed=B + L)
    b = basis(n_mels)
    rmx, rrms, _, _ = R.mel_errors(R.mel_yardstick(y, b, torch.float32), y, b)
    print(f"\nMELERR {kind} B{B} L{L} m{n_mels}: float32 reference max {rmx:.2e} rms {rrms:.2e}")
    assert rmx <= GATE_MAX / 3 * 1.5 and rrms <= GATE_RMS / 3 * 1.5, "the float32 reference moved: the gate constants are stale"
    got = engines[n_mels].mel_spectrogram(y.to(DEV))
    assert tuple(got.shape) == (B, n_mels, L // 256) and got.dtype == torch.float32
    _gate(f"{kind} B{B} L{L} m{n_mels}", got, y, b, clamp_share_max=1.0 if kind == "silent" else 0.10)
    if kind == "silent":
        fr = R.silent_frames(L)
        const = R.silent_constant(b)                                   # log(max(sum w * sqrt(1e-9), 1e-5)) per mel bin, fp64
        assert len(fr) > 100 and float((const - math.log(1e-5)).abs().max()) == 0.0
        z = got[0].cpu()[:, fr]
        assert float((z.double() - const[:, None]).abs().max()) <= 2.0 ** -20, "one float32 ulp of log(1e-5)"
        assert bool((z == z[0, 0]).all()), "every silent frame, every mel bin: the same bits"


def test_committed_fixture_against_the_reference_output(engines):
    with np.load(os.path.join(REPO, "tests", "golden", "mel_vectors.npz")) as z:
        y, mel = torch.from_numpy(z["y"]), torch.from_numpy(z["mel"])
    got = engines[80].mel_spectrogram(y.to(DEV)).cpu()
    d = (got.double() - mel.double()).abs()
    print(f"\nMELERR fixture: engine vs the reference's float32 output, max {float(d.max()):.2e} rms {float(d.pow(2).mean().sqrt()):.2e}")
    assert float(d.max()) <= GATE_MAX and float(d.pow(2).mean().sqrt()) <= GATE_RMS
    _gate("fixture (fp64)", got, y, basis(80))


@pytest.mark.parametrize("kind,B,L,n_mels", MUTANT_CASES)
def test_mutants_exceed_the_gate(kind, B, L, n_mels):
    y = R.signal(kind, B, L, seed=B + L)
    b = basis(n_mels)
    for name, kw in (("1e-9 outside the root", dict(eps_inside=False)), ("symmetric Hann", dict(periodic=False))):
        mx, rms, _, _ = R.mel_errors(R.mel_yardstick(y, b, **kw), y, b)
        print(f"\nMELERR mutant {name} on {kind} B{B} L{L}: max {mx:.2e} rms {rms:.2e}")
        assert mx > GATE_MAX and rms > GATE_RMS, (name, kind, mx, rms)


def test_public_function_scale_shift_and_caching():
    y = R.signal("noise1e-2", 3, 256 * 40, seed=5).to(DEV)
    plain = audio.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000, center=False)
    _gate("public mel_spectrogram", plain, y.cpu(), basis(80))
    n_eng = len(audio._engines)
    assert torch.equal(plain, audio.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000)), "two calls, the same bits"
    assert len(audio._engines) == n_eng, "handle and filter bank are cached per (device, sr, n_mels, fmin, fmax)"
    mean, std = -6.8566, 2.6098
    norm = audio.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000, out_scale=1.0 / std, out_shift=-mean / std)
    assert float((norm - (plain - mean) / std).abs().max()) <= 1e-6
    full = audio.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, None)
    assert len(audio._engines) == n_eng + 1
    _gate("fmax=None (513 bins in LDS)", full, y.cpu(), audio.mel_filterbank(22050, 1024, 80, 0, None))


def test_arithmetic_settings_streams_and_repeats_give_the_same_bits(engines):
    eng = engines[80]
    y = R.signal("mixed", 64, 256 * 132, seed=9).to(DEV)              # large enough for the balanced conv builds
    outs = []
    for s in (16, 6, 0, 16):
        eng.set_arithmetic(s)
        outs.append(eng.mel_spectrogram(y))
    assert all(torch.equal(outs[0], o) for o in outs[1:]), "the path is fp32-MFMA only"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o2 = eng.mel_spectrogram(y)
    side.synchronize()
    assert torch.equal(outs[0], o2)
    assert torch.equal(outs[0], eng.mel_spectrogram(y))
    _gate("mixed B64 L33792", outs[0], y.cpu(), basis(80))


def test_reserved_handle_does_not_allocate():
    eng = Engine(0)
    eng.load_mel_basis(basis(80))
    B, T = 4, 96
    eng.reserve(B, 0, 0, T)
    n0 = eng.alloc_count()
    y = R.signal("noise1e-2", B, 256 * T, seed=1).to(DEV)
    a = eng.mel_spectrogram(y)
    b = eng.mel_spectrogram(y[:2, : 256 * 40].contiguous())
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0
    _gate("reserved", a, y.cpu(), basis(80))
    assert torch.equal(b, eng.mel_spectrogram(y[:2, : 256 * 40].contiguous()))
    eng.close()


def test_denoiser_on_the_same_handle_is_not_disturbed():
    g = torch.Generator().manual_seed(11)
    wav = (torch.randn(3, 256 * 48, generator=g) * 0.1).to(DEV)
    bias = torch.rand(513, generator=g).to(DEV)
    fresh = Engine(0)
    want, want_mag = fresh.denoise(wav, bias, 0.05), fresh.stft_magnitude(wav)
    torch.cuda.synchronize()
    fresh.close()
    eng = Engine(0)
    eng.load_mel_basis(basis(80))
    before = eng.denoise(wav, bias, 0.05)
    m1 = eng.mel_spectrogram(R.signal("noise1", 5, 256 * 64, seed=2).to(DEV))       # a larger scratch plan than the denoiser's
    after, mag = eng.denoise(wav, bias, 0.05), eng.stft_magnitude(wav)
    m2 = eng.mel_spectrogram(R.signal("noise1", 5, 256 * 64, seed=2).to(DEV))
    assert torch.equal(before, want) and torch.equal(after, want) and torch.equal(mag, want_mag)
    assert torch.equal(m1, m2)
    eng.close()


def test_errors_name_the_cause():
    eng = Engine(0)
    y = torch.zeros(1, 1024, device=DEV)
    with pytest.raises(EvLibraryError, match="mel basis not loaded"):
        eng.mel_spectrogram(y)
    with pytest.raises(EvLibraryError, match="n_freq"):
        eng.load_mel_basis(np.zeros((80, 512), np.float32))
    with pytest.raises(EvLibraryError, match="n_mels"):
        eng.load_mel_basis(np.zeros((129, 513), np.float32))
    eng.load_mel_basis(basis(80))
    for bad in (torch.zeros(1, 256, device=DEV), torch.zeros(1, 1000, device=DEV)):
        with pytest.raises(EvLibraryError, match="multiple of 256"):
            eng.mel_spectrogram(bad)
    eng.close()


def test_a_gapped_basis_gives_the_dense_product():
    """Rows that are not one contiguous run (and an all-zero row, and one reloaded bank) still give the matrix product."""
    g = torch.Generator().manual_seed(4)
    b = basis(80).copy()
    b[3, 200:260] = 0.01                          # a second run far from the first
    b[10, :] = 0.0                                # an empty filter
    b[20, 512] = 0.02                             # the Nyquist bin: all 513 bins go through LDS
    b[40] = (torch.rand(513, generator=g) * 0.01).numpy()
    eng = Engine(0)
    eng.load_mel_basis(basis(80))
    y = R.signal("noise1e-2", 2, 256 * 40, seed=8)
    first = eng.mel_spectrogram(y.to(DEV))
    eng.load_mel_basis(b)                         # replaces the bank
    got = eng.mel_spectrogram(y.to(DEV))
    _gate("gapped basis", got, y, b, clamp_share_max=0.05)
    assert float((got[:, 10] - math.log(1e-5)).abs().max()) <= 2.0 ** -20
    eng.load_mel_basis(basis(80))
    assert torch.equal(first, eng.mel_spectrogram(y.to(DEV)))
    eng.close()


def test_round_trip_through_the_vocoder():
    """mel_reconstruction_error at B = 8 x 128 frames on the synthetic V1 generator equals the same quantity from the fp64 yardstick
    on the vocoder's output.  Untrained weights: the value itself means nothing, this checks the plumbing."""
    from emojivoice_amd.hifigan import synthetic

    voc = synthetic(DEV)
    g = torch.Generator().manual_seed(21)
    mel = (torch.randn(8, 80, 128, generator=g) * 2.0 - 5.0).to(DEV)
    lengths = torch.tensor([128, 127, 96, 64, 33, 17, 2, 1])
    err = audio.mel_reconstruction_error(voc, mel, lengths.to(DEV))
    err_all = audio.mel_reconstruction_error(voc, mel)
    assert tuple(err.shape) == (8,) and err.is_cuda and torch.isfinite(err).all() and torch.isfinite(err_all).all()
    wav = voc(mel).squeeze(1).cpu()
    ref = R.mel_yardstick(wav, basis(80))
    d = (mel.cpu().double() - ref).abs()
    want_all = d.mean(dim=(1, 2))
    want = torch.stack([d[i, :, : int(n)].mean() for i, n in enumerate(lengths)])
    print(f"\nMELERR round trip: reconstruction error {err.cpu().tolist()}  (fp64 {want.tolist()})")
    # a mean of absolute differences moves by at most the largest difference between the two mels: the parity gate
    assert float((err.cpu().double() - want).abs().max()) <= GATE_MAX
    assert float((err_all.cpu().double() - want_all).abs().max()) <= GATE_MAX


def test_cli_mel_from_wav_and_copy_synthesis(tmp_path):
    from emojivoice_amd.cli import cli, write_wav_pcm24

    g = torch.Generator().manual_seed(33)
    x = (torch.randn(10000, generator=g) * 0.1).numpy()
    p = tmp_path / "voice.wav"
    write_wav_pcm24(p, x)
    cli(["--mel_from_wav", str(p), "--synthetic"])
    mel = np.load(f"{p}.mel.npy")
    assert mel.shape == (80, 39) and mel.dtype == np.float32            # 10000 samples trimmed to 39 * 256
    y = torch.from_numpy(audio.read_wav_pcm(p)[: 39 * 256]).unsqueeze(0)
    _gate("cli --mel_from_wav", torch.from_numpy(mel).unsqueeze(0), y, basis(80))
    assert audio.read_wav_pcm(f"{p}.copysyn.wav").shape == (39 * 256,)
