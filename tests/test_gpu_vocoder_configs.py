"""HiFi-GAN V2 / V3 and an off-standard ResBlock2 config on the MI355X: against the reference's golden (itself fp32: RMS 1e-4 / L-inf 1e-3),
against the fp64 restatement (test_vocoder_configs.restate) at ragged and odd shapes under arithmetic settings 0 / 6 / 16, row by row at the
gates of test_gpu_vocoder_configs_fp64.py (which covers the remaining paths), the one-launch ResBlock2
(resblock2_h16_kernel) against the conv launches, and the callers that take any vocoder (Denoiser, Engine chunking, the CLI)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from emojivoice_amd import weights as W
from emojivoice_amd.hifigan import AttrDict, Generator, v1, v3
from oracle import matcha_oracle as O
from test_vocoder_configs import NAMES, WIDE_LAST, golden_config, golden_vocoder, restate
from vocoder_ref import check

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAV_RMS, WAV_LINF = 1e-4, 1e-3


def _vocoder(h):
    g = Generator(AttrDict(h)).to("cuda:0")
    g.load_state_dict(W.synthetic_hifigan_state(h))
    g.eval()
    g.remove_weight_norm()
    return g


@pytest.fixture(scope="module")
def gold():
    return golden_vocoder()


@pytest.fixture(scope="module")
def vocoders(gold):
    return {name: _vocoder(golden_config(gold, name)) for name in NAMES}


def _err(wav, ref):
    e = wav.detach().cpu().double() - ref.double()
    return float(e.pow(2).mean().sqrt()), float(e.abs().max())


@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference_golden(gold, vocoders, name):
    wav = vocoders[name](torch.from_numpy(gold[f"{name}_mel"]).cuda())
    assert wav.shape == (3, 1, 24 * 256)
    rms, linf = _err(wav, torch.from_numpy(gold[f"{name}_wav"]))
    assert rms <= WAV_RMS and linf <= WAV_LINF, (rms, linf)


_REF = {}


def _ragged(name, h, B, T):
    """mel (B, 80, T) with ragged lengths, padded with mel_mean, and its fp64 restated waveform (cached over the settings)."""
    key = (name, B, T)
    if key not in _REF:
        g = torch.Generator().manual_seed(B * 1000 + T)
        mel = torch.full((B, 80, T), W.MEL_MEAN_EMOJI)
        for b in range(B):
            n = max(1, T - 7 * b)
            mel[b, :, :n] = torch.randn(80, n, generator=g) * 2.0 - 5.0
        _REF[key] = (mel, restate(W.synthetic_hifigan_state(h), mel, h))
    return _REF[key]


@pytest.mark.parametrize("setting", [16, 6, 0])
@pytest.mark.parametrize("B,T", [(1, 1), (1, 17), (3, 45), (2, 100), (1, 600)])
@pytest.mark.parametrize("name", ["v3", "offstd", "v2"])
def test_ragged_shapes_against_the_fp64_restatement(gold, vocoders, name, B, T, setting):
    voc = vocoders[name]
    mel, ref = _ragged(name, golden_config(gold, name), B, T)
    voc._sync_engine()
    voc.engine.set_arithmetic(setting)
    try:
        wav = voc(mel.cuda())
        torch.cuda.synchronize()
    finally:
        voc.engine.set_arithmetic(16)
    assert wav.shape == (B, 1, 256 * T)
    bad = []
    check(f"{name} ragged {B}x{T} s{setting}", "std", wav, [(r, 0, T) for r in range(B)], list(ref[:, 0]), bad, label="VCERR")
    assert not bad, bad                                    # per row: RMS <= 5e-6, L-inf <= 5e-5 (vocoder_ref.GATE)


@pytest.mark.parametrize("setting", [16, 6, 0])
@pytest.mark.parametrize("B,T", [(1, 17), (3, 45)])
@pytest.mark.parametrize("name", list(WIDE_LAST))
def test_wide_last_level_against_the_fp64_restatement(name, B, T, setting):
    h = WIDE_LAST[name]
    key = ("wide", name)
    if key not in _REF:
        _REF[key] = _vocoder(h)
    voc = _REF[key]
    mel, ref = _ragged(name, h, B, T)
    voc._sync_engine()
    voc.engine.set_arithmetic(setting)
    try:
        wav = voc(mel.cuda())
        torch.cuda.synchronize()
    finally:
        voc.engine.set_arithmetic(16)
    assert wav.shape == (B, 1, 256 * T)
    bad = []
    check(f"{name} ragged {B}x{T} s{setting}", "std", wav, [(r, 0, T) for r in range(B)], list(ref[:, 0]), bad, label="VCERR")
    assert not bad, bad                                    # per row: RMS <= 5e-6, L-inf <= 5e-5 (vocoder_ref.GATE)


@pytest.mark.parametrize("B,T", [(2, 100), (1, 600), (8, 64)])
def test_fused_resblock2_matches_the_conv_launches(vocoders, B, T):
    voc = vocoders["v3"]
    mel = torch.randn(B, 80, T, generator=torch.Generator().manual_seed(T)) * 2.0 - 5.0
    voc._sync_engine()
    eng = voc.engine
    eng.set_chain(True)
    fused = voc(mel.cuda()).cpu()
    assert eng.last_cfg() == 207, eng.last_cfg()          # the last ResBlock (k = 7, d = 3 / 12, 32 channels) ran as one resblock2_h16_kernel
    eng.set_chain(False)
    try:
        unfused = voc(mel.cuda()).cpu()
        assert eng.last_cfg() != 207
    finally:
        eng.set_chain(True)
    assert float((fused.double() - unfused.double()).pow(2).mean().sqrt()) <= 1e-5


def test_fused_resblock2_saves_launches(vocoders):
    voc = vocoders["v3"]
    voc._sync_engine()
    eng = voc.engine
    mel = torch.randn(1, 80, 64, generator=torch.Generator().manual_seed(5)).cuda()
    counts = {}
    for on in (True, False):
        eng.set_chain(on)
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        voc(mel)
        torch.cuda.synchronize()
        counts[on] = eng.profile_read(reset=True)[2]
        eng.profile_enable(False)
    eng.set_chain(True)
    assert counts[True] < counts[False], counts


def test_denoiser_on_a_v3_generator(vocoders):
    from emojivoice_amd.denoiser import Denoiser

    voc = vocoders["v3"]
    den = Denoiser(voc, mode="zeros")
    sd = W.synthetic_hifigan_state(v3)
    bias_audio = restate(sd, torch.zeros(1, 80, 88), v3).float().squeeze(0)
    spec = torch.stft(bias_audio, n_fft=1024, hop_length=256, win_length=1024, window=torch.hann_window(1024), return_complex=True)
    bias = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1))[:, :, 0][:, :, None]
    assert float((den.bias_spec.cpu() - bias).abs().max()) <= 1e-3 * max(1.0, float(bias.abs().max()))
    mel = torch.randn(2, 80, 40, generator=torch.Generator().manual_seed(3)) * 2.0 - 5.0
    audio = voc(mel.cuda()).clamp(-1, 1).squeeze(1)
    got = den(audio, strength=0.01).cpu()
    ref = O.denoiser(audio.cpu(), bias, strength=0.01)
    assert float((got - ref).abs().max()) <= 1e-3


def test_reserve_then_no_allocation_on_v3():
    voc = _vocoder(v3)
    voc.warmup(max_frames=300, batch=4)
    eng = voc.engine
    n0 = eng.alloc_count()
    for B, T in ((4, 300), (2, 120), (1, 7), (3, 299)):
        voc(torch.randn(B, 80, T).cuda())
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0


def test_chunked_batch_equals_smaller_pieces():
    voc = _vocoder(v3)
    voc._sync_engine()
    eng = voc.engine
    T = 4000
    bmax = (2**32 - 2**20) // ((T + 2 * eng.voc_pad0) * eng.voc_frame_bytes)
    B = bmax + 1                                           # one more utterance than a chunk holds: two ev_hifigan calls
    mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(9)) * 2.0 - 5.0).cuda()
    whole = voc(mel).cpu()
    pieces = torch.cat([voc(mel[b0:b0 + 8]).cpu() for b0 in range(0, B, 8)])
    del mel
    torch.cuda.empty_cache()
    assert whole.shape == (B, 1, 256 * T)
    # (other batch sizes tile the flattened time axis differently, hence other fp16 tile scales: equal to rounding)
    assert float((whole.double() - pieces.double()).pow(2).mean().sqrt()) <= 1e-5


def test_v1_and_v3_in_one_process():
    mel = torch.randn(2, 80, 50, generator=torch.Generator().manual_seed(11)) * 2.0 - 5.0
    g1 = _vocoder(v1)
    alone = g1(mel.cuda()).cpu()
    g3 = _vocoder(v3)
    w3 = g3(mel.cuda()).cpu()
    again = g1(mel.cuda()).cpu()
    assert torch.equal(alone, again)
    rms1, _ = _err(again, O.hifigan_forward(W.synthetic_hifigan_state(), mel, W.HIFIGAN_V1))
    rms3, linf3 = _err(w3, restate(W.synthetic_hifigan_state(v3), mel, v3))
    assert rms1 <= WAV_RMS and rms3 <= WAV_RMS and linf3 <= WAV_LINF, (rms1, rms3, linf3)


def test_cli_synthesises_with_v3(tmp_path):
    r = subprocess.run([sys.executable, "-m", "emojivoice_amd.cli", "--synthetic", "--vocoder_config", "v3", "--ids", "0 23 0 51 0 17 0",
                        "--spk", "12", "--steps", "4", "--output_folder", str(tmp_path)], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    wavs = list(tmp_path.glob("*.wav"))
    assert len(wavs) == 1
    T = np.load(wavs[0].with_suffix(".npy")).shape[-1]                      # the decoded mel the CLI saves next to the WAV: (80, T)
    data = wavs[0].read_bytes()
    n = int.from_bytes(data[40:44], "little") // 3                       # PCM_24 mono: 3 bytes a sample
    assert T > 0 and n == 256 * T, (n, T)
