"""Path-level parity on a real MI355X: HIP path (through the C ABI) vs the CPU oracle on the
same seeded inputs, and vs the committed reference-generated golden vectors.

Gates (BASELINE.json north_star): mel L-inf <= 1e-4 (evaluated on the denormalised ``mel``),
waveform RMS error <= 1e-3 on Generator.forward output.
"""
import numpy as np
import pytest
import torch

from emojivoice_amd import weights as W
from oracle import matcha_oracle as O

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
MEL_GATE = 1e-4
WAV_RMS_GATE = 1e-3


def _linf(a, b):
    return float((a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max())


@pytest.fixture(scope="module")
def model(matcha_sd):
    from emojivoice_amd.matcha_tts import MatchaTTS

    return MatchaTTS(matcha_sd, device="cuda:0")


@pytest.fixture(scope="module")
def vocoder(voc_sd):
    from emojivoice_amd.hifigan import AttrDict, Generator, v1

    g = Generator(AttrDict(v1)).to("cuda:0")
    g.load_state_dict(W.weight_norm_split(voc_sd))   # raw weight_g / weight_v checkpoint form
    g.eval()
    g.remove_weight_norm()
    return g


def test_native_library_is_loaded():
    from emojivoice_amd import _lib

    lib = _lib.load_library()
    assert lib.ev_abi_version() == 4
    with open("/proc/self/maps") as f:
        assert "libemojivoice_hip.so" in f.read()


def test_estimator_vs_golden(golden, model):
    lengths = T_(golden["g1_lengths"])
    spk = model._sd["spk_emb.weight"][T_(golden["g1_spk_ids"]).cuda()]
    for i, tv in enumerate(golden["g1_t"]):
        v = model.engine.estimator(T_(golden["g1_x"]).cuda(), T_(golden["g1_mu"]).cuda(), lengths.cuda(), spk, float(tv))
        assert _linf(v, golden[f"g1_v_t{i}"]) <= 5e-5, i


def test_cfm_vs_golden(golden, model):
    lengths = T_(golden["g1_lengths"])
    spk = model._sd["spk_emb.weight"][T_(golden["g1_spk_ids"]).cuda()]
    for n in (2, 4, 10):
        dec, mel = model.decode(T_(golden["g1_mu"]).cuda(), lengths.cuda(), n, 0.667, spk, z=T_(golden["g2_z"]).cuda())
        assert _linf(dec, golden[f"g2_dec_n{n}"]) <= MEL_GATE / 2, n
    spk1 = model._sd["spk_emb.weight"][torch.tensor([58]).cuda()]
    dec, _ = model.decode(T_(golden["g2b_mu"]).cuda(), torch.tensor([24]).cuda(), 10, 0.667, spk1, z=T_(golden["g2b_z"]).cuda())
    assert _linf(dec, golden["g2b_dec_n10"]) <= MEL_GATE / 2


def test_synthesise_vs_golden(golden, model):
    for tag, ls in (("a", 1.0), ("b", 0.8)):
        r = model.synthesise(T_(golden["g3_ids"]).cuda(), T_(golden["g3_x_lengths"]).cuda(), n_timesteps=10, temperature=0.667,
                             spks=T_(golden["g3_spks"]).cuda(), length_scale=ls, z=T_(golden[f"g3{tag}_z"]).cuda())
        assert set(r) == {"encoder_outputs", "decoder_outputs", "attn", "mel", "mel_lengths", "rtf"}
        assert np.array_equal(r["mel_lengths"].cpu().numpy(), golden[f"g3{tag}_mel_lengths"])
        assert tuple(r["attn"].shape) == tuple(golden[f"g3{tag}_attn_shape"])
        assert _linf(r["mel"], golden[f"g3{tag}_mel"]) <= MEL_GATE
        # seed parity: the default draw reproduces the reference CPU run's noise for the same torch.manual_seed
        torch.manual_seed(777)
        r2 = model.synthesise(T_(golden["g3_ids"]).cuda(), T_(golden["g3_x_lengths"]).cuda(), n_timesteps=10, temperature=0.667,
                              spks=T_(golden["g3_spks"]).cuda(), length_scale=ls)
        assert _linf(r2["mel"], golden[f"g3{tag}_mel"]) <= MEL_GATE


def test_hifigan_vs_golden(golden, vocoder):
    wav = vocoder(T_(golden["g4_mel"]).cuda())
    assert wav.shape == (2, 1, 32 * 256)
    err = wav.cpu().numpy().astype(np.float64) - golden["g4_wav"]
    assert float(np.sqrt(np.mean(err**2))) <= WAV_RMS_GATE / 10
    assert float(np.abs(err).max()) <= 1e-3


@pytest.mark.parametrize("B,Tp,lens", [(3, 64, [64, 50, 9]), (2, 132, [132, 131]), (5, 260, [260, 13, 200, 77, 259])])
def test_cfm_vs_oracle_ragged(model, matcha_sd, B, Tp, lens):
    g = torch.Generator().manual_seed(Tp)
    mu = torch.randn(B, 80, Tp, generator=g)
    z = torch.randn(B, 80, Tp, generator=g)
    lengths = torch.tensor(lens)
    mask = O.sequence_mask(lengths, Tp).unsqueeze(1).float()
    ids = torch.tensor([107, 58, 79, 103, 66][:B])
    spk = matcha_sd["spk_emb.weight"][ids]
    ref = O.cfm_decode(matcha_sd, mu * mask, mask, 10, 0.667, spk, z=z)
    dec, mel = model.decode((mu * mask).cuda(), lengths.cuda(), 10, 0.667, spk.cuda(), z=z.cuda())
    ref_mel = O.denormalize(ref, matcha_sd["mel_mean"], matcha_sd["mel_std"])
    assert _linf(mel, ref_mel) <= MEL_GATE


@pytest.mark.parametrize("B,T", [(1, 17), (2, 100), (3, 45)])
def test_hifigan_vs_oracle(vocoder, voc_sd, B, T):
    g = torch.Generator().manual_seed(T)
    mel = torch.randn(B, 80, T, generator=g) * 2.0 - 5.0
    ref = O.hifigan_forward(voc_sd, mel, W.HIFIGAN_V1)
    wav = vocoder(mel.cuda())
    assert wav.shape == ref.shape == (B, 1, 256 * T)
    err = (wav.cpu().double() - ref.double())
    assert float(err.pow(2).mean().sqrt()) <= WAV_RMS_GATE / 10
    assert float(ref.pow(2).mean().sqrt()) > 0.05


@pytest.mark.parametrize("B,T", [(2, 777), (1, 1500)])
def test_hifigan_arithmetic_switch(vocoder, B, T):
    """The vocoder on one handle with its products on the bf16 pipe (default: fused split pairs at every level, split convs where the grid is
    deep enough) and on the fp32 MFMA (ev_set_arithmetic 0): odd lengths, ragged last tiles; the two agree far inside the waveform gate."""
    g = torch.Generator().manual_seed(T + B)
    mel = (torch.randn(B, 80, T, generator=g) * 2.0 - 5.0).cuda()
    orig = vocoder.engine.arithmetic()
    vocoder.engine.set_arithmetic(6)
    w6 = vocoder(mel)
    assert torch.equal(vocoder(mel), w6)
    try:
        vocoder.engine.set_arithmetic(0)
        w0 = vocoder(mel)
        vocoder.engine.set_arithmetic(3)                   # the opt-in fast setting: three products per fp32 product (~16 significand bits)
        w3 = vocoder(mel)
        vocoder.engine.set_arithmetic(16)                  # two block-scaled fp16 pieces, three products: fp32-grade like 6
        w16 = vocoder(mel)
        assert torch.equal(vocoder(mel), w16)
    finally:
        vocoder.engine.set_arithmetic(orig)
    assert float((w16 - w0).abs().max()) <= 5e-5 and float((w16 - w0).pow(2).mean().sqrt()) <= WAV_RMS_GATE / 100
    assert float(w0.abs().max()) > 1e-3
    assert float((w6 - w0).abs().max()) <= 5e-5 and float((w6 - w0).pow(2).mean().sqrt()) <= WAV_RMS_GATE / 100
    # not the default and not what bench.py times: inside the waveform gate with a margin of ~10, two orders above the default's error
    assert float((w3 - w0).pow(2).mean().sqrt()) <= WAV_RMS_GATE / 5


def test_config2_shape_properties(model, vocoder):
    """Full-size (B=8 slice of config 2: T=516) size-independent checks: batch-row independence when nothing is
    padded (all lengths = Tp: no cross-utterance coupling left) and wav_len == 256 * mel_len (cli.py:310)."""
    B, Tp = 8, 516
    g = torch.Generator().manual_seed(1234)
    mu = torch.randn(B, 80, Tp, generator=g).cuda()
    z = torch.randn(B, 80, Tp, generator=g).cuda()
    lengths = torch.full((B,), Tp).cuda()
    spk = model._sd["spk_emb.weight"][torch.tensor([107, 58, 79, 103, 66, 18, 12, 15]).cuda()]
    dec, mel = model.decode(mu, lengths, 10, 0.667, spk, z=z)
    dec1, mel1 = model.decode(mu[2:3], lengths[2:3], 10, 0.667, spk[2:3], z=z[2:3])
    assert _linf(mel[2:3], mel1.cpu()) <= 1e-5
    wav = vocoder(mel)
    assert wav.shape == (B, 1, 256 * Tp)
    wav1 = vocoder(mel[2:3])
    assert _linf(wav[2:3], wav1.cpu()) <= 5e-5     # the batch-1 call takes the split-K build for its small launches: other k-chunk summation order
    assert torch.isfinite(wav).all()


def test_fails_loudly_without_gpu_path():
    from emojivoice_amd._lib import EvLibraryError
    from emojivoice_amd.hifigan import AttrDict, Generator, v1

    with pytest.raises(EvLibraryError):
        Generator(AttrDict(v1)).to("cpu")


def test_denoiser_vs_golden(golden, vocoder):
    """device-side Denoiser (bias spectrum from the HIP vocoder on a zero mel) vs the reference's."""
    from emojivoice_amd.denoiser import Denoiser

    den = Denoiser(vocoder, mode="zeros")
    ref_bias = golden["g7_bias_spec"]
    assert _linf(den.bias_spec, ref_bias) <= 1e-3 * max(1.0, float(np.abs(ref_bias).max()))
    audio = T_(golden["g4_wav"]).clamp(-1, 1).squeeze().cuda()
    d = den(audio, strength=0.00025)
    assert tuple(d.shape) == golden["g7_denoised"].shape        # length stays 256*T, (B, L)
    assert _linf(d, golden["g7_denoised"]) <= 1e-4
    assert tuple(den(audio[0], strength=0.00025).shape) == (1, audio.shape[-1])     # 1-D input comes back as a batch of one (bias broadcast)


def test_cli_writes_pcm24_wav(tmp_path):
    """Config 1 plumbing: ids + an unmapped emoji (-> speaker 0) -> 22.05 kHz PCM_24 wav, wav_len == 256 * mel_len."""
    import wave

    from emojivoice_amd import cli

    ids = " ".join(str(i) for i in [23, 51, 7, 99, 140, 31, 12, 64, 8, 77, 101, 5])
    cli.cli(["--synthetic", "--ids", ids, "--add_blank", "--emoji-text", "Hello world \U0001F60A", "--steps", "10",
             "--output_folder", str(tmp_path)])
    wavs = sorted(tmp_path.glob("*.wav"))
    assert len(wavs) == 1 and "speaker_000" in wavs[0].name
    mel = np.load(str(wavs[0])[:-4] + ".npy")
    with wave.open(str(wavs[0])) as w:
        assert (w.getframerate(), w.getsampwidth(), w.getnchannels()) == (22050, 3, 1)
        assert w.getnframes() == 256 * mel.shape[1]


@pytest.mark.parametrize("B,Tp,lens,steps", [(1, 4, [3], 2), (2, 8, [8, 1], 3), (1, 1032, [1030], 2), (7, 4, [4, 1, 3, 4, 2, 4, 3], 2)])
def test_cfm_edge_shapes(model, matcha_sd, B, Tp, lens, steps):
    """Smallest legal Tp (4), a 1-frame utterance beside a full one, a 12-s utterance (33 key tiles in attention), and a batch
    of utterances shorter than one epilogue pass (S < 8 rows: several wraps of the row bookkeeping)."""
    g = torch.Generator().manual_seed(Tp + 7)
    mu = torch.randn(B, 80, Tp, generator=g)
    z = torch.randn(B, 80, Tp, generator=g)
    lengths = torch.tensor(lens)
    mask = O.sequence_mask(lengths, Tp).unsqueeze(1).float()
    spk = matcha_sd["spk_emb.weight"][torch.tensor([17, 0, 5, 9, 33, 71, 108][:B])]
    ref = O.cfm_decode(matcha_sd, mu * mask, mask, steps, 1.0, spk, z=z)
    dec, _ = model.decode((mu * mask).cuda(), lengths.cuda(), steps, 1.0, spk.cuda(), z=z.cuda())
    assert _linf(dec, ref) <= MEL_GATE / 2


def test_hifigan_single_frame(vocoder, voc_sd):
    mel = torch.randn(1, 80, 1, generator=torch.Generator().manual_seed(3)) - 5.0
    ref = O.hifigan_forward(voc_sd, mel, W.HIFIGAN_V1)
    wav = vocoder(mel.cuda())
    assert wav.shape == (1, 1, 256)
    assert float((wav.cpu() - ref).pow(2).mean().sqrt()) <= WAV_RMS_GATE / 10


def test_argument_errors(model):
    from emojivoice_amd._lib import EvLibraryError

    mu = torch.zeros(1, 80, 6).cuda()       # Tp not a multiple of 4 (fix_len_compatibility violated)
    with pytest.raises(EvLibraryError):
        model.engine.cfm_decode(mu, torch.tensor([6]).cuda(), torch.zeros(1, 64).cuda(), mu, 2)
    mu = torch.zeros(1, 80, 8).cuda()
    with pytest.raises(EvLibraryError):
        model.engine.cfm_decode(mu, torch.tensor([8]).cuda(), torch.zeros(1, 64).cuda(), mu, 0)     # steps > 0 (cli.py:143)
    with pytest.raises(AttributeError):   # spks required when n_spks > 1, same failure mode as matcha_tts.py:118
        model.synthesise(torch.ones(1, 5, dtype=torch.long).cuda(), torch.tensor([5]).cuda(), 2, spks=None)


def test_single_speaker_model_vs_oracle():
    """n_spks = 1 (the LJSpeech-style checkpoint of synthesis.ipynb): no speaker embedding, estimator in_channels = 160."""
    from emojivoice_amd.matcha_tts import MatchaTTS

    sd = W.synthetic_matcha_state(178, 1)
    assert "spk_emb.weight" not in sd and sd["decoder.estimator.time_mlp.linear_1.weight"].shape[1] == 160
    m = MatchaTTS(sd, device="cuda:0")
    assert m.n_spks == 1
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1, 178, (2, 20), generator=g)
    xl = torch.tensor([20, 13])
    # same z for both paths: drawn at the padded length the host stage produces
    ref0 = O.text_encoder(sd, ids, xl, None)
    w = torch.ceil(torch.exp(ref0[1]) * ref0[2])
    tp = O.fix_len_compatibility(int(torch.clamp_min(w.sum([1, 2]), 1).max()))
    z = torch.randn(2, 80, tp, generator=g)
    ref = O.synthesise(sd, ids, xl, 4, 0.667, None, 1.0, z=z)
    got = m.synthesise(ids.cuda(), xl.cuda(), 4, 0.667, None, 1.0, z=z.cuda())
    # integer output: exact (how often device and host rounding can disagree on a ceil() is measured by
    # tests/test_gpu_configs.py::test_device_encoder_duration_flips)
    assert np.array_equal(got["mel_lengths"].cpu().numpy(), ref["mel_lengths"].numpy())
    assert _linf(got["mel"], ref["mel"]) <= MEL_GATE


def test_vocoder_batch_chunking_matches(vocoder):
    """Batches beyond the 4 GiB-per-tensor buffer-addressing limit are split by rows: the result must not depend on
    where the split falls (the vocoder has no cross-utterance coupling)."""
    g = torch.Generator().manual_seed(21)
    mel = (torch.randn(5, 80, 24, generator=g) * 2 - 5).cuda()
    full = vocoder(mel)
    parts = torch.cat([vocoder(mel[:2]), vocoder(mel[2:])], dim=0)
    assert _linf(full, parts.cpu()) <= 5e-5      # tiny chunks take the split-K build for some layers: other k-chunk summation order


def test_batch_pipeline_is_bit_identical(model, vocoder):
    """Two-stream software pipeline over consecutive batches (emojivoice_amd/pipeline.py): same results as the two stages
    called back to back, for every batch in flight."""
    from emojivoice_amd.pipeline import BatchPipeline

    g = torch.Generator().manual_seed(33)
    B, Tp = 3, 36
    spk = model._sd["spk_emb.weight"][torch.tensor([2, 4, 6]).cuda()]
    lengths = torch.tensor([36, 20, 29], dtype=torch.int32).cuda()
    batches = [(torch.randn(B, 80, Tp, generator=g).cuda(), (torch.randn(B, 80, Tp, generator=g) * 0.667).cuda()) for _ in range(4)]
    ref = []
    for mu, z in batches:
        mel = model.engine.cfm_decode(mu, lengths, spk, z, 3, model.mel_std, model.mel_mean)
        ref.append(vocoder(mel).cpu())
    pipe = BatchPipeline(model, vocoder)
    outs = [pipe.submit(mu, lengths, spk, z, 3) for mu, z in batches]
    pipe.synchronize()
    for r, o in zip(ref, outs):
        assert torch.equal(r, o.cpu())


def test_two_pipelines_in_flight_are_bit_identical(model, vocoder, matcha_sd, voc_sd):
    """PipelineGroup: two batch pipelines (two engine pairs, four streams), batches alternating — what bench.py times."""
    from emojivoice_amd.hifigan import AttrDict, Generator, v1
    from emojivoice_amd.matcha_tts import MatchaTTS
    from emojivoice_amd.pipeline import PipelineGroup

    model2 = MatchaTTS(matcha_sd, device=model.device)
    voc2 = Generator(AttrDict(v1)).to(model.device)      # built exactly as the `vocoder` fixture is (weight-norm form, folded)
    voc2.load_state_dict(W.weight_norm_split(voc_sd))
    voc2.eval()
    voc2.remove_weight_norm()
    g = torch.Generator().manual_seed(34)
    B, Tp = 2, 44
    spk = model._sd["spk_emb.weight"][torch.tensor([3, 8]).cuda()]
    lengths = torch.tensor([44, 30], dtype=torch.int32).cuda()
    batches = [(torch.randn(B, 80, Tp, generator=g).cuda(), (torch.randn(B, 80, Tp, generator=g) * 0.667).cuda()) for _ in range(5)]
    ref = []
    for mu, z in batches:
        mel = model.engine.cfm_decode(mu, lengths, spk, z, 2, model.mel_std, model.mel_mean)
        ref.append(vocoder(mel).cpu())
    group = PipelineGroup([(model, vocoder), (model2, voc2)])
    outs = [group.submit(mu, lengths, spk, z, 2) for mu, z in batches]
    group.synchronize()
    for r, o in zip(ref, outs):
        assert torch.equal(r, o.cpu())
    model2.engine.close()
    voc2.engine.close()


def test_device_text_encoder_vs_golden_and_host(golden, model, matcha_sd):
    """ev_text_encoder (HIP kernels through the C ABI) vs the reference-generated golden text-encoder outputs, vs the CPU
    oracle on a ragged batch, and vs the plain-torch host stage."""
    ids = T_(golden["g3_ids"]).long()
    lens = T_(golden["g3_x_lengths"])
    spk = model._sd["spk_emb.weight"][T_(golden["g3_spks"]).long().cuda()]
    mu, logw = model.engine.text_encoder(ids.cuda(), lens.cuda(), spk)
    assert _linf(mu, golden["g3_mu_x"]) <= 1e-4
    assert _linf(logw, golden["g3_logw"]) <= 1e-4
    # ragged batch incl. a length-1 utterance, vs the oracle
    g = torch.Generator().manual_seed(5)
    ids2 = torch.randint(1, 178, (4, 37), generator=g)
    lens2 = torch.tensor([37, 1, 20, 9])
    sid = torch.tensor([0, 3, 7, 10])
    spk2 = model._sd["spk_emb.weight"][sid.cuda()]
    mu2, logw2 = model.engine.text_encoder(ids2.cuda(), lens2.cuda(), spk2)
    rmu, rlogw, _ = O.text_encoder(matcha_sd, ids2, lens2, torch.nn.functional.embedding(sid, matcha_sd["spk_emb.weight"]))
    assert _linf(mu2, rmu) <= 1e-4 and _linf(logw2, rlogw) <= 1e-4
    hmu, hlogw, _ = model.encoder(ids2.cuda(), lens2.cuda(), spk2)
    assert _linf(mu2, hmu.cpu()) <= 1e-4 and _linf(logw2, hlogw.cpu()) <= 1e-4


def test_denoiser_vs_oracle_batched(vocoder):
    """ev_denoise / ev_stft_magnitude (DFT-basis convolutions) vs torch.stft / torch.istft on a ragged-content batch, including the
    shortest supported length (4 hops) and the magnitude spectrum itself: every row against the fp64 yardstick at the per-row gates
    of tests/denoiser_ref.py (set from the float32 restatement, tests/test_denoiser_reference.py; tests/test_gpu_denoiser.py has the
    conv builds beyond this one)."""
    import denoiser_ref as D

    vocoder._sync_engine()
    eng = vocoder.engine
    g = torch.Generator().manual_seed(77)
    for B, L in ((3, 256 * 21), (1, 1024)):
        audio = (torch.randn(B, L, generator=g) * 0.3).clamp(-1, 1)
        bias = torch.rand(513, generator=g) * 2.0
        ref_mag, ref = D.yardstick(audio, bias, 0.01)
        assert tuple(ref.shape) == tuple(O.denoiser(audio, bias[None, :, None], strength=0.01).shape)
        mag = eng.stft_magnitude(audio.cuda())
        assert tuple(mag.shape) == tuple(ref_mag.shape)
        got = eng.denoise(audio.cuda(), bias.cuda(), 0.01)
        rms, mx, mg = D.row_errors((mag, got), (ref_mag, ref), audio)
        assert bool((rms <= D.GATE_RMS).all()) and bool((mx <= D.GATE_MAX).all()) and bool((mg <= D.GATE_MAG).all()), (B, L, rms, mx, mg)


def test_text_encoder_short_utterances(model, matcha_sd):
    """Utterances shorter than one epilogue pass (S = Tx + 4 < 8 rows): several wraps of the row bookkeeping per pass."""
    g = torch.Generator().manual_seed(9)
    for B, Tx in ((6, 3), (10, 3), (9, 1), (5, 2)):
        ids = torch.randint(0, 178, (B, Tx), generator=g)
        lens = torch.randint(1, Tx + 1, (B,), generator=g)
        sid = torch.randint(0, 109, (B,), generator=g)
        spk = torch.nn.functional.embedding(sid, matcha_sd["spk_emb.weight"])
        mu, logw = model.engine.text_encoder(ids.cuda(), lens.cuda(), spk.cuda())
        rmu, rlogw, _ = O.text_encoder(matcha_sd, ids, lens, spk)
        assert _linf(mu, rmu) <= 1e-4 and _linf(logw, rlogw) <= 1e-4, (B, Tx)


def test_warmup_calls(model, vocoder):
    model.warmup()
    vocoder.warmup()


def test_align_vs_oracle(model):
    """ev_align (generate_path + mu_y = attn^T mu_x) vs the oracle's generate_path / matmul, integer and fractional
    length scales, ragged token lengths, incl. an all-zero-duration utterance (y_length clamps to 1)."""
    g = torch.Generator().manual_seed(13)
    for scale in (1.0, 0.8, 1.37):
        B, Tx = 5, 23
        xl = torch.tensor([23, 1, 17, 9, 23])
        x_mask = O.sequence_mask(xl, Tx).unsqueeze(1).float()
        logw = torch.randn(B, 1, Tx, generator=g) * 0.7 + 0.3
        logw[3] = -30.0                                            # exp -> 0: ceil(0) = 0 for every token
        w_ceil = torch.ceil(torch.exp(logw) * x_mask) * scale
        yl = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
        Tp = O.fix_len_compatibility(int(yl.max()))
        y_mask = O.sequence_mask(yl, Tp).unsqueeze(1).float()
        ref_attn = O.generate_path(w_ceil.squeeze(1), (x_mask.unsqueeze(-1) * y_mask.unsqueeze(2)).squeeze(1))
        mu_x = torch.randn(B, 80, Tx, generator=g)
        ref_mu_y = torch.matmul(ref_attn.transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
        mu_y, attn = model.engine.align(w_ceil.cuda(), mu_x.cuda(), xl.cuda(), yl.cuda(), Tp)
        assert torch.equal(attn.squeeze(1).cpu(), ref_attn), scale
        assert torch.equal(mu_y.cpu(), ref_mu_y), scale
