"""HiFi-GAN V1 on the MI355X against the fp64 restatement (tests/vocoder_ref.py), row by row, at gates set from measured error.

Four cases, each under arithmetic settings 16 / 6 / 0 and with two checkpoints: the standard synthetic weights (what bench.py runs) and
the linear-regime weights (conv_post x 0.05), whose output tanh does not shrink upstream errors.

  bench     B = 64 x T = 516, the mel bench.py decodes, every row (head, tail and a rotating interior window), and a ragged batch of the
            same size: B * T > 16384, the single-stream plan bench.py times (plus set_chain / set_amax off)
  streams   B = 32 at T = 512 (B * T = 16384: three MRF streams, balancing off) and T = 513 (one stream); one small shape on three
            streams and with the fan-out switched off, where a balanced build does run
  small     full rows at T in {1 .. 300} x B in {1, 2, 3} (partial tiles at every level; B = 1, T = 300 is where the upsamplers' amax
            granules used to run past their slots) and a ragged B = 5 batch
  2 GiB     B = 2 x T = 66000: tensors of 2.16 GB per utterance, one row per ev_hifigan call, windows across the 2^31 byte offset

The fp64 references run through torch on the GPU (one window per case is also run on the CPU and must agree to 1e-10) and are cached
across settings.  Gates, per row over the compared samples: standard weights RMS <= 5e-6, L-inf <= 5e-5; linear-regime weights RMS <= 5e-6
and L-inf <= 3e-5 of that row's fp64 RMS.  The worst values measured on an MI355X over every case and setting were 1.5e-6 / 1.5e-5 and
1.4e-6 / 7.9e-6 (relative): each gate is 3.4-3.8x its worst value (the case tables print with -s).

Which path a call takes: B * T <= mrf_max_frames (16384) fans the three ResBlock1 chains of a level out to three streams and turns the
balanced persistent builds off; a larger call stays on one stream with balancing allowed.  The fan-out plan carries six more scratch
tensors a level, so workspace_bytes tells the two plans apart; the balanced-launch epoch (Engine.sk_stats) shows balancing switching off.
At B = 64 x 516 and B = 32 x 513 every vocoder conv grid is too deep for the balanced builds (bal_ok / split_bal_ok in ev_engine.hip),
so no vocoder launch takes one there (the epoch stays put, measured): the single-stream plan is what those shapes exercise.
"""
import time

import pytest
import torch

import bench
from emojivoice_amd import weights as W
from emojivoice_amd.hifigan import AttrDict, Generator, v1
from vocoder_ref import MARGIN, WEIGHTS, gpu_refs, linear_regime_state   # (the gates, GATE and REF_FLOOR, live there too)
from vocoder_ref import check as _check, fanout_planned as _fanout_planned, row_windows as _row_windows, run as _run, sweep as _sweep

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CLOCK = {"gpu_ref": 0.0, "cpu_ref": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report_clock():
    t0 = time.perf_counter()
    yield
    print(f"\nV1CLOCK wall {time.perf_counter() - t0:.1f} s  fp64 reference on the GPU {_CLOCK['gpu_ref']:.1f} s  "
          f"on the CPU {_CLOCK['cpu_ref']:.1f} s ({torch.get_num_threads()} threads)")


@pytest.fixture(scope="module")
def sds():
    return {"std": W.synthetic_hifigan_state(), "lin": linear_regime_state()}


@pytest.fixture(scope="module")
def vocs(sds):
    out = {}
    for name, sd in sds.items():
        g = Generator(AttrDict(v1)).to(DEV)
        g.load_state_dict(sd)
        g._sync_engine()
        out[name] = g
    return out


def _refs(sds, mel, wins, check_cpu=1):
    """{weights: [fp64 samples of each window]}; the first ``check_cpu`` windows are also run on the CPU and must agree to 1e-10."""
    return gpu_refs(sds, mel, v1, wins, _CLOCK, check_cpu=check_cpu, margin=MARGIN, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# the bench batch: B = 64 x 516, every row
# ---------------------------------------------------------------------------------------------------------------------
B64, T64 = 64, 516


@pytest.fixture(scope="module")
def bench_mel():
    """The mel bench.py's batch decodes to (10 Euler steps, temperature 0.667), as in test_gpu_configs.test_config2."""
    from emojivoice_amd.matcha_tts import MatchaTTS

    model = MatchaTTS(W.synthetic_matcha_state(), device=DEV)
    mu, z, spk_ids, lengths = bench.make_inputs(B64, T64, 0, B64, torch.device(DEV))
    spk = model._sd["spk_emb.weight"][spk_ids]
    mel = model.engine.cfm_decode(mu, lengths, spk, z * 0.667, 10, model.mel_std, model.mel_mean)
    torch.cuda.synchronize()
    mean = float(model.mel_mean)
    del model
    return mel, mean


def test_bench_batch_every_row(vocs, sds, bench_mel):
    mel, _ = bench_mel
    wins = _row_windows([T64] * B64)
    refs = _refs(sds, mel, wins)
    bad = []
    epochs = _sweep("bench 64x516", vocs, mel, wins, refs, bad)
    for w in WEIGHTS:
        wav, _ = _run(vocs[w], mel, 16, chain=False)
        _check("bench 64x516 s16 chain off", w, wav, wins, refs[w], bad)
        wav, _ = _run(vocs[w], mel, 16, amax=False)
        _check("bench 64x516 s16 amax off", w, wav, wins, refs[w], bad)
    print(f"V1PATH bench 64x516 balanced launches per call {epochs}")
    assert not bad, bad
    assert not _fanout_planned(vocs["std"].engine, B64, T64)   # one stream: the plan bench.py times


def test_bench_batch_ragged(vocs, sds, bench_mel):
    mel, mean = bench_mel
    lengths = [T64 - (37 * r) % 300 for r in range(B64)]
    mel = mel.clone()
    for r, L in enumerate(lengths):
        mel[r, :, L:] = mean                             # the decoder's padding: mel_mean past each length
    wins = _row_windows(lengths)
    refs = _refs(sds, mel, wins)
    bad = []
    epochs = _sweep("bench 64x516 ragged", vocs, mel, wins, refs, bad, settings=(16, 6, 0))
    print(f"V1PATH bench ragged balanced launches per call {epochs}")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# both sides of the three-stream threshold (B * T <= 16384)
# ---------------------------------------------------------------------------------------------------------------------
def test_both_sides_of_the_stream_threshold(vocs, sds):
    B, rows = 32, [0, 1, 6, 11, 17, 22, 30, 31]
    mel513 = torch.randn(B, 80, 513, generator=torch.Generator().manual_seed(513)).to(DEV) * 2.0 - 5.0
    mel512 = mel513[..., :512].contiguous()
    shared = [(r, 0, 8) for r in rows] + [(r, 16 + (61 * r) % 470, 24 + (61 * r) % 470) for r in rows]   # (ends <= 510: same fp64 on both)
    ref_shared = _refs(sds, mel513, shared)
    tails = {T: [(r, T - 8, T) for r in rows] for T in (512, 513)}
    ref_tail = {T: _refs(sds, m, tails[T], check_cpu=0) for T, m in ((512, mel512), (513, mel513))}
    bad, epochs = [], {}
    for T, m in ((512, mel512), (513, mel513)):
        wins = shared + tails[T]
        refs = {w: ref_shared[w] + ref_tail[T][w] for w in WEIGHTS}
        epochs[T] = _sweep(f"streams 32x{T}", vocs, m, wins, refs, bad)
    # one small shape with the fan-out switched off: the three chains on the caller's stream
    mel = torch.randn(4, 80, 100, generator=torch.Generator().manual_seed(100)).to(DEV) * 2.0 - 5.0
    wins = [(r, 0, 100) for r in range(4)]
    refs = _refs(sds, mel, wins)
    epochs["4x100 three streams"] = _sweep("streams 4x100", vocs, mel, wins, refs, bad)
    saved = {w: vocs[w].engine.mrf_streams_max for w in WEIGHTS}
    try:
        for w in WEIGHTS:
            vocs[w].engine.set_mrf_streams_max(0)
        epochs["4x100 one stream"] = _sweep("streams 4x100 fan-out off", vocs, mel, wins, refs, bad)
    finally:
        for w in WEIGHTS:
            vocs[w].engine.set_mrf_streams_max(saved[w])
    eng = vocs["std"].engine
    plans = {T: _fanout_planned(eng, B, T) for T in (512, 513)}
    print(f"V1PATH streams balanced launches per call {epochs}  fan-out planned {plans}")
    assert not bad, bad
    assert plans == {512: True, 513: False}, plans      # T = 512: three streams; T = 513: one
    # the fan-out turns balancing off: at 4 x 100 a balanced build runs only once the fan-out is switched off
    assert epochs["4x100 three streams"][16] == 0 and epochs["4x100 one stream"][16] > 0, epochs


# ---------------------------------------------------------------------------------------------------------------------
# odd and small shapes, full rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 7, 31, 33, 63, 65, 127, 129, 255, 257, 300])
def test_small_shapes_full_rows(vocs, sds, T):
    mel3 = torch.randn(3, 80, T, generator=torch.Generator().manual_seed(7000 + T)).to(DEV) * 2.0 - 5.0
    refs3 = _refs(sds, mel3, [(r, 0, T) for r in range(3)])   # rows do not interact: the B = 1 / 2 references are rows of B = 3
    bad = []
    for B in (1, 2, 3):
        _sweep(f"small {B}x{T}", vocs, mel3[:B].contiguous(), [(r, 0, T) for r in range(B)], {w: refs3[w][:B] for w in WEIGHTS}, bad)
    assert not bad, bad


def test_small_ragged_batch(vocs, sds):
    lengths = [300, 257, 129, 33, 1]
    mel = torch.full((5, 80, 300), W.MEL_MEAN_EMOJI)
    g = torch.Generator().manual_seed(55)
    for r, L in enumerate(lengths):
        mel[r, :, :L] = torch.randn(80, L, generator=g) * 2.0 - 5.0
    mel = mel.to(DEV)
    wins = [(r, 0, L) for r, L in enumerate(lengths)]
    refs = _refs(sds, mel, wins)
    bad = []
    _sweep("small ragged 5x300", vocs, mel, wins, refs, bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# past 2 GiB: one utterance per ev_hifigan call, byte offsets past 2^31
# ---------------------------------------------------------------------------------------------------------------------
T_BIG = 66000
CROSS = 65532          # pad frame 4 + 65532 = flattened frame 65536: 65536 x 32 KB = 2^31 bytes into the 32-KB-per-frame tensors


def test_past_2gib(vocs, sds):
    eng = vocs["std"].engine
    per_utt = (T_BIG + 2 * eng.voc_pad0) * eng.voc_frame_bytes
    assert 2**31 < per_utt < 2**32 - 2**20 < 2 * per_utt       # the widest tensor passes 2^31 bytes; two rows need two calls
    print(f"V1WS workspace_bytes(1, 0, {T_BIG}) = {eng.workspace_bytes(1, 0, T_BIG)}")
    mel = torch.randn(2, 80, T_BIG, generator=torch.Generator().manual_seed(66)).to(DEV) * 2.0 - 5.0
    wins = []
    for r in range(2):
        wins += [(r, CROSS - 4, CROSS + 4), (r, 0, 8), (r, T_BIG - 8, T_BIG)]
    refs = _refs(sds, mel, wins)
    bad = []
    _sweep(f"2GiB 2x{T_BIG}", vocs, mel, wins, refs, bad)
    assert not bad, bad
