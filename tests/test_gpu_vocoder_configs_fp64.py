"""HiFi-GAN V2, V3 and the envelope configs (``offstd``, ``v3_512``, ``rb1_2lvl``) on the MI355X against the fp64 restatement
(tests/vocoder_ref.py), row by row, on every path the engine can take for them, at the gates test_gpu_vocoder_v1.py holds V1 to.

Every comparison is per row, under arithmetic settings 16 / 6 / 0, with two checkpoints of the config: the standard synthetic weights and
the linear-regime weights (conv_post x 0.05), whose output tanh does not shrink upstream errors (test_vocoder_configs_reference.py).

  small      full rows at T in {1 .. 300} x B in {1, 3}, all five configs (partial tiles at every level: V3 stores 58 / 32 frames of a tile
             at level 1, 122 / 96 at level 2, 250 / 224 / 166 at level 3), and a ragged B = 5 batch padded with MEL_MEAN_EMOJI
  streams    B = 32 at T = 512 (three MRF streams, balancing off) and T = 513 (one stream) for v2 / v3 / offstd on 8 rows; 4 x 100 on
             three streams and with the fan-out switched off
  batch      B = 64 x T = 516 for v2 / v3, full rows and ragged, every row (head, tail, rotating interior window): the single-stream plan
             tools/vocoder_configs_bench.py times; setting 16 again with set_chain(False) and with set_amax(False)
  switches   set_chain and EV_RB2_MINKEEP change the launch count as documented, and every such engine holds the gates
  setting 3  the ~16-bit opt-in arithmetic FAILS the same per-row check: the gates tell 16 significand bits from 23

The fp64 references run through torch on the GPU (one window per case is also run on the CPU and must agree to 1e-10), with the margin
``vocoder_ref.default_margin(h)`` that follows the config's receptive field.  Beside every table line stands the error of the plain fp32
torch restatement (``restate_body(..., dtype=float32)`` on torch's own conv kernels, not the HIP path) against fp64 on the same windows:
how far an honest fp32 evaluation sits below the gate.

Gates (vocoder_ref.GATE, V1's: the deepest config, the same kernel families and arithmetic), per row over the compared samples: standard
weights RMS <= 5e-6, L-inf <= 5e-5; linear-regime weights RMS <= 5e-6 and L-inf <= 3e-5 of that row's fp64 RMS; the row's fp64 RMS
above 0.2 / 0.01.  Worst values measured on an MI355X over every case and setting: profiles/vocoder_configs_fp64_errors.txt.
"""
import time

import pytest
import torch

from emojivoice_amd import weights as W
from emojivoice_amd.hifigan import AttrDict, Generator
from test_vocoder_configs_reference import NAMES, configs
from vocoder_ref import WEIGHTS, check, fanout_planned, gpu_refs, linear_regime_state, row_windows, run, sweep

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LABEL = "VCERR"
CONFIGS = configs()
_CLOCK = {"gpu_ref": 0.0, "cpu_ref": 0.0}
_SDS, _VOCS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report_clock():
    t0 = time.perf_counter()
    yield
    for v in _VOCS.values():
        for g in v.values():
            g.engine.close()
    _VOCS.clear()
    print(f"\nVCCLOCK wall {time.perf_counter() - t0:.1f} s  fp64 / fp32 references on the GPU {_CLOCK['gpu_ref']:.1f} s  "
          f"on the CPU {_CLOCK['cpu_ref']:.1f} s ({torch.get_num_threads()} threads)")


def _sds(name):
    if name not in _SDS:
        _SDS[name] = {"std": W.synthetic_hifigan_state(CONFIGS[name]), "lin": linear_regime_state(CONFIGS[name])}
    return _SDS[name]


def _generator(name, weights):
    g = Generator(AttrDict(CONFIGS[name])).to(DEV)
    g.load_state_dict(_sds(name)[weights])
    g._sync_engine()
    return g


def _vocs(name):
    """{weights: Generator} of a config, one engine each, made on first use and kept for the module."""
    if name not in _VOCS:
        _VOCS[name] = {w: _generator(name, w) for w in WEIGHTS}
    return _VOCS[name]


def _refs(name, mel, wins, check_cpu=1):
    """(fp64 references, fp32 torch restatement) of the windows, {weights: [samples]} each."""
    return gpu_refs(_sds(name), mel, CONFIGS[name], wins, _CLOCK, check_cpu=check_cpu, device=DEV, f32=True)


def _mel(B, T, seed):
    return torch.randn(B, 80, T, generator=torch.Generator().manual_seed(seed)).to(DEV) * 2.0 - 5.0


def _sweep(name, tag, mel, wins, refs, bad, **kw):
    return sweep(f"{name} {tag}", _vocs(name), mel, wins, refs[0], bad, f32=refs[1], label=LABEL, **kw)


def _check(name, tag, weights, wav, wins, refs, bad):
    check(f"{name} {tag}", weights, wav, wins, refs[0][weights], bad, label=LABEL, f32=refs[1][weights])


# ---------------------------------------------------------------------------------------------------------------------
# odd and small shapes, full rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 7, 33, 65, 129, 257, 300])
@pytest.mark.parametrize("name", NAMES)
def test_small_shapes_full_rows(name, T):
    mel3 = _mel(3, T, 7000 + T)
    wins = [(r, 0, T) for r in range(3)]
    refs = _refs(name, mel3, wins)                          # rows do not interact: the B = 1 reference is row 0 of B = 3
    bad = []
    for B in (1, 3):
        sub = tuple({w: r[w][:B] for w in WEIGHTS} for r in refs)
        _sweep(name, f"small {B}x{T}", mel3[:B].contiguous(), wins[:B], sub, bad)
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_small_ragged_batch(name):
    lengths = [300, 257, 129, 33, 1]
    mel = torch.full((5, 80, 300), W.MEL_MEAN_EMOJI)
    g = torch.Generator().manual_seed(55)
    for r, L in enumerate(lengths):
        mel[r, :, :L] = torch.randn(80, L, generator=g) * 2.0 - 5.0
    mel = mel.to(DEV)
    wins = [(r, 0, L) for r, L in enumerate(lengths)]
    bad = []
    _sweep(name, "small ragged 5x300", mel, wins, _refs(name, mel, wins), bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# both sides of the three-stream threshold (B * T <= 16384)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v2", "v3", "offstd"])
def test_both_sides_of_the_stream_threshold(name):
    B, rows = 32, [0, 1, 6, 11, 17, 22, 30, 31]
    vocs = _vocs(name)
    mel513 = _mel(B, 513, 513)
    mel512 = mel513[..., :512].contiguous()
    # (window ends <= 466: farther from frame 512 than offstd's reach of 18.62 frames, so one fp64 serves both lengths)
    shared = [(r, 0, 8) for r in rows] + [(r, 16 + (61 * r) % 450, 24 + (61 * r) % 450) for r in rows]
    ref_shared = _refs(name, mel513, shared)
    tails = {T: [(r, T - 8, T) for r in rows] for T in (512, 513)}
    ref_tail = {T: _refs(name, m, tails[T], check_cpu=0) for T, m in ((512, mel512), (513, mel513))}
    bad, epochs = [], {}
    for T, m in ((512, mel512), (513, mel513)):
        wins = shared + tails[T]
        refs = tuple({w: a[w] + b[w] for w in WEIGHTS} for a, b in zip(ref_shared, ref_tail[T]))
        epochs[T] = _sweep(name, f"streams 32x{T}", m, wins, refs, bad)
    mel = _mel(4, 100, 100)
    wins = [(r, 0, 100) for r in range(4)]
    refs = _refs(name, mel, wins)
    epochs["4x100 three streams"] = _sweep(name, "streams 4x100", mel, wins, refs, bad)
    saved = {w: vocs[w].engine.mrf_streams_max for w in WEIGHTS}
    try:
        for w in WEIGHTS:
            vocs[w].engine.set_mrf_streams_max(0)
        epochs["4x100 one stream"] = _sweep(name, "streams 4x100 fan-out off", mel, wins, refs, bad)
    finally:
        for w in WEIGHTS:
            vocs[w].engine.set_mrf_streams_max(saved[w])
    plans = {T: fanout_planned(vocs["std"].engine, B, T) for T in (512, 513)}
    print(f"VCPATH {name} streams balanced launches per call {epochs}  fan-out planned {plans}")
    assert not bad, bad
    assert plans == {512: True, 513: False}, plans      # T = 512: three streams; T = 513: one
    # the fan-out turns balancing off for the levels it forks (conv_pre runs before the fork and may still balance: V3 at 32 x 512 does)
    assert all(e == 0 for e in epochs["4x100 three streams"].values()), epochs


# ---------------------------------------------------------------------------------------------------------------------
# the batch plan: B = 64 x 516, one stream, every row
# ---------------------------------------------------------------------------------------------------------------------
B64, T64 = 64, 516


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("name", ["v2", "v3"])
def test_batch_plan_every_row(name, ragged):
    vocs = _vocs(name)
    mel = _mel(B64, T64, 516)
    lengths = [T64 - (37 * r) % 300 for r in range(B64)] if ragged else [T64] * B64
    for r, L in enumerate(lengths):
        mel[r, :, L:] = W.MEL_MEAN_EMOJI                  # the decoder's padding past each length
    wins = row_windows(lengths)
    refs = _refs(name, mel, wins)
    tag = f"batch 64x516{' ragged' if ragged else ''}"
    bad = []
    epochs = _sweep(name, tag, mel, wins, refs, bad)
    for w in WEIGHTS:
        wav, _ = run(vocs[w], mel, 16, chain=False)
        _check(name, f"{tag} s16 chain off", w, wav, wins, refs, bad)
        wav, _ = run(vocs[w], mel, 16, amax=False)
        _check(name, f"{tag} s16 amax off", w, wav, wins, refs, bad)
    print(f"VCPATH {name} {tag} balanced launches per call {epochs}")
    assert not bad, bad
    assert not fanout_planned(vocs["std"].engine, B64, T64)   # one stream: the plan a batch takes


# ---------------------------------------------------------------------------------------------------------------------
# the switches switch, and what they switch to holds the gates
# ---------------------------------------------------------------------------------------------------------------------
def _launches(voc, chain=True):
    """Launches of one 1 x 64 call (profiling on: the call stays on one stream)."""
    eng = voc.engine
    mel = _mel(1, 64, 5)
    eng.set_chain(chain)
    eng.profile_enable(True)
    try:
        eng.profile_read(reset=True)
        voc(mel)
        torch.cuda.synchronize()
        return eng.profile_read(reset=True)[2], eng.last_cfg()
    finally:
        eng.profile_enable(False)
        eng.set_chain(True)


@pytest.mark.parametrize("name", ["v2", "v3", "offstd"])
def test_chain_switch_changes_the_launch_count(name):
    voc = _vocs(name)["std"]
    (on, cfg_on), (off, cfg_off) = _launches(voc, True), _launches(voc, False)
    print(f"VCPATH {name} launches at 1x64: chain on {on} (last cfg {cfg_on}), off {off} (last cfg {cfg_off})")
    assert 0 < on < off, (on, off)
    if name == "v3":
        assert cfg_on == 207 and cfg_off != 207, (cfg_on, cfg_off)   # the last ResBlock2 (k = 7, d = 3 / 12, 32 channels) as one resblock2_h16_kernel


def test_rb2_minkeep_moves_the_gate(monkeypatch):
    """EV_RB2_MINKEEP (read when the engine is created) = 8: no ResBlock2 runs fused, as with set_chain(False); = 2: the k = 7 block at
    64 channels (38 of 128 frames stored per tile) joins the fused ones.  Both engines hold the gates at 2 x 100 and 1 x 300."""
    default = _vocs("v3")["std"]
    n_default, n_off = _launches(default)[0], _launches(default, chain=False)[0]
    counts, bad = {}, []
    cases = [(_mel(2, 100, 21), [(r, 0, 100) for r in range(2)]), (_mel(1, 300, 22), [(0, 0, 300)])]
    refs = [_refs("v3", mel, wins, check_cpu=0) for mel, wins in cases]
    for keep in (8, 2):
        monkeypatch.setenv("EV_RB2_MINKEEP", str(keep))
        vocs = {w: _generator("v3", w) for w in WEIGHTS}
        monkeypatch.delenv("EV_RB2_MINKEEP")
        try:
            counts[keep] = _launches(vocs["std"])[0]
            for (mel, wins), ref in zip(cases, refs):
                sweep(f"v3 minkeep {keep} {mel.shape[0]}x{mel.shape[2]}", vocs, mel, wins, ref[0], bad, f32=ref[1], label=LABEL)
        finally:
            for g in vocs.values():
                g.engine.close()
    print(f"VCPATH v3 launches at 1x64: default {n_default}, chain off {n_off}, EV_RB2_MINKEEP {counts}")
    assert counts[8] == n_off and counts[2] < n_default < n_off, (counts, n_default, n_off)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the gates tell 16 significand bits from 23
# ---------------------------------------------------------------------------------------------------------------------
def test_setting_3_fails_the_gate():
    """Arithmetic setting 3 (three bf16 products per fp32 product, ~16 significand bits; include/emojivoice.h: "NOT fp32-grade") through the
    same per-row check, linear-regime checkpoint, 3 x 129: it must FAIL on at least one row.

    V2 only.  Setting 3 exists in two places: the conv launches of deep grids (at least 4 tiles of 128 x 128 per CU), which no 3 x 129
    call of any config has, and the fused ResBlock1 pairs (resblock_pair_split_kernel), which V2's 64- and 32-channel levels take.  V3
    is ResBlock2 throughout: under setting 3 its blocks run as plain conv launches, so no launch of it is reached — its setting-3
    output is asserted bit-equal to its setting-0 output instead, and it is left out of the must-fail check."""
    B, T = 3, 129
    mel = _mel(B, T, 3129)
    wins = [(r, 0, T) for r in range(B)]
    refs = _refs("v2", mel, wins, check_cpu=0)
    wav, _ = run(_vocs("v2")["lin"], mel, 3)
    bad = []
    _check("v2", "setting 3 3x129", "lin", wav, wins, refs, bad)
    assert bad, "setting 3 passed the per-row gate on every row of V2"
    wav16, _ = run(_vocs("v2")["lin"], mel, 16)
    ok = []
    _check("v2", "setting 16 3x129", "lin", wav16, wins, refs, ok)   # (the same rows pass under the shipped arithmetic)
    assert not ok, ok
    v3 = _vocs("v3")["lin"]
    assert torch.equal(run(v3, mel, 3)[0], run(v3, mel, 0)[0])       # no launch of V3 at this shape has a setting-3 form
