"""The CFM decoder on the MI355X against the fp64 restatement (tests/decoder_ref.py), row by row, at gates set from measured error.

What is compared: ``dec`` of ev_cfm_decode2 (the normalised decoder output) on every valid frame of every row, against ``decode`` of
decoder_ref in fp64 (time grid and sinusoid in fp32, as the reference and the engine define them).  The fp64 references run through
torch on the GPU and are cached across settings; one small case is also run on the CPU and must agree to 1e-10.  Besides the gate,
every call's outputs are finite, the padded frames of ``dec`` hold the Euler state's input exactly (the velocity is exactly 0 there,
as in the reference), and ``mel`` is ``dec * mel_std + mel_mean``.

Cases (standard synthetic weights unless named):
  bench     bench.make_inputs(64, 516, 0, 64), z x 0.667, 10 steps, every row; the same tensors with ragged lengths (1, 2, 3, 4, 515,
            516 and odd / even lengths between).  Under arithmetic settings 16, 6 and 0, setting 16 with set_attn_h16(False) and with
            set_amax(False).  At this shape the U-Net takes the balanced persistent builds (SkCtl: conv_gemm_bal, the balanced ln_mlp),
            the fused LayerNorm + QKV and fp16-pipe attention (attn_out_h16_kernel) under setting 16, and the bf16-split builds under
            settings 16 and 6: the balanced-launch epoch (Engine.sk_stats) and profile_read_split show they ran.
  estimator one Engine.estimator call at the bench shape, t in {0, 0.5, 0.9}: one velocity field, no ten-step averaging.  Its gate is
            its own and twice as loose as the decode's relative to the row's RMS: one call's error is not averaged over ten steps.
  small     Tp = 4 .. 132 step 4 and 256, 260, 512, 516, 1032 at B = 1, 2, 3 (lengths Tp; Tp, Tp - 1; Tp / 2 + 1, 1, Tp), 3 steps:
            partial 32 / 64-row tiles at both U-Net resolutions, key-tile edges of the attention (33 key tiles at 1032), and the
            B = 1 builds (conv_sk32, split-key attention, per-tile GroupNorm statistics).
  mid       B = 8 x 516 and B = 48 x 284 (lengths up to 283), near where the balanced grids switch on (nt64 >= ncu).
  switches  the builds behind environment switches (read once in ev_create): one child process per switch and one default child per
            shape, compared with the parent's cached fp64 references.  Each child also reports its balanced launches, its fp16 / split
            launches and its profiled launches (kind, widths, taps, rows, tile config, epilogue): every switch but the six of
            PROFILE_BLIND must change them, and EV_NO_QKV_H16 must take exactly the 6 x 10 ln_qkv_h16 and 6 x 10 attn_out_h16 launches off.
  graphs    MatchaTTS.enable_decode_graphs replays at two shapes; then capture A (1 x 396), eager B (1 x 64), replay A, and
            Engine.estimator at B on the same handle: every call of a handle that holds graphs re-zeroes its own plan (ensure_ws).
  peaked    decoder_ref.peaked_attention_state (to_q, to_k x 4: peaked softmaxes) on the bench batch and small shapes, settings 16 / 0,
            after PEAK_STEPS = 2 Euler steps; and the bench batch after 10 steps, held to a plain fp32 evaluation of the same rows.
  mutant    one fp16 rounding of z must exceed the standard gate on every bench row: the gate is not vacuous.  (set_arithmetic(3) runs
            the U-Net exactly as setting 0 does, so it is no mutant for the decoder.)

Gates, per row, relative to the row's fp64 RMS (decoder_ref.GATE*; a short row of a long padded batch has an RMS near 10, because
GroupNorm statistics include the padded frames): standard weights RMS <= 3.5e-6 and L-inf <= 1.5e-5 on ``dec``; one estimator call
RMS <= 7e-6 and L-inf <= 3.5e-5 on the velocity; peaked weights after 2 steps RMS <= 3.9e-4 and L-inf <= 3.2e-3.  The reference row's
RMS must exceed 0.3.  Worst values measured on an MI355X over every case, setting and switch (DECERR and DECWORST print with -s):
  standard dec 1.0e-6 / 4.3e-6 (ragged bench batch and its switches; full-length bench rows 3.2e-7 / 1.8e-6 at setting 16),
  estimator 2.1e-6 / 1.0e-5, peaked dec 1.3e-4 / 1.07e-3.  Each gate is 3.0-3.6x its worst value.

Why the peaked cases stop at 2 steps: with peaked softmaxes the U-Net amplifies any fp32 rounding chaotically over the Euler chain.
After 10 steps at the bench shape, a plain fp32 evaluation (decoder_ref in fp32 through torch on the GPU) is off fp64 by a relative
RMS of 2.0e-3 on its worst row and 4.3e-5 on its median row; the engine by 1.4e-3 / 3.3e-5 (setting 16) and 1.9e-3 / 4.8e-5
(setting 0), so no fp32-grade gate exists there.  After 1 step both are at 2e-5.  The 10-step case is therefore held to the fp32
evaluation (worst and median row within 3x), and the 2-step gate is one that q / k rounded to fp16, or a score scale off by 2^-8,
exceed by 10x (tests/test_decoder_reference.py).

Measured run time of this module on one MI355X: 70-73 s, 58 s of it in the 20 switch children.
"""
import os
import subprocess
import sys
import time

import pytest
import torch

import bench
import decoder_ref as R
from emojivoice_amd import weights as W
from emojivoice_amd.matcha_tts import MatchaTTS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = (16, 6, 0)
_CLOCK = {"gpu_ref": 0.0, "cpu_ref": 0.0, "children": 0.0}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_clock():
    t0 = time.perf_counter()
    yield
    print(f"\nDECCLOCK wall {time.perf_counter() - t0:.1f} s  fp64 references on the GPU {_CLOCK['gpu_ref']:.1f} s  on the CPU "
          f"{_CLOCK['cpu_ref']:.1f} s  switch children {_CLOCK['children']:.1f} s")
    print("DECWORST (relative) " + "  ".join(f"{k} rms {v[0]:.2e} linf {v[1]:.2e}" for k, v in sorted(_WORST.items())))


@pytest.fixture(scope="module")
def sds():
    return {"std": W.synthetic_matcha_state(), "peak": R.peaked_attention_state()}


@pytest.fixture(scope="module")
def models(sds):
    return {w: MatchaTTS(sd, device=DEV) for w, sd in sds.items()}


@pytest.fixture(scope="module")
def esds(sds):
    return {w: R.estimator_state(sd, torch.float64, DEV) for w, sd in sds.items()}


def _ref(sds, esds, w, mu, lengths, spk, z0, n, check_cpu=False):
    """fp64 dec of decoder_ref on the GPU (and, with check_cpu, on the CPU too: both agree to 1e-10)."""
    t0 = time.perf_counter()
    ref = R.decode(sds[w], mu, lengths.cpu(), spk, z0, n, device=DEV, esd=esds[w]).cpu()
    _CLOCK["gpu_ref"] += time.perf_counter() - t0
    if check_cpu:
        t0 = time.perf_counter()
        cpu = R.decode(sds[w], mu.cpu(), lengths.cpu(), spk.cpu(), z0.cpu(), n)
        _CLOCK["cpu_ref"] += time.perf_counter() - t0
        assert float((cpu - ref).abs().max()) <= 1e-10
    return ref


def _run(model, mu, lengths, spk, z0, n, setting=16, attn_h16=True, amax=True, profile=False):
    """(dec, mel, balanced launches, bf16-split launches or None) of one ev_cfm_decode2 call under one setting."""
    eng = model.engine
    eng.set_arithmetic(setting)
    eng.set_attn_h16(attn_h16)
    eng.set_amax(amax)
    split = None
    try:
        e0 = eng.sk_stats()[0]
        if profile:
            eng.profile_enable(True)
        dec, mel = eng.cfm_decode2(mu, lengths, spk, z0, n, model.mel_std, model.mel_mean)
        torch.cuda.synchronize()
        if profile:
            split = eng.profile_read_split()[2]
        e1 = eng.sk_stats()[0]
    finally:
        if profile:
            eng.profile_enable(False)
        eng.set_arithmetic(16)
        eng.set_attn_h16(True)
        eng.set_amax(True)
    return dec, mel, (e1 - e0) & 0xFFFFFFFF, split


def _check(tag, w, dec, ref, lengths, bad, z0=None, mel=None, model=None, gate=None, record=True):
    """Per row over its valid frames: (RMS, L-inf) of dec - ref relative to the row's fp64 RMS, gated;
    outputs finite, padded frames == z0, mel == dec * std + mean.  One DECERR line per call; returns the worst (rms, linf) seen."""
    g_rms, g_linf = gate or (R.GATE if w == "std" else R.GATE_PEAKED)
    dec_c = dec.double().cpu()
    worst = [0.0, 0.0, 0.0, 0.0, float("inf")]
    for r, L in enumerate(lengths.tolist()):
        got, rf = dec_c[r, :, :L], ref[r, :, :L]
        e = got - rf
        rms, linf, rr = float(e.pow(2).mean().sqrt()), float(e.abs().max()), float(rf.pow(2).mean().sqrt())
        worst = [max(worst[0], rms), max(worst[1], linf), max(worst[2], rms / rr), max(worst[3], linf / rr), min(worst[4], rr)]
        if not (rms <= g_rms * rr and linf <= g_linf * rr and rr > R.REF_FLOOR):
            bad.append((tag, w, r, L, rms, linf, rr))
    if not bool(torch.isfinite(dec).all()):
        bad.append((tag, w, "non-finite dec"))
    if z0 is not None:
        for r, L in enumerate(lengths.tolist()):
            if not torch.equal(dec[r, :, L:], z0[r, :, L:]):
                bad.append((tag, w, r, "padded frames of dec differ from the input state"))
    if mel is not None:
        scaled = dec.double() * model.mel_std
        d = float(((mel.double() - (scaled + model.mel_mean)).abs() / (scaled.abs() + abs(model.mel_mean))).max())
        if not (bool(torch.isfinite(mel).all()) and d <= 2.4e-7):          # two fp32 roundings (of dec * std, then of + mean)
            bad.append((tag, w, "mel != dec * std + mean", d))
    if record:
        key = "est" if gate is not None else w
        _WORST[key] = (max(_WORST.get(key, (0, 0))[0], worst[2]), max(_WORST.get(key, (0, 0))[1], worst[3]))
    print(f"DECERR {tag:<40s} {w:<4s} rms {worst[0]:.2e}  linf {worst[1]:.2e}  rel rms {worst[2]:.2e}  rel linf {worst[3]:.2e}  "
          f"min ref rms {worst[4]:.3f}")
    return worst


def _spk(model, ids):
    return model._sd["spk_emb.weight"][ids.to(DEV)].float().contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the bench batch: B = 64 x 516, 10 steps, every row
# ---------------------------------------------------------------------------------------------------------------------
B64, T64, N64 = 64, 516, 10
N_PEAK = R.PEAK_STEPS


def _ragged_lengths(B=B64, T=T64):
    """Odd and even lengths over the batch, with 1, 2, 3, 4, T - 1 and T spread over it."""
    L = [5 + (89 * r) % (T - 6) for r in range(B)]
    for pos, v in zip((0, B // 5, 2 * B // 5, 3 * B // 5, 4 * B // 5, B - 1), (T, 1, T - 1, 2, 4, 3)):
        L[pos] = v
    return torch.tensor(L, dtype=torch.int32)


@pytest.fixture(scope="module")
def bench_case(models, sds, esds):
    mu, z, spk_ids, _ = bench.make_inputs(B64, T64, 0, B64, torch.device(DEV))
    z0 = (z * 0.667).contiguous()
    spk = _spk(models["std"], spk_ids)
    full = torch.full((B64,), T64, dtype=torch.int32)
    ragged = _ragged_lengths()
    refs = {}
    for name, L in (("full", full), ("ragged", ragged)):
        refs[(name, "std")] = _ref(sds, esds, "std", mu, L, spk, z0, N64)
        refs[(name, "peak")] = _ref(sds, esds, "peak", mu, L, spk, z0, N_PEAK)
    return mu, z0, spk, {"full": full, "ragged": ragged}, refs


def test_bench_batch_every_row(models, bench_case):
    mu, z0, spk, lens, refs = bench_case
    bad, paths = [], {}
    m = models["std"]
    for name in ("full", "ragged"):
        L = lens[name].to(DEV)
        for s in SETTINGS:
            dec, mel, ep, split = _run(m, mu, L, spk, z0, N64, s, profile=True)
            _check(f"bench 64x516 {name} s{s}", "std", dec, refs[(name, "std")], lens[name], bad, z0, mel, m)
            paths[(name, s)] = (ep, split)
        dec, mel, ep, split = _run(m, mu, L, spk, z0, N64, 16, attn_h16=False, profile=True)
        _check(f"bench 64x516 {name} s16 attn_h16 off", "std", dec, refs[(name, "std")], lens[name], bad, z0, mel, m)
        paths[(name, "attn32")] = (ep, split)
        dec, mel, ep, split = _run(m, mu, L, spk, z0, N64, 16, amax=False)
        _check(f"bench 64x516 {name} s16 amax off", "std", dec, refs[(name, "std")], lens[name], bad, z0, mel, m)
    print(f"DECPATH bench (balanced launches, bf16-split launches) per call {paths}")
    assert not bad, bad
    for name in ("full", "ragged"):
        assert paths[(name, 16)][0] > 0 and paths[(name, 6)][0] > 0, paths       # balanced persistent builds ran (settings 16, 6)
        assert paths[(name, 16)][1] > 0 and paths[(name, 6)][1] > 0, paths       # bf16-split / fp16 builds ran
        assert paths[(name, 0)][1] == 0, paths                                     # setting 0: every product on the fp32 MFMA
        # attn_out_h16_kernel ran for each of the six transformer blocks of every step, and set_attn_h16(False) took it off
        assert paths[(name, 16)][1] - paths[(name, "attn32")][1] == 6 * N64, paths


def test_bench_batch_peaked_attention(models, bench_case):
    mu, z0, spk, lens, refs = bench_case
    bad = []
    m = models["peak"]
    for name in ("full", "ragged"):
        for s in (16, 0):
            dec, mel, _, _ = _run(m, mu, lens[name].to(DEV), spk, z0, N_PEAK, s)
            _check(f"bench 64x516 {name} {N_PEAK} steps s{s}", "peak", dec, refs[(name, "peak")], lens[name], bad, z0, mel, m)
    assert not bad, bad


def _row_rel_rms(dec, ref):
    e = (dec.double().cpu() - ref).flatten(1)
    return e.pow(2).mean(1).sqrt() / ref.flatten(1).pow(2).mean(1).sqrt()


def test_bench_batch_peaked_ten_steps_no_worse_than_fp32(models, sds, esds, bench_case):
    """Ten steps with peaked weights: the engine's per-row error against fp64 is held to that of an independent plain fp32 evaluation
    (decoder_ref in fp32 through torch on the GPU) of the same rows: worst and median row each within 3x (measured 0.6-1.1x)."""
    mu, z0, spk, lens, _ = bench_case
    L = lens["full"]
    t0 = time.perf_counter()
    ref = R.decode(sds["peak"], mu, L, spk, z0, N64, device=DEV, esd=esds["peak"]).cpu()
    f32 = R.decode(sds["peak"], mu, L, spk, z0, N64, torch.float32, device=DEV, esd=R.estimator_state(sds["peak"], torch.float32, DEV))
    _CLOCK["gpu_ref"] += time.perf_counter() - t0
    e32 = _row_rel_rms(f32, ref)
    ratios = {}
    for s in (16, 0):
        dec, _, _, _ = _run(models["peak"], mu, L.to(DEV), spk, z0, N64, s)
        e = _row_rel_rms(dec, ref)
        assert bool(torch.isfinite(dec).all())
        ratios[s] = (float(e.max() / e32.max()), float(e.median() / e32.median()))
        print(f"DECERR bench 64x516 full 10 steps s{s} peak  rel rms worst {float(e.max()):.2e} median {float(e.median()):.2e}  "
              f"(plain fp32: {float(e32.max()):.2e} / {float(e32.median()):.2e})")
    assert all(w <= 3.0 and m <= 3.0 for w, m in ratios.values()), ratios


def test_gate_sees_one_fp16_rounding_of_z(models, bench_case):
    """The gate is not vacuous: one fp16 rounding of the engine's input state z (a single 2^-11 relative error at the start of the
    chain) must fail it on the bench batch.  (Arithmetic setting 3, documented as not fp32-grade, cannot serve: the U-Net runs it on
    the fp32 MFMA builds of setting 0, and measured dec equals setting 0's.)"""
    mu, z0, spk, lens, refs = bench_case
    bad = []
    dec, _, _, _ = _run(models["std"], mu, lens["full"].to(DEV), spk, z0.half().float(), N64)
    w = _check("bench 64x516 full s16 z in fp16 (mutant)", "std", dec, refs[("full", "std")], lens["full"], bad, record=False)
    assert len(bad) == B64, "one fp16 rounding of z stayed inside the gate on some row"
    assert w[2] > 10 * R.GATE[0]


def test_estimator_one_call(models, sds, esds, bench_case):
    mu, z0, spk, lens, _ = bench_case
    bad = []
    m = models["std"]
    for name in ("full", "ragged"):
        L = lens[name]
        for t in (0.0, 0.5, 0.9):
            t0 = time.perf_counter()
            ref = R.velocity(sds["std"], z0, mu, L, spk, t, device=DEV, esd=esds["std"]).cpu()
            _CLOCK["gpu_ref"] += time.perf_counter() - t0
            for s in SETTINGS:
                m.engine.set_arithmetic(s)
                try:
                    v = m.engine.estimator(z0, mu, L.to(DEV), spk, t)
                    torch.cuda.synchronize()
                finally:
                    m.engine.set_arithmetic(16)
                _check(f"estimator 64x516 {name} t={t} s{s}", "std", v, ref, L, bad, gate=R.GATE_EST)
                for r, n in enumerate(L.tolist()):
                    if bool((v[r, :, n:] != 0).any()):
                        bad.append(("estimator", name, t, s, r, "velocity not 0 on padded frames"))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# small and edge shapes: full rows at B = 1, 2, 3
# ---------------------------------------------------------------------------------------------------------------------
SMALL_TP = list(range(4, 133, 4)) + [256, 260, 512, 516, 1032]
N_SMALL = 3


def _small_inputs(model, Tp, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(3, 80, Tp, generator=g)
    z0 = torch.randn(3, 80, Tp, generator=g) * 0.667
    ids = torch.tensor([107, 58, 12])
    return mu.to(DEV), z0.to(DEV), _spk(model, ids)


def _small_plan(Tp):
    """[(B, row indices into the 5-row reference, lengths)]: the reference rows are (input row, length) pairs, rows being independent
    (tests/test_decoder_reference.py)."""
    half = Tp // 2 + 1
    ref_rows = [(0, Tp), (1, Tp - 1), (0, half), (1, 1), (2, Tp)]
    calls = [(1, [0], [Tp]), (2, [0, 1], [Tp, Tp - 1]), (3, [2, 3, 4], [half, 1, Tp])]
    return ref_rows, calls


def _small_refs(sds, esds, w, mu, z0, spk, Tp, n, check_cpu=False):
    ref_rows, _ = _small_plan(Tp)
    idx = torch.tensor([r for r, _ in ref_rows])
    L = torch.tensor([l for _, l in ref_rows], dtype=torch.int32)
    return _ref(sds, esds, w, mu[idx.to(DEV)], L, spk[idx.to(DEV)], z0[idx.to(DEV)], n, check_cpu)


def _small_sweep(models, w, mu, z0, spk, Tp, ref, bad, settings=SETTINGS, n=N_SMALL):
    ref_rows, calls = _small_plan(Tp)
    m = models[w]
    for B, rows, L in calls:
        idx = torch.tensor([ref_rows[i][0] for i in rows], device=DEV)
        mu_b, z_b, spk_b = mu[idx].contiguous(), z0[idx].contiguous(), spk[idx].contiguous()
        Lt = torch.tensor(L, dtype=torch.int32)
        for s in settings:
            dec, mel, _, _ = _run(m, mu_b, Lt.to(DEV), spk_b, z_b, n, s)
            _check(f"small {B}x{Tp} s{s}", w, dec, ref[rows], Lt, bad, z_b, mel, m)


@pytest.mark.parametrize("Tp", SMALL_TP)
def test_small_shapes(models, sds, esds, Tp):
    mu, z0, spk = _small_inputs(models["std"], Tp, 9000 + Tp)
    bad = []
    ref = _small_refs(sds, esds, "std", mu, z0, spk, Tp, N_SMALL, check_cpu=(Tp == 36))
    _small_sweep(models, "std", mu, z0, spk, Tp, ref, bad)
    if Tp in (36, 132, 516, 1032):
        ref = _small_refs(sds, esds, "peak", mu, z0, spk, Tp, N_PEAK)
        _small_sweep(models, "peak", mu, z0, spk, Tp, ref, bad, settings=(16, 0), n=N_PEAK)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# mid batches, near the balanced grids' threshold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tp", [(8, 516), (48, 284), (32, 772)])
def test_mid_batches(models, sds, esds, B, Tp):
    g = torch.Generator().manual_seed(B * 1000 + Tp)
    mu = torch.randn(B, 80, Tp, generator=g).to(DEV)
    z0 = (torch.randn(B, 80, Tp, generator=g) * 0.667).to(DEV)
    spk = _spk(models["std"], torch.tensor([(5 * r + 3) % 109 for r in range(B)]))
    L = torch.tensor([min(Tp - 1, Tp - 1 - (53 * r) % (Tp - 8)) if r else Tp - 1 for r in range(B)], dtype=torch.int32)
    if Tp > 768:
        # 32 x 772: the first Tp above 768 at the smallest batch of groupnorm_mish_kernel<512> — its three-pass fallback in all three
        # epilogue modes inside the estimator; lengths up to 771, one utterance of a single frame
        L[B - 1] = 1
    ref = _ref(sds, esds, "std", mu, L, spk, z0, N64)
    bad, epochs = [], {}
    for s in SETTINGS:
        dec, mel, ep, split = _run(models["std"], mu, L.to(DEV), spk, z0, N64, s, profile=True)
        _check(f"mid {B}x{Tp} s{s}", "std", dec, ref, L, bad, z0, mel, models["std"])
        epochs[s] = (ep, split)
    print(f"DECPATH mid {B}x{Tp} (balanced launches, bf16-split launches) per call {epochs}")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# builds behind environment switches: one child process each
# ---------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys, torch
sys.path.insert(0, %r)
from emojivoice_amd import weights as W
from emojivoice_amd.matcha_tts import MatchaTTS
inp = torch.load(sys.argv[1])
dev = torch.device("cuda", 0)
m = MatchaTTS(W.synthetic_matcha_state(), device=dev)
e0 = m.engine.sk_stats()[0]
m.engine.profile_enable(True)
dec, mel = m.engine.cfm_decode2(inp["mu"].to(dev), inp["len"].to(dev), inp["spk"].to(dev), inp["z0"].to(dev), inp["n"], m.mel_std, m.mel_mean)
torch.cuda.synchronize()
split = m.engine.profile_read_split()[2]
os.environ["EV_PROFILE_DUMP"] = sys.argv[2] + ".prof"
m.engine.profile_read()
m.engine.profile_enable(False)
sig = sorted(tuple(l.split()[:8]) for l in open(sys.argv[2] + ".prof") if l.strip() and not l.startswith("#"))
torch.save({"dec": dec.cpu(), "epoch": (m.engine.sk_stats()[0] - e0) & 0xFFFFFFFF, "split": split, "sig": sig}, sys.argv[2])
""" % REPO

SWITCHES = {
    "b64": [{"EV_NO_SK_BALANCE": "1"}, {"EV_FUSE_ATTN": "0", "EV_SK_WGS": "3"}, {"EV_FUSE_MLP": "0"}, {"EV_NO_QKV_H16": "1"},
            {"EV_SPLIT": "0"}, {"EV_SPLIT": "6"}],
    "b3": [{"EV_FUSE_MLP_MIN": "1"}, {"EV_NO_LEAN": "1"}, {"EV_FORCE_CFG": "0"}, {"EV_FORCE_CFG": "5"}, {"EV_FORCE_CFG": "6"}],
    "b1": [{"EV_NO_ATTN_SK": "1"}, {"EV_NO_GN_STATS": "1"}, {"EV_NO_SK32_LEAN": "1"}, {"EV_ATTN_TPW": "1"}, {"EV_ATTN_TPW": "3"},
           {"EV_NO_SK": "1"}],
}


PROFILE_BLIND = ["b3 EV_NO_LEAN=1", "b1 EV_NO_ATTN_SK=1", "b1 EV_NO_GN_STATS=1", "b1 EV_NO_SK32_LEAN=1", "b1 EV_ATTN_TPW=1",
                 "b1 EV_ATTN_TPW=3"]


def test_switch_builds(models, sds, esds, bench_case, tmp_path):
    mu, z0, spk, lens, refs = bench_case
    cases = {"b64": (mu, z0, spk, lens["ragged"], N64, refs[("ragged", "std")])}
    g = torch.Generator().manual_seed(44)
    for name, B, Tp, L in (("b3", 3, 44, [44, 31, 17]), ("b1", 1, 100, [100])):
        m_, z_ = torch.randn(B, 80, Tp, generator=g).to(DEV), (torch.randn(B, 80, Tp, generator=g) * 0.667).to(DEV)
        s_ = _spk(models["std"], torch.tensor([(4 * r + 1) % 109 for r in range(B)]))
        Lt = torch.tensor(L, dtype=torch.int32)
        cases[name] = (m_, z_, s_, Lt, 4, _ref(sds, esds, "std", m_, Lt, s_, z_, 4))
    bad, epochs, same = [], {}, []
    for name, (m_, z_, s_, Lt, n, ref) in cases.items():
        inp = tmp_path / f"{name}_in.pt"
        torch.save({"mu": m_.cpu(), "z0": z_.cpu(), "spk": s_.cpu(), "len": Lt, "n": n}, inp)
        default = None
        for extra in [{}] + SWITCHES[name]:
            tag = ",".join(f"{k}={v}" for k, v in extra.items())
            out = tmp_path / f"{name}_{len(epochs)}.pt"
            env = dict(os.environ)
            env.update(extra)
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-c", CHILD, str(inp), str(out)], env=env, capture_output=True, text=True, timeout=300)
            _CLOCK["children"] += time.perf_counter() - t0
            assert r.returncode == 0, (tag, r.stderr[-2000:])
            got = torch.load(out)
            epochs[f"{name} {tag or 'default'}"] = (got["epoch"], got["split"], len(got["sig"]))
            _check(f"switch {name} {tag or 'default'}", "std", got["dec"], ref, Lt, bad, z_.cpu())
            # the switch took another build: the profiled launches (kind, widths, taps, rows, tile config, epilogue, count) differ
            if default is None:
                default = got["sig"]
            elif got["sig"] == default:
                same.append(f"{name} {tag}")
    print(f"DECPATH switches (balanced launches, bf16-split / fp16 launches, profiled build kinds) per call {epochs}  "
          f"same builds as the default: {same}")
    assert not bad, bad
    # the profiled launches cannot tell these builds from the default (GroupNorm statistics, split-key attention and its tiles per wave,
    # the sk32 and lean epilogues are not among the profiled kinds): only their fp64 comparison above shows they compute the right thing
    assert same == PROFILE_BLIND, same
    assert epochs["b64 EV_NO_SK_BALANCE=1"][0] == 0 < epochs["b64 default"][0], epochs
    # ln_qkv_h16_kernel runs in the default build (six blocks a step); EV_NO_QKV_H16 takes it off, and with it the attn_out_h16_kernel
    # that reads its fp16 q / k / v pieces
    assert epochs["b64 default"][1] - epochs["b64 EV_NO_QKV_H16=1"][1] == 2 * 6 * N64, epochs


# ---------------------------------------------------------------------------------------------------------------------
# graph replay, and a handle that holds graphs serving other shapes in between
# ---------------------------------------------------------------------------------------------------------------------
def test_graph_replay_and_captured_handle(models, sds, esds):
    m = MatchaTTS(sds["std"], device=DEV)
    m.engine.reserve(2, 0, 396, 0)
    graphs = m.enable_decode_graphs()
    g = torch.Generator().manual_seed(396)

    def inputs(B, Tp, L):
        mu = torch.randn(B, 80, Tp, generator=g).to(DEV)
        z0 = (torch.randn(B, 80, Tp, generator=g) * 0.667).to(DEV)
        spk = _spk(m, torch.tensor([(7 * r + 18) % 109 for r in range(B)]))
        return mu, z0, spk, torch.tensor(L, dtype=torch.int32)

    n, bad = 4, []
    A, C, Bq = inputs(1, 396, [396]), inputs(2, 132, [132, 77]), inputs(1, 64, [64])
    ref = {k: _ref(sds, esds, "std", v[0], v[3], v[2], v[1], n) for k, v in (("A", A), ("C", C), ("B", Bq))}

    def graph_decode(tag, x):
        mu, z0, spk, L = x
        dec, mel = m.decode(mu, L.to(DEV), n, 1.0, spk, z=z0)
        torch.cuda.synchronize()
        _check(f"graphs {tag}", "std", dec, ref[tag[0]], L, bad, z0, mel, m)

    graph_decode("A 1x396 capture", A)
    graph_decode("C 2x132 capture", C)
    graph_decode("A 1x396 replay", A)
    graph_decode("C 2x132 replay", C)
    assert graphs.captures == 2 and graphs.hits == 2 and graphs.fallbacks == 0, (graphs.captures, graphs.hits, graphs.fallbacks)
    # eager B on the captured handle, replay A (its plan fills the arena), then one estimator call at B's shape
    mu, z0, spk, L = Bq
    dec, mel = m.engine.cfm_decode2(mu, L.to(DEV), spk, z0, n, m.mel_std, m.mel_mean)
    _check("graphs B 1x64 eager", "std", dec, ref["B"], L, bad, z0, mel, m)
    graph_decode("A 1x396 replay after B", A)
    t = 0.5
    v = m.engine.estimator(z0, mu, L.to(DEV), spk, t)
    torch.cuda.synchronize()
    vref = R.velocity(sds["std"], z0, mu, L, spk, t, device=DEV, esd=esds["std"]).cpu()
    _check("graphs estimator 1x64 after replay A", "std", v, vref, L, bad, gate=R.GATE_EST)
    fresh = models["std"].engine.estimator(z0, mu, L.to(DEV), spk, t)      # a handle that holds no graph
    torch.cuda.synchronize()
    assert not bad, bad
    assert torch.equal(v, fresh), float((v - fresh).abs().max())
