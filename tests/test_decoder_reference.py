"""The fp64 yardstick of tests/test_gpu_decoder.py, on the CPU: decoder_ref == the oracle (fp32, and fp64 with the oracle's fp32
sinusoid), fp64 decoder_ref against the reference-generated goldens, rows independent of each other, every masking trap and precision
slip either visible at 10x the GPU gate or pinned by equality, and the peaked-attention checkpoint peaking."""
import pytest
import torch

import decoder_ref as R
from oracle import matcha_oracle as O

T = torch.from_numpy


@pytest.fixture(scope="module")
def e64(matcha_sd):
    return R.estimator_state(matcha_sd)


def _g1(golden, matcha_sd):
    lengths = T(golden["g1_lengths"])
    return T(golden["g1_x"]), T(golden["g1_mu"]), lengths, matcha_sd["spk_emb.weight"][T(golden["g1_spk_ids"])]


def test_restatement_equals_the_oracle(golden, matcha_sd, monkeypatch):
    """In fp64, with the oracle's fp32 sinusoid, decoder_ref is the oracle's algorithm to 1e-12; in fp32 the two differ by fp32
    rounding of different operation orders (measured 3.5e-6 on the velocity, 2.3e-6 on dec)."""
    x, mu, lengths, spk = _g1(golden, matcha_sd)
    mask32 = O.sequence_mask(lengths, 32).unsqueeze(1).float()
    sd64 = {k: v.double() for k, v in matcha_sd.items()}
    z0 = T(golden["g2_z"]) * 0.667
    ts = (0.0, 0.37, 0.9)
    ref32 = [O.estimator(matcha_sd, x, mask32, mu, torch.tensor(t), spk) for t in ts]
    dec32 = O.solve_euler(matcha_sd, z0, mu, mask32, 4, spk)
    fp32_sin = O.sinusoidal_pos_emb
    monkeypatch.setattr(O, "sinusoidal_pos_emb", lambda t, dim: fp32_sin(t.float(), dim).double())
    for t, r32 in zip(ts, ref32):
        ref = O.estimator(sd64, x.double(), mask32.double(), mu.double(), torch.tensor(t), spk.double())
        got = R.velocity(matcha_sd, x, mu, lengths, spk, t)
        assert ref.dtype == torch.float64 and float((got - ref).abs().max()) <= 1e-12, t
        got32 = R.velocity(matcha_sd, x, mu, lengths, spk, t, torch.float32)
        assert float((got32 - r32).abs().max()) <= 1e-5, t
    ref = O.solve_euler(sd64, z0.double(), mu.double(), mask32.double(), 4, spk.double())
    assert float((R.decode(matcha_sd, mu, lengths, spk, z0, 4) - ref).abs().max()) <= 1e-12
    assert float((R.decode(matcha_sd, mu, lengths, spk, z0, 4, torch.float32) - dec32).abs().max()) <= 5e-6


def test_fp32_time_grid_and_sinusoid_are_the_oracles():
    """The two fp32 parts of the precision contract, bit for bit: solve_euler's running t / dt and sinusoidal_pos_emb."""
    for n in (2, 4, 10, 16):
        span = torch.linspace(0, 1, n + 1)
        t, dt = span[0], span[1] - span[0]
        for s, (tr, dtr) in enumerate(R.time_grid(n), start=1):
            assert tr.dtype == dtr.dtype == torch.float32
            assert torch.equal(tr, t) and torch.equal(dtr, dt), (n, s)
            t = t + dt
            if s < n:
                dt = span[s + 1] - t
        for tv, _ in R.time_grid(n):
            assert torch.equal(R.sinusoid(tv, 224), O.sinusoidal_pos_emb(tv, 224))


def test_restatement_against_the_goldens(golden, matcha_sd, e64):
    """fp64 decoder_ref against the reference's own fp32 run: within that run's fp32 error (measured 3.6e-6 on the velocity, 1.9e-6
    on dec; bounds 1e-5 and 5e-6)."""
    x, mu, lengths, spk = _g1(golden, matcha_sd)
    for i, tv in enumerate(golden["g1_t"]):
        v = R.velocity(matcha_sd, x, mu, lengths, spk, float(tv), esd=e64)
        assert float((v - T(golden[f"g1_v_t{i}"]).double()).abs().max()) <= 1e-5, i
    z0 = T(golden["g2_z"]) * 0.667
    for n in (2, 4, 10):
        d = R.decode(matcha_sd, mu, lengths, spk, z0, n, esd=e64)
        assert float((d - T(golden[f"g2_dec_n{n}"]).double()).abs().max()) <= 5e-6, n
    spk1 = matcha_sd["spk_emb.weight"][torch.tensor([58])]
    d = R.decode(matcha_sd, T(golden["g2b_mu"]), [24], spk1, T(golden["g2b_z"]) * 0.667, 10, esd=e64)
    assert float((d - T(golden["g2b_dec_n10"]).double()).abs().max()) <= 5e-6


def _ragged(matcha_sd, B=3, Tp=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    mu, z0 = torch.randn(B, 80, Tp, generator=g), torch.randn(B, 80, Tp, generator=g) * 0.667
    spk = matcha_sd["spk_emb.weight"][torch.tensor([107, 58, 12][:B])]
    return mu, z0, spk, torch.tensor([Tp, 41, 23][:B])


def test_rows_are_independent(matcha_sd, e64):
    """A row alone equals the same row inside a ragged batch; padded frames of dec keep the input state exactly (the velocity is
    exactly 0 there, as in the reference)."""
    mu, z0, spk, lengths = _ragged(matcha_sd)
    full = R.decode(matcha_sd, mu, lengths, spk, z0, 3, esd=e64)
    for r in range(3):
        one = R.decode(matcha_sd, mu[r:r + 1], lengths[r:r + 1], spk[r:r + 1], z0[r:r + 1], 3, esd=e64)
        assert float((one[0] - full[r]).abs().max()) <= 1e-12, r
        L = int(lengths[r])
        assert torch.equal(full[r, :, L:], z0[r, :, L:].double())


def _rel(d, ref, lengths):
    """Per row (RMS, L-inf) of d relative to the row's RMS of ref, over the valid frames."""
    out = []
    for r, L in enumerate(lengths.tolist()):
        rr = float(ref[r, :, :L].pow(2).mean().sqrt())
        out.append((float(d[r, :, :L].pow(2).mean().sqrt()) / rr, float(d[r, :, :L].abs().max()) / rr))
    return out


VISIBLE = ("gn_valid_only", "keys_neg_inf", "no_mask_before_conv", "qk_fp16")


def test_slips_are_visible(matcha_sd, e64):
    """Each plausible kernel slip moves some row of a ragged 10-step decode by at least 10x the GPU gate (RMS or L-inf).  The two
    fp64-for-fp32 slips of the precision contract stay below it (module docstring of decoder_ref): they are measured here and pinned by
    test_fp32_time_grid_and_sinusoid_are_the_oracles instead."""
    mu, z0, spk, lengths = _ragged(matcha_sd)
    base = R.decode(matcha_sd, mu, lengths, spk, z0, 10, esd=e64)
    seen = {}
    for slip in VISIBLE + ("sinusoid_fp64", "grid_fp64"):
        d = R.decode(matcha_sd, mu, lengths, spk, z0, 10, esd=e64, slips=(slip,)) - base
        rel = _rel(d, base, lengths)
        seen[slip] = max(max(rms / R.GATE[0], linf / R.GATE[1]) for rms, linf in rel)
    assert set(VISIBLE) | {"sinusoid_fp64", "grid_fp64", "score_scale"} == set(R.SLIPS)
    for slip in VISIBLE:
        assert seen[slip] >= 10, seen
    assert 0 < seen["sinusoid_fp64"] < 1 and 0 < seen["grid_fp64"] < 0.1, seen


def test_peaked_slips_are_visible():
    """On the peaked-attention weights, after the peaked cases' 2 Euler steps, q and k rounded once to fp16 and scores off by one bf16
    ulp of their scale (a mis-rounded static q / k scale) each move some row by at least 10x GATE_PEAKED; a plain fp32 evaluation of
    the same rows stays below a fifth of it."""
    sd = R.peaked_attention_state()
    esd = R.estimator_state(sd)
    mu, z0, spk, lengths = _ragged(sd)
    base = R.decode(sd, mu, lengths, spk, z0, R.PEAK_STEPS, esd=esd)
    seen = {}
    for slip in ("qk_fp16", "score_scale"):
        d = R.decode(sd, mu, lengths, spk, z0, R.PEAK_STEPS, esd=esd, slips=(slip,)) - base
        seen[slip] = max(max(rms / R.GATE_PEAKED[0], linf / R.GATE_PEAKED[1]) for rms, linf in _rel(d, base, lengths))
    d = R.decode(sd, mu, lengths, spk, z0, R.PEAK_STEPS, torch.float32).double() - base
    seen["fp32"] = max(max(rms / R.GATE_PEAKED[0], linf / R.GATE_PEAKED[1]) for rms, linf in _rel(d, base, lengths))
    assert seen["qk_fp16"] >= 10 and seen["score_scale"] >= 10 and seen["fp32"] < 0.2, seen


def test_peaked_checkpoint_peaks(matcha_sd):
    """Mean largest softmax weight: about 0.1 with the standard weights (near-uniform attention), above 0.7 with the peaked ones."""
    mu, z0, spk, lengths = _ragged(matcha_sd)
    peaks = {}
    for name, sd in (("std", matcha_sd), ("peak", R.peaked_attention_state())):
        R.PROBE = []
        try:
            R.decode(sd, mu, lengths, spk, z0, 1)
            peaks[name] = sum(R.PROBE) / len(R.PROBE)
        finally:
            R.PROBE = None
    peaked = R.peaked_attention_state()
    assert set(peaked) == set(matcha_sd)
    assert all(torch.equal(peaked[k], matcha_sd[k]) for k in matcha_sd if "attn1.to_q" not in k and "attn1.to_k" not in k)
    assert peaks["std"] < 0.2 and peaks["peak"] > 0.6 and peaks["peak"] > 4 * peaks["std"], peaks
