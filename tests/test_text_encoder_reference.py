"""The fp64 yardstick of tests/test_gpu_text_encoder.py, on the CPU: text_encoder_ref == the oracle in fp64 to 1e-12, within the
existing 1e-4 of the reference-generated golden, rows independent of their neighbours and of their padding, every slip visible at
10x the GPU gate, the peaked checkpoint peaking, the float32 reference error the gates are set from, and the duration band's caps.

Measured here (RMS / max over the valid tokens of one call, float32 oracle against fp64 text_encoder_ref; TEREF lines print with -s):
  standard checkpoint, worst over the case list, the single-speaker case and the golden: mu_x 8.1e-7 / 4.1e-6, logw 1.3e-6 / 3.3e-6
  peaked checkpoint (conv_q, conv_k x 3), worst over the case list:                     mu_x 1.9e-5 / 2.5e-4, logw 2.6e-5 / 1.9e-4
The peaked encoder amplifies float32 rounding through its six layers about 60-fold: that is the float32 reference's own behaviour,
so the two checkpoints have gates of their own (a gate pooled over both would be 7.6e-4 and let the standard checkpoint pass at the
old 1e-4 and beyond; each gate here is at most the pooled one).
"""
import pytest
import torch

import text_encoder_ref as R
from emojivoice_amd.matcha_tts import text_encoder_tensors
from oracle import matcha_oracle as O

T = torch.from_numpy


@pytest.fixture(scope="module")
def sds():
    return R.states()


@pytest.fixture(scope="module")
def refs(sds):
    """{(checkpoint, case name): (mu fp64, logw fp64, (rms, max) of the fp32 oracle's mu, of its logw)} over the whole case list."""
    out = {}
    for w, sd in sds.items():
        e64 = R.encoder_state(sd)
        for name, ids, L, sid in R.cases():
            spk = R.speaker_rows(sd, sid)
            mu, lw = R.encode(sd, ids, L, spk, esd=e64)
            fmu, flw, _ = O.text_encoder(sd, ids, L, spk)
            out[(w, name)] = (mu, lw, R.errors(fmu, mu, L), R.errors(flw, lw, L))
    return out


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_restatement_equals_the_oracle_in_fp64(sds):
    picked = {"edge 5", "edge 65", "edge 129", "zero-length row"}
    for w, sd in sds.items():
        sd64 = {k: v.double() for k, v in sd.items()}
        todo = [c for c in R.cases() if c[0] in picked]
        name, ids, L, sid = R.cases()[1]
        todo.append((name + " rows 0-11", ids[:12], L[:12], sid[:12]))
        for name, ids, L, sid in todo:
            spk = R.speaker_rows(sd, sid)
            mu, lw = R.encode(sd, ids, L, spk)
            omu, olw, _ = O.text_encoder(sd64, ids, L, spk.double())
            assert omu.dtype == torch.float64 and mu.shape == omu.shape and lw.shape == olw.shape
            assert _rel(mu, omu) <= 1e-12 and _rel(lw, olw) <= 1e-12, (w, name, _rel(mu, omu), _rel(lw, olw))
    sd1, ids, L = R.single_speaker_case()
    mu, lw = R.encode(sd1, ids, L, None)
    omu, olw, _ = O.text_encoder({k: v.double() for k, v in sd1.items()}, ids, L, None)
    assert _rel(mu, omu) <= 1e-12 and _rel(lw, olw) <= 1e-12


def test_rope_table_is_the_engines_and_fp32(matcha_sd):
    """theta as the loader hands it to the engine, and a float32 angle table, bit for bit the oracle's."""
    theta = text_encoder_tensors(matcha_sd)["rope_theta"]
    cos, sin = R.rope_table(37, 64)
    ang = torch.arange(37).float()[:, None] * theta[None, :]
    assert cos.dtype == torch.float32 and torch.equal(cos, ang.cos()) and torch.equal(sin, ang.sin())
    x = torch.randn(1, 1, 37, 128, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R._rope(x[0], 64), O._rope(x, 64)[0])


def _golden_inputs(golden, matcha_sd):
    ids, L = T(golden["g3_ids"]).long(), T(golden["g3_x_lengths"])
    return ids, L, matcha_sd["spk_emb.weight"][T(golden["g3_spks"]).long()]


def test_matches_the_golden(golden, matcha_sd):
    ids, L, spk = _golden_inputs(golden, matcha_sd)
    for dtype in (torch.float32, torch.float64):
        mu, lw = R.encode(matcha_sd, ids, L, spk, dtype)
        assert mu.dtype == dtype
        assert float((mu.double() - T(golden["g3_mu_x"]).double()).abs().max()) <= R.OLD_GATE
        assert float((lw.double() - T(golden["g3_logw"]).double()).abs().max()) <= R.OLD_GATE


def test_durations_and_alignment_restate_the_reference(golden, matcha_sd):
    """The rounding and the path against the golden synthesise runs (length scales 1.0 and 0.8), and against the oracle's
    generate_path / matmul at 1.37 and on a batch with a zero-length row."""
    ids, L, spk = _golden_inputs(golden, matcha_sd)
    mu_x, logw = T(golden["g3_mu_x"]), T(golden["g3_logw"])
    for tag, ls in (("a", 1.0), ("b", 0.8)):
        w_ceil, yl = R.mel_lengths(R.token_frames(logw, L), ls)
        assert torch.equal(yl, T(golden[f"g3{tag}_mel_lengths"]))
        Tp = R.padded_frames(int(yl.max()))
        attn = R.path(w_ceil, L, yl, Tp)
        assert list(attn.shape) == [2, 24, Tp] and int(golden[f"g3{tag}_attn_shape"][-1]) == Tp
        assert torch.equal(attn.sum(-1), T(golden[f"g3{tag}_attn_sum_text"])[:, 0])
        assert torch.equal(R.expand(attn, mu_x)[:, :, :int(yl.max())], T(golden[f"g3{tag}_enc"]))
    name, ids, L, sid = [c for c in R.cases() if c[0] == "zero-length row"][0]
    mu_x, logw = (t.float() for t in R.encode(matcha_sd, ids, L, R.speaker_rows(matcha_sd, sid)))
    for ls in R.LENGTH_SCALES:
        w_ceil, yl = R.mel_lengths(R.token_frames(logw, L), ls)
        x_mask = O.sequence_mask(L, ids.shape[1]).unsqueeze(1).float()
        ow = torch.ceil(torch.exp(logw) * x_mask) * ls
        oyl = torch.clamp_min(torch.sum(ow, [1, 2]), 1).long()
        assert torch.equal(w_ceil, ow[:, 0]) and torch.equal(yl, oyl) and int(yl[1]) == 1
        Tp = R.padded_frames(int(yl.max()))
        y_mask = O.sequence_mask(oyl, Tp).unsqueeze(1).float()
        oattn = O.generate_path(ow.squeeze(1), (x_mask.unsqueeze(-1) * y_mask.unsqueeze(2)).squeeze(1))
        attn = R.path(w_ceil, L, yl, Tp)
        assert torch.equal(attn, oattn)
        assert torch.equal(R.expand(attn, mu_x), torch.matmul(oattn.transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2))
        assert not bool(attn[1].any())


def test_rows_are_independent(sds):
    """A row's valid frames do not change with its neighbours, its padding ids (ids outside the vocabulary beyond the length
    included) or the padded Tx: to fp64 rounding of another summation blocking (1e-12)."""
    sd = sds["std"]
    e64 = R.encoder_state(sd)
    ids, sid = R.random_inputs(3, 70, 70)
    L = torch.tensor([70, 33, 1])
    spk = R.speaker_rows(sd, sid)
    mu, lw = R.encode(sd, ids, L, spk, esd=e64)
    for r, n in enumerate(L.tolist()):
        alone = R.encode(sd, ids[r:r + 1, :n], L[r:r + 1], spk[r:r + 1], esd=e64)          # no neighbours, no padding
        ids2 = torch.cat((ids[r:r + 1], torch.full((1, 31), 5)), dim=1)                   # a longer padded Tx
        ids2[0, n:] = torch.tensor([10**6, -3] * 60)[:ids2.shape[1] - n]                  # ids outside the vocabulary beyond the length
        padded = R.encode(sd, ids2, L[r:r + 1], spk[r:r + 1], esd=e64)
        others = R.encode(sd, torch.cat((ids[r:r + 1], ids.flip(1))), torch.cat((L[r:r + 1], L)), torch.cat((spk[r:r + 1], spk.flip(0))), esd=e64)
        for got in (alone, padded, others):
            assert float((got[0][0, :, :n] - mu[r, :, :n]).abs().max()) <= 1e-12
            assert float((got[1][0, :, :n] - lw[r, :, :n]).abs().max()) <= 1e-12
        assert not bool(padded[0][0, :, n:].any()) and not bool(padded[1][0, :, n:].any())
        assert not bool(mu[r, :, n:].any()) and not bool(lw[r, :, n:].any())


def test_peaked_checkpoint_peaks(sds):
    """In fp64 at Tx = 151 the median, over heads, layers and valid queries, of the largest softmax weight exceeds 0.5 (standard
    weights: near-flat attention)."""
    ids, sid = R.bench_inputs()
    L = R.bench_ragged_lengths()[:16]
    L[0] = R.TX_BENCH
    med = {}
    for w, sd in sds.items():
        R.PROBE = []
        try:
            R.encode(sd, ids[:16], L, R.speaker_rows(sd, sid[:16]))
            per_layer = [float(torch.cat(R.PROBE[2 * i:2 * i + 2]).median()) for i in range(R.N_LAYERS)]
            med[w] = float(torch.cat(R.PROBE).median())
        finally:
            R.PROBE = None
        print(f"TEREF largest softmax weight, median: {w} {med[w]:.3f}  per layer {[round(v, 3) for v in per_layer]}")
    assert med["peak"] > 0.5 > med["std"], med


def test_reference_error_is_what_the_gates_were_set_from(refs, golden, matcha_sd):
    """Re-measures REF_ERR (the float32 oracle and the golden against fp64 over the whole case list) and holds the committed constants
    to it: no measured value above 1.5x its constant (another BLAS blocking or thread count moves a maximum; the gate then still is 2x what was measured), no constant
    above twice its measured value; and the standard gates stay more than 5x under the old 1e-4."""
    worst = {w: {"mu": [0.0, 0.0], "logw": [0.0, 0.0]} for w in ("std", "peak")}

    def note(w, em, el, tag):
        print(f"TEREF {w:4s} {tag:18s} mu rms {em[0]:.2e} max {em[1]:.2e}   logw rms {el[0]:.2e} max {el[1]:.2e}")
        for k, e in (("mu", em), ("logw", el)):
            worst[w][k] = [max(worst[w][k][0], e[0]), max(worst[w][k][1], e[1])]

    for (w, name), (_, _, em, el) in refs.items():
        note(w, em, el, name)
    sd1, ids, L = R.single_speaker_case()
    mu, lw = R.encode(sd1, ids, L, None)
    fmu, flw, _ = O.text_encoder(sd1, ids, L, None)
    note("std", R.errors(fmu, mu, L), R.errors(flw, lw, L), "single speaker")
    ids, L, spk = _golden_inputs(golden, matcha_sd)
    mu, lw = R.encode(matcha_sd, ids, L, spk)
    note("std", R.errors(T(golden["g3_mu_x"]), mu, L), R.errors(T(golden["g3_logw"]), lw, L), "golden g3")
    print(f"TEREF worst {worst}")
    print(f"TEREF gates {R.GATE}")
    for w in worst:
        for k in ("mu", "logw"):
            for i in (0, 1):
                assert worst[w][k][i] <= 1.5 * R.REF_ERR[w][k][i] and R.REF_ERR[w][k][i] <= 2.0 * worst[w][k][i], (w, k, i, worst[w][k][i])
                assert R.GATE[w][k][i] == R.MARGIN * R.REF_ERR[w][k][i]
    assert max(R.GATE["std"]["mu"][1], R.GATE["std"]["logw"][1]) < R.OLD_GATE / 5


@pytest.mark.parametrize("slip", R.SLIPS)
def test_slips_are_visible(sds, refs, slip):
    """Each plausible kernel mistake moves mu_x or logw by at least 10x the checkpoint's gate (RMS or max over the valid tokens of a call) on some case."""
    small = [c for c in R.cases() if c[0] in ("edge 5", "edge 65", "edge 129", "edge 513", "long 2x1200", "zero-length row")]
    for w, sd in sds.items():
        e64 = R.encoder_state(sd)
        ratio = 0.0
        for name, ids, L, sid in small:
            mu, lw = R.encode(sd, ids, L, R.speaker_rows(sd, sid), esd=e64, slips=(slip,))
            em, el = R.errors(mu, refs[(w, name)][0], L), R.errors(lw, refs[(w, name)][1], L)
            ratio = max(ratio, *(e[i] / R.GATE[w][k][i] for k, e in (("mu", em), ("logw", el)) for i in (0, 1)))
        print(f"TEREF slip {slip:12s} {w:4s} moves the output by {ratio:.1f} gates")
        assert ratio >= 10.0, (slip, w, ratio)


def test_duration_exclusion_band_stays_inside_its_caps(refs):
    """Standard checkpoint, every case: the tokens whose fp64 exp(logw) lies within GATE logw (max) x exp(logw) of an integer, where a
    logw inside the gate may round the other way, are at most 0.2 % of the valid tokens, and at most 10 % of the utterances hold one.
    (The peaked checkpoint has no duration check: its float32 reference is off by 1.9e-4 on logw, a band that a fifth of all
    151-token utterances touch.)"""
    tokens = excluded = utts = utts_hit = 0
    for name, ids, L, sid in R.cases():
        near = R.near_integer(refs[("std", name)][1], L, R.GATE["std"]["logw"][1])
        tokens += int(L.sum())
        excluded += int(near.sum())
        utts += int((L > 0).sum())
        utts_hit += int(near.any(1).sum())
    print(f"TEREF exclusion band {R.GATE['std']['logw'][1]:.2e} x exp(logw): {excluded} of {tokens} tokens, {utts_hit} of {utts} utterances")
    assert excluded <= R.CAP_TOKENS * tokens and utts_hit <= R.CAP_UTTERANCES * utts
