"""Monotonic alignment search on the MI355X through the C ABI (ev_maximum_path, ev_log_prior, ev_mas_align) and the no-grad
MatchaTTS.forward / MatchaTTS.align on top of it, against tests/mas_ref.py.

The search is held EXACTLY: path and durations equal the float32 restatement (pinned to the reference's compiled loop by
tests/test_mas_host.py) bit for bit — one fp32 max and one fp32 add per cell leave no room for a tolerance.  ev_mas_align is compared
with the restatement fed the call's own d_logp, exact against exact, so a near-tie cannot flake.

Scores.  The reference's own arithmetic (its expanded form, two float32 matmuls on the CPU) was measured against the float64 yardstick
(the direct form) on exactly LOGP_CASES, max abs error per case:
    aligned  6.8e-6 (1,1,1)  4.0e-5 (1,1,37)  7.1e-5 (3,17,17)  8.5e-5 (3,50,129)  1.43e-4 (64,120,516)  1.01e-4 (1,400,1032)  1.00e-4 (2,1100,1200)
    noise    2.4e-6          2.8e-5           3.5e-5            4.4e-5             6.5e-5                4.8e-5                5.0e-5
(scores reach -480).  The engine is gated at 3x the worst figure, as the mel, decoder and vocoder modules gate:  GATE_LOGP = 4.3e-4.
The float32 reference is re-measured live (LOGPERR lines with -s) and must stay under 1.5x its recorded worst.
Engine, measured on one MI355X: ENGINE_LOGP_WORST (see the bottom of this docstring).

Losses of MatchaTTS.forward on the synthetic checkpoint (FORWARD_CASES), against the float64 helpers evaluated with the RETURNED attn
and the float64 encoder of tests/text_encoder_ref.py: dur_loss and prior_loss within a relative 1e-5 (the float32 host encoder through
the same formula: 9.8e-8 / 3.2e-9).  diff_loss against the same formula over tests/decoder_ref.velocity in float64: the reference's
evaluation in float32 on the CPU (y_t, u, the estimator and both reductions in float32) differs from it by a relative 8.4e-8 (B = 3)
and 1.7e-8 (B = 16); gate 3x the worst: GATE_DIFF = 2.5e-7, the float32 figure re-measured live under 1.5x.

Measured on one MI355X: not yet recorded.
Run time of this module: not yet recorded.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import decoder_ref as D
import mas_ref as R
import text_encoder_ref as TE
from emojivoice_amd import weights as W
from emojivoice_amd._lib import _stream_ptr
from emojivoice_amd.matcha_tts import MatchaTTS
from emojivoice_amd.text_encoder import generate_path, sequence_mask

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LOGP_WORST = 1.43e-4
GATE_LOGP = 3 * REF_LOGP_WORST
REF_DIFF_WORST = 8.4e-8
GATE_DIFF = 3 * REF_DIFF_WORST
GATE_LOSS = 1e-5
LOGP_CASES = [(kind, k) for k in range(len(R.SHAPES)) for kind in ("aligned", "noise")]


@pytest.fixture(scope="module")
def sd():
    return W.synthetic_matcha_state(178, 109)


@pytest.fixture(scope="module")
def model(sd):
    """The one engine of this process: the kernel-level tests use the model's handle."""
    return MatchaTTS(sd, device=DEV)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


def _search_equals_restatement(eng, value, xl, yl, tag):
    path, dur = eng.maximum_path(value.to(DEV), xl, yl)
    want, _ = R.maximum_path(value, xl, yl)
    assert path.dtype == torch.float32 and dur.dtype == torch.int32
    assert np.array_equal(path.cpu().numpy().astype(np.int8), want), tag
    assert np.array_equal(dur.cpu().numpy(), want.sum(-1, dtype=np.int64).astype(np.int32)), tag
    _, dur_only = eng.maximum_path(value.to(DEV), xl, yl, want_path=False)
    assert torch.equal(dur_only, dur), tag


def test_maximum_path_equals_the_golden_paths(eng):
    with np.load(os.path.join(REPO, "tests", "golden", "mas_vectors.npz")) as z:
        names = sorted(k[: -len("_value")] for k in z.files if k.endswith("_value"))
        assert len(names) >= 5
        for n in names:
            v, xl, yl = torch.from_numpy(z[f"{n}_value"]), torch.from_numpy(z[f"{n}_xlen"]), torch.from_numpy(z[f"{n}_ylen"])
            path, dur = eng.maximum_path(v.to(DEV), xl, yl)
            assert np.array_equal(path.cpu().numpy().astype(np.int8), z[f"{n}_path"]), n
            assert np.array_equal(dur.cpu().numpy(), z[f"{n}_path"].sum(-1, dtype=np.int64).astype(np.int32)), n


@pytest.mark.parametrize("B,Tx,Ty", R.SHAPES, ids=[f"B{b}-Tx{x}-Ty{y}" for b, x, y in R.SHAPES])
def test_maximum_path_is_bit_equal_on_random_scores(eng, B, Tx, Ty):
    xl, yl = R.ragged_lengths(B, Tx, Ty, seed=B + Tx + Ty)
    value = R.random_scores(B, Tx, Ty, seed=7 * B + Tx)
    v0 = value.clone()
    _search_equals_restatement(eng, value, xl, yl, "random")
    assert torch.equal(value, v0)
    if B * Tx * Ty <= 3 * 50 * 129 or (B, Tx, Ty) == (1, 400, 1032):
        _search_equals_restatement(eng, torch.full((B, Tx, Ty), -0.75), xl, yl, "ties everywhere")
        _search_equals_restatement(eng, R.random_scores(B, Tx, Ty, seed=11, scale=1e6), xl, yl, "magnitude 1e6")
        grid = torch.randint(-2, 3, (B, Tx, Ty), generator=torch.Generator().manual_seed(5)).float()
        _search_equals_restatement(eng, grid, xl, yl, "integer grid: many exact ties")


def test_maximum_path_input_is_not_modified_and_large_magnitudes_at_the_bench_shape(eng):
    B, Tx, Ty = 64, 120, 516
    xl, yl = R.ragged_lengths(B, Tx, Ty, seed=3)
    _search_equals_restatement(eng, R.random_scores(B, Tx, Ty, seed=12, scale=1e6), xl, yl, "1e6 at the bench shape")
    _search_equals_restatement(eng, torch.zeros(B, Tx, Ty), xl, yl, "all equal at the bench shape")


@pytest.mark.parametrize("kind,k", LOGP_CASES, ids=[f"{kind}-B{R.SHAPES[k][0]}-Tx{R.SHAPES[k][1]}-Ty{R.SHAPES[k][2]}" for kind, k in LOGP_CASES])
def test_log_prior_and_the_fused_search_against_fp64(eng, kind, k):
    B, Tx, Ty = R.SHAPES[k]
    mu_x, y, xl, yl = R.mel_pairs(kind, B, Tx, Ty, seed=1000 + 10 * k + (kind == "noise"))
    ref = R.log_prior_fp64_chunked(mu_x, y)
    e_ref = float((R.log_prior(mu_x, y, torch.float32).double() - ref).abs().max())
    print(f"\nLOGPERR {kind} {(B, Tx, Ty)}: float32 reference max {e_ref:.2e}")
    assert e_ref <= 1.5 * REF_LOGP_WORST, "the float32 reference moved: the gate constant is stale"
    logp = eng.log_prior(mu_x.to(DEV), y.to(DEV))
    e = float((logp.cpu().double() - ref).abs().max())
    print(f"LOGPERR {kind} {(B, Tx, Ty)}: ev_log_prior max {e:.2e}  gate {GATE_LOGP:.2e}")
    assert tuple(logp.shape) == (B, Tx, Ty) and e <= GATE_LOGP
    r = eng.mas_align(mu_x.to(DEV), y.to(DEV), xl, yl, want_logp=True)
    e2 = float((r["logp"].cpu().double() - ref).abs().max())
    print(f"LOGPERR {kind} {(B, Tx, Ty)}: ev_mas_align d_logp max {e2:.2e}")
    assert e2 <= GATE_LOGP
    assert torch.equal(r["logp"], logp), "the fused call and ev_log_prior form every cell with the same fmaf chain"
    # exact against exact: the restatement on the call's own scores
    want, _ = R.maximum_path(r["logp"].cpu(), xl, yl)
    assert np.array_equal(r["attn"].cpu().numpy().astype(np.int8), want)
    assert np.array_equal(r["dur"].cpu().numpy(), want.sum(-1, dtype=np.int64).astype(np.int32))
    R.check_structure(r["attn"], xl, yl, r["dur"])
    # the same with other outputs requested
    r2 = eng.mas_align(mu_x.to(DEV), y.to(DEV), xl, yl, want_attn=False, want_mu_y=False)
    r3 = eng.mas_align(mu_x.to(DEV), y.to(DEV), xl, yl, want_dur=False)
    assert r2["attn"] is None and r2["mu_y"] is None and r2["logp"] is None and torch.equal(r2["dur"], r["dur"])
    assert torch.equal(r3["attn"], r["attn"]) and torch.equal(r3["mu_y"], r["mu_y"])
    p2, d2 = eng.maximum_path(logp, xl, yl)
    assert torch.equal(p2, r["attn"]) and torch.equal(d2, r["dur"]), "the two-call route gives the fused call's result"
    # mu_y is the gather
    tok = torch.from_numpy(want.astype(np.int64)).argmax(1)                                    # (B, Ty)
    g = torch.gather(mu_x, 2, tok.unsqueeze(1).expand(-1, 80, -1)) * (torch.arange(Ty)[None, None, :] < yl[:, None, None])
    assert torch.equal(r["mu_y"].cpu(), g.float())
    if kind == "aligned" and 1 < Tx < Ty:
        assert float((r["dur"].cpu()[0].float() - 1).abs().sum()) > 0                           # not the trivial path


def test_bad_rows_are_zero_and_nothing_outside_is_written(eng):
    B, Tx, Ty, M = 5, 19, 44, 4096
    mu_x, y, xl, yl = R.mel_pairs("aligned", B, Tx, Ty, seed=77)
    xl_bad, yl_bad = xl.clone(), yl.clone()
    xl_bad[1], yl_bad[1] = 12, 7                     # xlen > ylen
    xl_bad[3] = 0                                    # xlen = 0
    lib, h = eng.lib, eng.h
    mu_d, y_d = mu_x.to(DEV), y.to(DEV)

    def guarded(n, dtype):
        t = torch.full((n + 2 * M,), -7, dtype=dtype, device=DEV)
        return t, t[M:M + n]

    def call(xl_, yl_):
        bufs = {k: guarded(n, dt) for k, n, dt in (("attn", B * Tx * Ty, torch.float32), ("dur", B * Tx, torch.int32),
                                                   ("mu_y", B * 80 * Ty, torch.float32), ("logp", B * Tx * Ty, torch.float32))}
        xd, yd = xl_.to(DEV, torch.int32), yl_.to(DEV, torch.int32)
        rc = lib.ev_mas_align(h, mu_d.data_ptr(), y_d.data_ptr(), xd.data_ptr(), yd.data_ptr(), B, Tx, Ty, bufs["attn"][1].data_ptr(),
                              bufs["dur"][1].data_ptr(), bufs["mu_y"][1].data_ptr(), bufs["logp"][1].data_ptr(), _stream_ptr())
        assert rc == 0
        pbuf, dbuf = guarded(B * Tx * Ty, torch.float32), guarded(B * Tx, torch.int32)
        rc = lib.ev_maximum_path(h, bufs["logp"][1].data_ptr(), xd.data_ptr(), yd.data_ptr(), B, Tx, Ty, pbuf[1].data_ptr(), dbuf[1].data_ptr(), _stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        for full, inner in list(bufs.values()) + [pbuf, dbuf]:
            assert bool((full[:M] == -7).all()) and bool((full[M + inner.numel():] == -7).all()), "a margin was written"
        out = {k: v[1].clone() for k, v in bufs.items()}
        assert torch.equal(pbuf[1], out["attn"]) and torch.equal(dbuf[1], out["dur"])
        return (out["attn"].view(B, Tx, Ty), out["dur"].view(B, Tx), out["mu_y"].view(B, 80, Ty), out["logp"].view(B, Tx, Ty))

    good = call(xl, yl)
    bad = call(xl_bad, yl_bad)
    for b in range(B):
        if b in (1, 3):
            assert float(bad[0][b].abs().sum()) == 0 and int(bad[1][b].abs().sum()) == 0 and float(bad[2][b].abs().sum()) == 0
        else:
            for g_, b_ in zip(good, bad):
                assert torch.equal(g_[b], b_[b]), b
    assert torch.equal(good[3], bad[3]), "the scores do not depend on the lengths"
    R.check_structure(good[0], xl, yl, good[1])
    with pytest.raises(Exception, match="bad arguments"):
        eng.maximum_path(torch.zeros(1, 5000, 2, device=DEV), torch.tensor([1]), torch.tensor([2]))


def test_the_search_only_enqueues(eng):
    for (B, Tx, Ty) in ((8, 60, 200), (2, 1100, 1200)):                 # decision bits in LDS / in the handle's scratch
        mu_x, y, xl, yl = R.mel_pairs("noise", B, Tx, Ty, seed=5)
        a = eng.mas_align(mu_x.to(DEV), y.to(DEV), xl, yl)
        torch.cuda.synchronize()
        n0 = eng.alloc_count()
        b = eng.mas_align(mu_x.to(DEV), y.to(DEV), xl, yl)
        eng.maximum_path(eng.log_prior(mu_x.to(DEV), y.to(DEV)), xl, yl)
        torch.cuda.synchronize()
        assert eng.alloc_count() == n0
        assert torch.equal(a["attn"], b["attn"]) and torch.equal(a["dur"], b["dur"])


def _forward_case(sd, name):
    B, Tx, Ty, seed = R.FORWARD_CASES[name]
    ids, xl, spks, yl, t, z = R.forward_texts(B, Tx, Ty, seed)
    spk = TE.speaker_rows(sd, spks)
    mu64, logw64 = TE.encode(sd, ids, xl, spk)
    _, y, _, _ = R.mel_pairs("aligned", B, Tx, Ty, seed + 2, mu_x=mu64.float(), x_lengths=xl, y_lengths=yl)
    return ids, xl, spks, spk, yl, t, z, y, mu64, logw64


def _check_losses(sd, case, out, tag):
    ids, xl, spks, spk, yl, t, z, y, mu64, logw64 = case
    dur_loss, prior_loss, diff_loss, attn = out
    assert tuple(attn.shape) == (ids.shape[0], ids.shape[1], y.shape[-1])
    R.check_structure(attn, xl, yl)
    d64, p64, mu_y = R.dur_and_prior_loss(attn, logw64, mu64, y, xl, yl)
    e_d, e_p = abs(float(dur_loss) - d64) / d64, abs(float(prior_loss) - p64) / p64
    y_t, u = R.cfm_inputs(y, t, z)
    v64 = R.velocity_padded(D.velocity, sd, y_t, mu_y.float(), yl, spk, t, torch.float64)
    l64 = R.diff_loss_from_velocity(v64, u, yl)
    e_ref = R.diff_loss_fp32_oracle(D.velocity, sd, y, mu_y, yl, spk, t, z, l64)
    e_l = abs(float(diff_loss) - l64) / l64
    print(f"\nLOSSERR {tag}: dur {float(dur_loss):.6f} rel {e_d:.2e}  prior {float(prior_loss):.6f} rel {e_p:.2e}  (gate {GATE_LOSS:.0e});  "
          f"diff {float(diff_loss):.6f} rel {e_l:.2e}  float32 oracle rel {e_ref:.2e}  gate {GATE_DIFF:.2e}")
    assert e_ref <= 1.5 * REF_DIFF_WORST, "the float32 oracle moved: the gate constant is stale"
    assert e_d <= GATE_LOSS and e_p <= GATE_LOSS
    assert e_l <= GATE_DIFF


@pytest.mark.parametrize("name", list(R.FORWARD_CASES))
def test_forward_losses_against_fp64(sd, model, name):
    case = _forward_case(sd, name)
    ids, xl, spks, spk, yl, t, z, y, mu64, logw64 = case
    out = model.forward(ids, xl, y, yl, spks, t=t, z=z)
    assert len(out) == 4 and all(o.dtype == torch.float32 for o in out)
    _check_losses(sd, case, out, f"{name} device encoder")
    again = model(ids, xl, y, yl, spks=spks, t=t, z=z)
    assert torch.equal(again[3], out[3]) and all(float(a) == float(b) for a, b in zip(again[:3], out[:3]))
    drawn = model.forward(ids, xl, y, yl, spks)                      # t and z drawn inside
    assert torch.equal(drawn[3], out[3]) and float(drawn[0]) == float(out[0]) and float(drawn[1]) == float(out[1])
    assert torch.isfinite(drawn[2]) and float(drawn[2]) > 0
    # MatchaTTS.align: the durations script
    al = model.align(ids, xl, y, yl, spks)
    assert al["durations"].dtype == torch.int64 and torch.equal(al["durations"], out[3].sum(-1).long())
    assert torch.equal(al["attn"], out[3]) and tuple(al["mu_y"].shape) == (ids.shape[0], 80, y.shape[-1])
    x_mask = sequence_mask(xl, ids.shape[1]).unsqueeze(1).float()
    assert torch.equal(al["logw_"], torch.log(1e-8 + out[3].sum(-1)).unsqueeze(1) * x_mask.to(DEV))       # the same op on the same device
    want = torch.log(1e-8 + out[3].sum(-1).cpu().double()).unsqueeze(1) * x_mask.double()
    assert float((al["logw_"].cpu().double() - want).abs().max()) <= 1e-6                                   # a few float32 ulps of log(frames)
    model.encoder_stage = "host"
    try:
        _check_losses(sd, case, model.forward(ids, xl, y, yl, spks, t=t, z=z), f"{name} host encoder")
    finally:
        model.encoder_stage = "device"


def test_forward_with_durations_errors_and_out_size(sd, model):
    case = _forward_case(sd, "B3 ragged")
    ids, xl, spks, spk, yl, t, z, y, mu64, logw64 = case
    attn = model.forward(ids, xl, y, yl, spks, t=t, z=z)[3]
    durs = attn.sum(-1)
    out = model.forward(ids, xl, y, yl, spks, durations=durs.unsqueeze(1), t=t, z=z)
    mask = (sequence_mask(xl, ids.shape[1]).unsqueeze(-1) & sequence_mask(yl, y.shape[-1]).unsqueeze(1)).float()
    assert torch.equal(out[3].cpu(), generate_path(durs.cpu(), mask))
    assert torch.equal(out[3], attn), "durations taken from a path give that path back"
    _check_losses(sd, case, out, "precomputed durations")
    with pytest.raises(NotImplementedError, match="out_size"):
        model.forward(ids, xl, y, yl, spks, out_size=32)
    for bad_x, bad_y in ((yl + 1, yl), (torch.zeros_like(xl), yl), (xl, torch.zeros_like(yl))):
        with pytest.raises(ValueError, match="x_lengths"):
            model.forward(ids, bad_x.clamp(max=ids.shape[1] + 5), y, bad_y, spks)
        with pytest.raises(ValueError, match="x_lengths"):
            model.align(ids, bad_x.clamp(max=ids.shape[1] + 5), y, bad_y, spks)


def test_round_trip_of_the_analysis_side(model):
    g = torch.Generator().manual_seed(9)
    B, Tx = 4, 30
    ids = torch.randint(1, 178, (B, Tx), generator=g)
    xl = torch.tensor([30, 11, 23, 1])
    spks = torch.randint(0, 109, (B,), generator=g)
    syn = model.synthesise(ids.to(DEV), xl.to(DEV), 2, 0.667, spks.to(DEV))
    yl = syn["mel_lengths"]
    y = syn["decoder_outputs"][:, :, : int(yl.max())] * sequence_mask(yl, int(yl.max())).unsqueeze(1)
    al = model.align(ids, xl, y, yl, spks)
    assert torch.equal(al["durations"].sum(1), yl.long())
    R.check_structure(al["attn"], xl, yl.cpu(), al["durations"])


def test_cli_align_mel(model, tmp_path):
    from emojivoice_amd.cli import cli

    g = torch.Generator().manual_seed(2)
    mel = torch.randn(80, 57, generator=g).numpy().astype(np.float32)
    p = tmp_path / "utt.mel.npy"
    np.save(p, mel)
    ids = "0 23 0 51 0 7 0 99 0"
    cli(["--synthetic", "--align_mel", str(p), "--ids", ids, "--spk", "3"])
    dur = np.load(f"{p}.durations.npy")
    assert dur.shape == (9,) and dur.sum() == 57 and (dur >= 1).all() and np.issubdtype(dur.dtype, np.integer)
