"""The batched flow-matching loss on the MI355X: ev_estimator_rows (one time per utterance inside the U-Net), ev_cfm_loss (mix kernel,
estimator, loss kernel in one call) and MatchaTTS.forward(batched=True) / MatchaTTS.score / the CLI's --losses on top of them, against
the float64 restatements of tests/decoder_ref.py, tests/mas_ref.py and tests/text_encoder_ref.py.  Weights: the synthetic checkpoint
of tests/test_gpu_mas.py.

Velocity.  ev_estimator_rows against decoder_ref.velocity in float64, row by row at the row's own time, at the smallest shapes that
take each path: (B, Tp) = (1, 4) the one-utterance GroupNorm (groupnorm_apply_kernel), (3, 40) ragged 37 / 20 / 5 the 1024-thread
groupnorm_mish_kernel, (32, 8) the 512-thread one, (65, 4) more rows than the 64 planned time slots.  Times are distinct per row and
include 0 and 0.9995.  Gate: the project's own for one estimator call (decoder_ref.GATE_EST, tests/test_gpu_decoder.py): per row over
its valid frames, RMS <= 7e-6 and L-inf <= 3.5e-5 of the row's float64 RMS.  The scalar ev_estimator at a uniform t is printed against
float64 at every shape beside it (ESTERR lines with -s); a uniform-t ev_estimator_rows call must be within the gate of it (bit-equality
is printed, not required: the time MLP may take another build at B rows than at one); at (3, 40) giving every row the time of row 0
must move row 1 by more than 100x the gate, so the comparison does see which row got which time.

Losses.  forward(batched=True), forward(batched=False) and score on mas_ref.FORWARD_CASES plus "B5 Ty37" (B = 5, Tx = 9, Ty = 37: not
a multiple of 4, one row with xlen = ylen = 1), against the float64 formulas evaluated with the RETURNED attn.  dur_loss and prior_loss
within a relative 1e-5, batch value and every row.  diff_loss by the convention of tests/test_gpu_mas.py: the reference's own float32
evaluation on the CPU (mas_ref.diff_loss_fp32_oracle; per row the same float32 evaluation over the row's valid cells) was measured
against the float64 formula on exactly these cases:
    batch value   8.4e-8 (B3 ragged)   1.7e-8 (B16)   3.7e-9 (B5 Ty37)      worst 8.4e-8  ->  GATE_DIFF     = 3 x = 2.5e-7
    worst row     1.0e-7               2.2e-7         1.4e-7                worst 2.2e-7  ->  GATE_DIFF_ROW = 3 x = 6.5e-7
Both are re-measured live (LOSSERR lines with -s) and must stay under 1.5x the recorded figure.  The batch value of the reference
counts the padded frames of shorter rows too (the estimator is 0 there, u is not: mas_ref.diff_loss_from_velocity); a row's value is
over its own ylen x 80 cells.

Measured on one MI355X: see CFMWORST at the end of a run with -s.
"""
import ctypes as C
import json
import math
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

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE_EST = D.GATE_EST
GATE_LOSS = 1e-5
REF_DIFF_WORST, REF_DIFF_ROW_WORST = 8.4e-8, 2.2e-7
GATE_DIFF, GATE_DIFF_ROW = 3 * REF_DIFF_WORST, 3 * REF_DIFF_ROW_WORST
EST_SHAPES = [(1, 4), (3, 40), (32, 8), (65, 4)]
CASES = dict(R.FORWARD_CASES)
CASES["B5 Ty37"] = (5, 9, 37, 33)
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nCFMWORST " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(_WORST.items())))


def _note(key, v):
    _WORST[key] = max(_WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def sd():
    return W.synthetic_matcha_state(178, 109)


@pytest.fixture(scope="module")
def model(sd):
    return MatchaTTS(sd, device=DEV)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def esd(sd):
    return D.estimator_state(sd, torch.float64, DEV)


# ---------------------------------------------------------------------------------------------------------------------
# the velocity with one time per row
# ---------------------------------------------------------------------------------------------------------------------
def _lengths(B, Tp):
    if (B, Tp) == (3, 40):
        return torch.tensor([37, 20, 5], dtype=torch.int32)
    return torch.tensor([Tp] + [(i % Tp) + 1 for i in range(1, B)], dtype=torch.int32)


def _est_inputs(sd, B, Tp):
    g = torch.Generator().manual_seed(100 * B + Tp)
    x = torch.randn(B, 80, Tp, generator=g) * 0.667
    mu = torch.randn(B, 80, Tp, generator=g)
    spk = TE.speaker_rows(sd, torch.randint(0, 109, (B,), generator=g))
    t = torch.linspace(0.05, 0.95, B) if B > 1 else torch.tensor([0.9995])
    t[0] = 0.0 if B > 1 else t[0]
    t[-1] = 0.9995
    return x.to(DEV), mu.to(DEV), spk.to(DEV), _lengths(B, Tp), t.float()


def _ref_rows(sd, esd, x, mu, L, spk, t):
    """decoder_ref.velocity in float64, each row at its own time (rows are independent: tests/test_decoder_reference.py)."""
    rows = [D.velocity(sd, x[b:b + 1], mu[b:b + 1], L[b:b + 1], spk[b:b + 1], float(t[b]), device=DEV, esd=esd) for b in range(x.shape[0])]
    return torch.cat(rows).cpu()


def _rel_err(got, ref, L):
    """Worst over the rows of (RMS, L-inf) of got - ref over the row's valid frames, relative to the RMS of ref there."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    w = [0.0, 0.0]
    for b, n in enumerate(L.tolist()):
        e, rr = got[b, :, :n] - ref[b, :, :n], float(ref[b, :, :n].pow(2).mean().sqrt())
        assert rr > 0
        w = [max(w[0], float(e.pow(2).mean().sqrt()) / rr), max(w[1], float(e.abs().max()) / rr)]
    return w


def _within(e, gate=GATE_EST):
    return e[0] <= gate[0] and e[1] <= gate[1]


@pytest.mark.parametrize("B,Tp", EST_SHAPES, ids=[f"B{b}-Tp{t}" for b, t in EST_SHAPES])
def test_estimator_rows_against_fp64(sd, eng, esd, B, Tp):
    x, mu, spk, L, t = _est_inputs(sd, B, Tp)
    Ld = L.to(DEV)
    times = [t] if B > 1 else [t, torch.tensor([0.0])]          # one row: both ends of the time range, one after the other
    for tt in times:
        ref = _ref_rows(sd, esd, x, mu, L, spk, tt)
        v = eng.estimator_rows(x, mu, Ld, spk, tt)
        torch.cuda.synchronize()
        e = _rel_err(v, ref, L)
        print(f"\nESTERR rows   ({B}, {Tp}) t {float(tt[0]):.4f}..{float(tt[-1]):.4f}: rel rms {e[0]:.2e} linf {e[1]:.2e}  gate {GATE_EST[0]:.1e} / {GATE_EST[1]:.1e}")
        _note("est_rows_rms", e[0]); _note("est_rows_linf", e[1])
        assert bool(torch.isfinite(v).all()) and _within(e), (B, Tp, e)
        for b, n in enumerate(L.tolist()):
            assert not bool((v[b, :, n:] != 0).any()), "the velocity is exactly 0 on padded frames"
        again = eng.estimator_rows(x, mu, Ld, spk, tt)
        assert torch.equal(again, v), "two calls on the same inputs give the same bits"
    # uniform t: the scalar call against float64 (printed), and the per-row call against the scalar call
    tu = torch.full((B,), 0.5)
    ref_u = _ref_rows(sd, esd, x, mu, L, spk, tu)
    v_s = eng.estimator(x, mu, Ld, spk, 0.5)
    v_r = eng.estimator_rows(x, mu, Ld, spk, tu)
    torch.cuda.synchronize()
    e_s, e_r, e_sr = _rel_err(v_s, ref_u, L), _rel_err(v_r, ref_u, L), _rel_err(v_r, v_s, L)
    print(f"ESTERR scalar ({B}, {Tp}) t 0.5: rel rms {e_s[0]:.2e} linf {e_s[1]:.2e};  rows at uniform t: {e_r[0]:.2e} / {e_r[1]:.2e};  "
          f"rows vs scalar {e_sr[0]:.2e} / {e_sr[1]:.2e}  bit-equal {torch.equal(v_r, v_s)}")
    assert _within(e_r) and _within(e_sr), (e_r, e_sr)


def test_each_row_gets_its_own_time(sd, eng, esd):
    B, Tp = 3, 40
    x, mu, spk, L, t = _est_inputs(sd, B, Tp)
    assert float(t[0]) == 0.0 and 0.4 < float(t[1]) < 0.6
    v = eng.estimator_rows(x, mu, L.to(DEV), spk, t)
    v0 = eng.estimator_rows(x, mu, L.to(DEV), spk, torch.full((B,), float(t[0])))
    one = slice(1, 2)
    moved = _rel_err(v0[one], v[one], L[one])
    print(f"\nESTERR row 1 at row 0's time differs by rel rms {moved[0]:.2e} (100 x gate = {100 * GATE_EST[0]:.1e})")
    assert moved[0] >= 100 * GATE_EST[0] and moved[1] >= 100 * GATE_EST[1]
    assert torch.equal(v0[0], v[0]), "row 0 has the same time in both calls and does not see the others'"
    ref1 = D.velocity(sd, x[one], mu[one], L[one], spk[one], float(t[1]), device=DEV, esd=esd).cpu()
    assert _within(_rel_err(v[one], ref1, L[one]))


def test_more_rows_than_time_slots_grow_the_plan_once_and_repeat_calls_allocate_nothing(sd):
    fresh = MatchaTTS(sd, device=DEV).engine                      # its own handle: the plan still has its 64 time slots
    x, mu, spk, L, t = _est_inputs(sd, 3, 40)
    a = fresh.estimator_rows(x, mu, L.to(DEV), spk, t)
    n0 = fresh.alloc_count()
    assert torch.equal(fresh.estimator_rows(x, mu, L.to(DEV), spk, t), a) and fresh.alloc_count() == n0
    x, mu, spk, L, t = _est_inputs(sd, 65, 4)
    b = fresh.estimator_rows(x, mu, L.to(DEV), spk, t)
    n1 = fresh.alloc_count()
    print(f"\nALLOC (65, 4) after (3, 40): ev_alloc_count moved by {n1 - n0}")
    assert 0 <= n1 - n0 <= 1
    assert torch.equal(fresh.estimator_rows(x, mu, L.to(DEV), spk, t), b) and fresh.alloc_count() == n1
    # ev_cfm_loss at 65 rows on the same handle: the time plan is there
    g = torch.Generator().manual_seed(1)
    z = torch.randn(65, 80, 4, generator=g).to(DEV)
    s1, v1 = fresh.cfm_loss(x, mu, L.to(DEV), spk, z, t, 1e-4, want_v=True)
    n2 = fresh.alloc_count()
    s2, v2 = fresh.cfm_loss(x, mu, L.to(DEV), spk, z, t, 1e-4, want_v=True)
    torch.cuda.synchronize()
    assert fresh.alloc_count() == n2 and n2 == n1
    assert torch.equal(s1, s2) and torch.equal(v1, v2), "float64 sums and velocity: the same bits from two calls"
    assert bool(torch.isfinite(s1).all()) and bool((s1 > 0).all())
    fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# ev_cfm_loss: padding, skipped rows, nothing written outside
# ---------------------------------------------------------------------------------------------------------------------
def test_cfm_loss_padding_bad_rows_and_margins(sd, eng, esd):
    B, Ty, M = 3, 37, 4096
    g = torch.Generator().manual_seed(21)
    x1, mu_y, z = (torch.randn(B, 80, Ty, generator=g).to(DEV) for _ in range(3))
    spk = TE.speaker_rows(sd, torch.tensor([5, 77, 101])).to(DEV)
    t = torch.tensor([0.0, 0.37, 0.9995])
    good, bad = torch.tensor([37, 30, 12], dtype=torch.int32), torch.tensor([0, 30, Ty + 1], dtype=torch.int32)

    def call(yl):
        buf = torch.full((B * 80 * Ty + 2 * M,), -7.0, device=DEV)
        sums = torch.full((2 * B + 2 * M,), -7.0, dtype=torch.float64, device=DEV)
        yd, tv = yl.to(DEV), np.ascontiguousarray(t.numpy())
        rc = eng.lib.ev_cfm_loss(eng.h, x1.data_ptr(), mu_y.data_ptr(), yd.data_ptr(), spk.data_ptr(), z.data_ptr(), tv.ctypes.data_as(C.c_void_p), B, Ty,
                                 1e-4, sums[M:].data_ptr(), buf[M:].data_ptr(), _stream_ptr())
        assert rc == 0, eng.lib.ev_last_error(eng.h)
        torch.cuda.synchronize()
        for full, n in ((buf, B * 80 * Ty), (sums, 2 * B)):
            assert bool((full[:M] == -7).all()) and bool((full[M + n:] == -7).all()), "a margin was written"
        return sums[M:M + 2 * B].view(B, 2).clone(), buf[M:M + B * 80 * Ty].view(B, 80, Ty).clone()

    s_good, v_good = call(good)
    s_bad, v_bad = call(bad)
    assert bool(torch.isfinite(v_good).all()) and bool(torch.isfinite(v_bad).all())
    for b in (0, 2):
        assert float(s_bad[b].abs().sum()) == 0 and float(v_bad[b].abs().sum()) == 0, "a skipped row is zeros"
    one = slice(1, 2)
    e_v = _rel_err(v_bad[one], v_good[one], good[one])
    e_s = float(((s_bad[1] - s_good[1]).abs() / s_good[1]).max())
    print(f"\nLOSSERR valid row beside skipped rows: velocity rel {e_v[0]:.2e} / {e_v[1]:.2e}  sums rel {e_s:.2e}  bit-equal {torch.equal(v_bad[1], v_good[1])}")
    assert _within(e_v) and e_s <= GATE_DIFF_ROW
    # d_v is (B, 80, 37): the velocity of the padded call (Tp = 40) cut back, and zeros past each row's length
    y_t, u = R.cfm_inputs(x1, t.to(DEV), z)
    pad = torch.nn.functional.pad
    v_rows = eng.estimator_rows(pad(y_t, (0, 3)), pad(mu_y, (0, 3)), good.to(DEV), spk, t)
    assert float(v_rows[:, :, Ty:].abs().sum()) == 0
    e = _rel_err(v_good, v_rows[:, :, :Ty], good)
    print(f"LOSSERR d_v against ev_estimator_rows on torch's y_t: rel {e[0]:.2e} / {e[1]:.2e}  bit-equal {torch.equal(v_good, v_rows[:, :, :Ty])}")
    assert _within(e)
    for b, n in enumerate(good.tolist()):
        assert float(v_good[b, :, n:].abs().sum()) == 0
    # the sums are those of the float64 formula over each row's valid cells, the velocity in float64
    v64 = _ref_rows(sd, esd, pad(y_t, (0, 3)), pad(mu_y, (0, 3)), good, spk, t)[:, :, :Ty]
    for b, n in enumerate(good.tolist()):
        want_d = float(((v64[b, :, :n] - u[b, :, :n].double().cpu()) ** 2).sum())
        want_p = float((0.5 * ((x1[b, :, :n] - mu_y[b, :, :n]).double() ** 2 + math.log(2 * math.pi))).sum())
        e_d, e_p = abs(float(s_good[b, 0]) - want_d) / want_d, abs(float(s_good[b, 1]) - want_p) / want_p
        print(f"LOSSERR row {b} ({n} frames): sum d^2 rel {e_d:.2e}  prior sum rel {e_p:.2e}")
        _note("sum_d2_row", e_d)
        assert e_d <= GATE_DIFF_ROW and e_p <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the losses against float64
# ---------------------------------------------------------------------------------------------------------------------
def _case(sd, name):
    B, Tx, Ty, seed = CASES[name]
    ids, xl, spks, yl, t, z = R.forward_texts(B, Tx, Ty, seed)
    if name == "B5 Ty37":
        xl, yl = torch.tensor([9, 1, 4, 7, 3]), torch.tensor([37, 1, 4, 20, 30])       # a row of one token and one frame; a row with t_x == t_y
    spk = TE.speaker_rows(sd, spks)
    mu64, logw64 = TE.encode(sd, ids, xl, spk)
    _, y, _, _ = R.mel_pairs("aligned", B, Tx, Ty, seed + 2, mu_x=mu64.float(), x_lengths=xl, y_lengths=yl)
    return ids, xl, spks, spk, yl, t, z, y, mu64, logw64


def _yardsticks(sd, case, attn):
    """Float64 losses for the returned attn, batch values and per row, and the float32 oracle's distance from them (computed once per case)."""
    ids, xl, spks, spk, yl, t, z, y, mu64, logw64 = case
    B = ids.shape[0]
    d64, p64, mu_y = R.dur_and_prior_loss(attn, logw64, mu64, y, xl, yl)
    y_t, u = R.cfm_inputs(y, t, z)
    v64 = R.velocity_padded(D.velocity, sd, y_t, mu_y.float(), yl, spk, t, torch.float64)
    l64 = R.diff_loss_from_velocity(v64, u, yl)
    e_ref = R.diff_loss_fp32_oracle(D.velocity, sd, y, mu_y, yl, spk, t, z, l64)
    v32 = R.velocity_padded(D.velocity, sd, y_t, mu_y.float(), yl, spk, t, torch.float32).float()
    a64 = attn.detach().cpu().double()
    x_mask = (torch.arange(ids.shape[1])[None, :] < xl[:, None]).double()
    logw_ = torch.log(1e-8 + a64.sum(-1)) * x_mask
    rows, e_ref_row = {"dur_loss": [], "prior_loss": [], "diff_loss": []}, 0.0
    for b in range(B):
        n, nx = int(yl[b]), int(xl[b])
        rows["dur_loss"].append(float(((logw64[b].reshape(-1).double() - logw_[b]) ** 2).sum() / nx))
        rows["prior_loss"].append(float((0.5 * ((y[b, :, :n].double() - mu_y[b, :, :n]) ** 2 + math.log(2 * math.pi))).sum() / (n * 80)))
        w64 = float(((v64[b, :, :n].double() - u[b, :, :n].double()) ** 2).sum() / (n * 80))
        w32 = torch.nn.functional.mse_loss(v32[b, :, :n], u[b, :, :n], reduction="sum") / torch.tensor(float(n * 80))
        assert w32.dtype == torch.float32
        rows["diff_loss"].append(w64)
        e_ref_row = max(e_ref_row, abs(float(w32) - w64) / w64)
    return {"batch": (d64, p64, l64), "rows": rows, "e_ref": e_ref, "e_ref_row": e_ref_row}


def _check_batch(want, out, tag):
    d64, p64, l64 = want["batch"]
    e_d, e_p, e_l = abs(float(out[0]) - d64) / d64, abs(float(out[1]) - p64) / p64, abs(float(out[2]) - l64) / l64
    print(f"LOSSERR {tag}: dur rel {e_d:.2e}  prior rel {e_p:.2e}  (gate {GATE_LOSS:.0e});  diff {float(out[2]):.6f} rel {e_l:.2e}  gate {GATE_DIFF:.2e}")
    _note("diff_batch", e_l)
    assert all(o.dtype == torch.float32 for o in out[:3])
    assert e_d <= GATE_LOSS and e_p <= GATE_LOSS
    assert e_l <= GATE_DIFF


@pytest.mark.parametrize("name", list(CASES))
def test_losses_against_fp64(sd, model, name):
    case = _case(sd, name)
    ids, xl, spks, spk, yl, t, z, y, mu64, logw64 = case
    B = ids.shape[0]
    batched = model.forward(ids, xl, y, yl, spks, t=t, z=z, batched=True)
    rowwise = model.forward(ids, xl, y, yl, spks, t=t, z=z, batched=False)
    sc = model.score(ids, xl, y, yl, spks, t=t, z=z)
    assert len(batched) == 4 and len(rowwise) == 4 and tuple(batched[3].shape) == (B, ids.shape[1], y.shape[-1])
    assert torch.equal(batched[3], rowwise[3]) and torch.equal(sc["attn"], batched[3]), "the same alignment call"
    R.check_structure(batched[3], xl, yl, sc["durations"])
    assert sc["durations"].dtype == torch.int64 and set(sc) == {"dur_loss", "prior_loss", "diff_loss", "attn", "durations"}
    want = _yardsticks(sd, case, batched[3])
    print(f"\nLOSSERR {name}: float32 oracle rel {want['e_ref']:.2e} (recorded worst {REF_DIFF_WORST:.1e})  worst row {want['e_ref_row']:.2e} "
          f"(recorded worst {REF_DIFF_ROW_WORST:.1e})")
    assert want["e_ref"] <= 1.5 * REF_DIFF_WORST and want["e_ref_row"] <= 1.5 * REF_DIFF_ROW_WORST, "the float32 oracle moved: the gate constants are stale"
    _check_batch(want, batched, f"{name} batched=True ")
    _check_batch(want, rowwise, f"{name} batched=False")
    worst = {"dur_loss": 0.0, "prior_loss": 0.0, "diff_loss": 0.0}
    for k in worst:
        got = sc[k]
        assert got.dtype == torch.float32 and tuple(got.shape) == (B,)
        for b in range(B):
            worst[k] = max(worst[k], abs(float(got[b]) - want["rows"][k][b]) / want["rows"][k][b])
    print(f"LOSSERR {name} score, worst row: dur rel {worst['dur_loss']:.2e}  prior rel {worst['prior_loss']:.2e}  (gate {GATE_LOSS:.0e});  "
          f"diff rel {worst['diff_loss']:.2e}  gate {GATE_DIFF_ROW:.2e}")
    _note("diff_row", worst["diff_loss"])
    assert worst["dur_loss"] <= GATE_LOSS and worst["prior_loss"] <= GATE_LOSS
    assert worst["diff_loss"] <= GATE_DIFF_ROW
    # t and z drawn inside: the alignment side is unchanged, the diff loss is some finite positive number
    drawn = model.forward(ids, xl, y, yl, spks, batched=True)
    assert float(drawn[0]) == float(batched[0]) and float(drawn[1]) == float(batched[1]) and torch.isfinite(drawn[2]) and float(drawn[2]) > 0
    with pytest.raises(NotImplementedError, match="out_size"):
        model.forward(ids, xl, y, yl, spks, out_size=32, batched=True)


# ---------------------------------------------------------------------------------------------------------------------
# the CLI, and the refusal under stream capture
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_losses(model, tmp_path):
    from emojivoice_amd import audio
    from emojivoice_amd.cli import cli, loss_draws, write_wav_pcm24

    g = torch.Generator().manual_seed(34)
    wav = (torch.randn(57 * 256 + 100, generator=g) * 0.1).numpy()
    p, q = tmp_path / "voice.wav", tmp_path / "plain.wav"
    write_wav_pcm24(p, wav)
    write_wav_pcm24(q, wav)
    ids = "0 23 0 51 0 7 0 99 0"
    cli(["--synthetic", "--align_wav", str(q), "--ids", ids, "--spk", "3"])
    assert os.path.exists(f"{q}.durations.npy") and not os.path.exists(f"{q}.losses.json"), "without --losses nothing new is written"
    cli(["--synthetic", "--align_wav", str(p), "--ids", ids, "--spk", "3", "--losses", "--seed", "5"])
    assert np.array_equal(np.load(f"{p}.durations.npy"), np.load(f"{q}.durations.npy"))
    with open(f"{p}.losses.json") as f:
        rec = json.load(f)
    y = torch.from_numpy(audio.read_wav_pcm(str(p), 22050)[: 57 * 256].copy()).to(DEV).unsqueeze(0)
    mel = audio.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000, out_scale=1.0 / model.mel_std, out_shift=-model.mel_mean / model.mel_std)
    assert mel.shape[-1] == 57 and rec["frames"] == 57 and rec["tokens"] == 9 and rec["seed"] == 5
    t, z = loss_draws(5, 80, 57)
    x = torch.tensor([[int(i) for i in ids.split()]])
    sc = model.score(x, torch.tensor([9]), mel, torch.tensor([57]), torch.tensor([3]), t=t, z=z)
    for k in ("dur_loss", "prior_loss", "diff_loss"):
        assert math.isfinite(rec[k]) and rec[k] > 0 and rec[k] == float(sc[k][0]), (k, rec[k], float(sc[k][0]))
    assert rec["t"] == float(t[0])


def test_the_per_row_calls_refuse_stream_capture(sd, eng):
    """Checked at the C boundary with tensors made beforehand, so that the capture holds nothing: both calls return before they enqueue."""
    x, mu, spk, L, t = _est_inputs(sd, 3, 40)
    Ld, out = L.to(DEV), torch.empty_like(x)
    sums = torch.zeros(3, 2, dtype=torch.float64, device=DEV)
    tv = np.ascontiguousarray(t.numpy())
    eng.estimator_rows(x, mu, Ld, spk, t)                                   # the workspace is there: only the capture is in the way
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamBeginCapture.argtypes, hip.hipStreamEndCapture.argtypes, hip.hipGraphDestroy.argtypes = [C.c_void_p, C.c_int], [C.c_void_p, C.POINTER(C.c_void_p)], [C.c_void_p]
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    rcs, graph = [], C.c_void_p()
    assert hip.hipStreamBeginCapture(s.cuda_stream, 2) == 0                  # hipStreamCaptureModeRelaxed
    try:
        rcs.append(eng.lib.ev_estimator_rows(eng.h, x.data_ptr(), mu.data_ptr(), Ld.data_ptr(), spk.data_ptr(), tv.ctypes.data_as(C.c_void_p), 3, 40,
                                             out.data_ptr(), s.cuda_stream))
        msg1 = eng.lib.ev_last_error(eng.h).decode()
        rcs.append(eng.lib.ev_cfm_loss(eng.h, x.data_ptr(), mu.data_ptr(), Ld.data_ptr(), spk.data_ptr(), x.data_ptr(), tv.ctypes.data_as(C.c_void_p), 3, 40,
                                       1e-4, sums.data_ptr(), None, s.cuda_stream))
        msg2 = eng.lib.ev_last_error(eng.h).decode()
    finally:
        assert hip.hipStreamEndCapture(s.cuda_stream, C.byref(graph)) == 0    # an empty graph: never instantiated, never launched
        if graph.value:
            hip.hipGraphDestroy(graph)
    assert rcs[0] != 0 and rcs[1] != 0 and "eager-only" in msg1 and "eager-only" in msg2, (rcs, msg1, msg2)
    with pytest.raises(ValueError, match="one time per utterance"):
        eng.estimator_rows(x, mu, Ld, spk, t[:2])
    assert torch.equal(eng.estimator_rows(x, mu, Ld, spk, t), eng.estimator_rows(x, mu, Ld, spk, t)), "the handle works on after the refusals"
