"""ev_denoise / ev_stft_magnitude on the MI355X, row by row against the fp64 yardstick of tests/denoiser_ref.py, on every conv build the
two DFT-basis layers reach.

The yardstick is the reference's call sequence (torch.stft, |X|, angle, clamp(|X| - bias * strength, 0), torch.istft) in float64 on the
CPU; tests/test_denoiser_reference.py pins it to the oracle and to the committed reference output, and sets the gates from the float32
restatement of the engine's method, measured on exactly the cases below (denoiser_ref.CASES), never from the engine's output:
    GATE_RMS = 1.61e-6 (row RMS error / row input RMS),  GATE_MAX = 4.23e-6 (largest error / input peak),
    GATE_MAG = 6.10e-6 (largest |X| error / the row's largest |X|);   3 x the worst row of the sequential restatement.
Every row of every case is gated on its own: a quiet row (1e-4) between two loud ones has the same relative gate as they have.

The ladder.  A launch has B * (frames + 12) rows; launch_conv picks the build from the tile counts (pick_cfg).  ev_dbg_last_cfg after
stft_magnitude names the forward layer's build (Cin 256 -> Cout 1032: the last 64-channel M tile holds 8 channels), after denoise the
inverse layer's (Cin 1032, K padded to 1056, 4 taps at 0 .. -3):
    (B, frames)  rows   forward               inverse
    (1, 3)          15  19 SK32 (fast)        19 SK32 (general)
    (3, 21)         99  19                    19
    (64, 3)        960   8 64x64 prefetch     19
    (64, 8)       1280   1 64x128             19
    (64, 20)      2048   5 64x192             19
    (64, 40)      3328   1                     8
    (64, 52)      4096  56 64x64 balanced      8
    (64, 88)      6400   1                     1
    (64, 120)     8448   5                     5
    (64, 245)    16448   6 64x64              56
    (7, 516)      3696   1                     8     odd batch, a row count that is no multiple of a tile
    (1, 1200)     1212   1                    19     the streaming reserve length
and the bench shape 64 x 516 (33 792 rows: forward 1, inverse 5) once.  test_the_ladder_reaches_every_build asserts the two sets.
Every ladder shape runs under both (bias, strength) pairs of denoiser_ref.PAIRS and at strength 0.  One DNERR line per case with -s.

Measured on one MI355X (worst row over the cases; NOTES.md, "Denoiser against fp64, row by row", has the table per shape): relRMS / relLinf
3.5 .. 4.8e-7 / 4.5 .. 8.0e-7 where the inverse layer runs on the split-K build (19), 1.11e-6 / 2.8 .. 4.15e-6 on every conv_gemm build (8, 1, 5,
56): 0.69 x GATE_RMS and up to 0.98 x GATE_MAX, at (64, 245) under the `voc` pair.  Those builds sum the four taps as one chain of 4 x 1056 terms
where the restatement sums 1026 per frame and then overlap-adds; the same chain in float32 on the CPU gives 1.11e-6 / 3.63e-6.  Magnitude: 2.4e-7
(build 19) to 1.95e-6 (the 1024-term chains), 0.32 x GATE_MAG.  The figures repeat from run to run (same bits on every call and setting).
Run time of this module: 9 s.

Both layers run the exact fp32 MFMA in every arithmetic setting (their shapes keep them off the 16-bit pipes: Cout 1032 is a multiple of
neither 64 nor 128, and the inverse layer's K is padded); test_arithmetic_settings_do_not_change_a_bit pins that at three shapes.
"""
import pytest
import torch

import denoiser_ref as D
from emojivoice_amd._lib import Engine, EvLibraryError

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORWARD_BUILDS, INVERSE_BUILDS = {19, 8, 1, 5, 56, 6}, {19, 8, 1, 5, 56}


@pytest.fixture(scope="module")
def eng():
    return Engine(0)


def _gate(tag, got, y, audio, builds=""):
    """Every row of got = (mag, out) (either may be None) inside the three gates; one DNERR line."""
    rms, mx, mg = D.row_errors(got, y, audio)
    w = D.worst((rms, mx, mg))
    line = "  ".join(f"{name} {v:.2e} ({v / gate:.2f} x gate)" for name, v, gate in
                     (("relRMS", w[0], D.GATE_RMS), ("relLinf", w[1], D.GATE_MAX), ("mag", w[2], D.GATE_MAG)) if v is not None)
    print(f"\nDNERR {tag}{builds}: worst row  {line}")
    for t in got:
        assert t is None or bool(torch.isfinite(t).all())
    assert rms is None or bool((rms <= D.GATE_RMS).all()), (tag, rms)
    assert mx is None or bool((mx <= D.GATE_MAX).all()), (tag, mx)
    assert mg is None or bool((mg <= D.GATE_MAG).all()), (tag, mg)


def _run(eng, audio, bias, strength):
    """(mag, out, forward build, inverse build) of one stft_magnitude and one denoise call."""
    a, b = audio.to(DEV), bias.to(DEV)
    mag = eng.stft_magnitude(a)
    fwd = eng.last_cfg()
    out = eng.denoise(a, b, strength)
    inv = eng.last_cfg()
    return mag, out, fwd, inv


@pytest.mark.parametrize("case", D.CASES, ids=[D.case_id(c) for c in D.CASES])
def test_every_row_against_the_fp64_yardstick(eng, case):
    B, T, _, _ = case
    audio, bias, strength = D.case_inputs(case)
    y = D.yardstick(audio, bias, strength)
    mag, out, fwd, inv = _run(eng, audio, bias, strength)
    assert tuple(mag.shape) == (B, 513, T + 1) and tuple(out.shape) == (B, 256 * T) and mag.dtype == out.dtype == torch.float32
    assert fwd in FORWARD_BUILDS and inv in INVERSE_BUILDS, (fwd, inv)
    _gate(D.case_id(case), (mag, out), y, audio, f" rows {B * (T + 12)} forward {fwd} inverse {inv}")


def test_the_ladder_reaches_every_build(eng):
    fwd, inv = {}, {}
    for B, T, _ in D.LADDER:
        _, _, f, i = _run(eng, torch.zeros(B, 256 * T), D.bias("rand2"), 0.0005)
        fwd[(B, T)], inv[(B, T)] = f, i
    print(f"\nDNERR builds: forward {fwd}\nDNERR builds: inverse {inv}")
    assert set(fwd.values()) == FORWARD_BUILDS, fwd
    assert set(inv.values()) == INVERSE_BUILDS, inv


@pytest.mark.parametrize("B,T", [(1, 3), (64, 40), (64, 245)])
def test_arithmetic_settings_do_not_change_a_bit(B, T):
    """the denoiser runs the exact fp32 MFMA in every setting."""
    e = Engine(0)
    audio, bias, strength = D.case_inputs((B, T, "mixed", "flat"))
    res = {}
    for s in (0, 16, 6, 3):
        e.set_arithmetic(s)
        res[s] = _run(e, audio, bias, strength)
    e.close()
    mag0, out0, fwd0, inv0 = res[0]
    assert fwd0 in FORWARD_BUILDS and inv0 in INVERSE_BUILDS
    for s in (16, 6, 3):
        mag, out, fwd, inv = res[s]
        assert (fwd, inv) == (fwd0, inv0), (s, fwd, inv)
        assert torch.equal(mag, mag0) and torch.equal(out, out0), f"setting {s} changes the denoiser's bits"
    _gate(f"arithmetic settings B{B}-T{T}", (mag0, out0), D.yardstick(audio, bias, strength), audio, f" forward {fwd0} inverse {inv0}")


@pytest.mark.parametrize("B,T", [(3, 5), (64, 120)])
@pytest.mark.parametrize("strength", [0.0005, 0.0])
def test_a_zero_row_between_full_scale_rows_is_exactly_zero(eng, B, T, strength):
    """No leak across the 4 pad rows between utterances and no stale scratch (a larger call of full-scale rows runs on the handle first):
    zero tolerance, every element of the row's output and of its magnitude."""
    _run(eng, D.signal("noise1", 64, 256 * 132, seed=4), D.bias("rand2"), strength)
    audio = D.signal("loud_zero_loud", B, 256 * T, seed=B)
    mag, out, _, _ = _run(eng, audio, D.bias("rand2"), strength)
    zero = torch.arange(B) % 3 == 1
    assert int(zero.sum()) >= 1 and float(audio[zero].abs().max()) == 0.0 and float(audio[~zero].abs().amax(1).min()) > 1.0
    assert float(out.cpu()[zero].abs().max()) == 0.0 and float(mag.cpu()[zero].abs().max()) == 0.0
    _gate(f"zero rows B{B}-T{T} strength {strength}", (mag, out), D.yardstick(audio, D.bias("rand2"), strength), audio)


def test_a_row_below_the_bias_everywhere_is_exactly_zero(eng):
    audio = D.signal("loud_quiet_loud", 3, 256 * 9, seed=2)
    audio[0] = 0.5 * audio[1]                                            # two quiet rows and a loud one
    bias, strength = D.bias("decay"), 10.0                               # threshold >= 0.1; the quiet rows' |X| stays under 0.02
    mag, out = D.yardstick(audio, bias, strength)
    assert float(mag[:2].max()) < 0.02 and float(out[:2].abs().max()) == 0.0 and float(out[2].abs().max()) > 0.1
    got_mag, got, _, _ = _run(eng, audio, bias, strength)
    assert float(got.cpu()[:2].abs().max()) == 0.0
    _gate("below the bias", (got_mag, got), (mag, out), audio)


def test_negative_strength_follows_the_yardstick(eng):
    """The reference adds bias * |strength| to every magnitude; a silent row comes out as -bias * strength at angle 0.  The silent row has
    no input, so its denominators are those of denoiser_ref.silent_frame (tests/test_denoiser_reference.py holds the restatement to
    the same measure)."""
    audio, bias, strength, den = D.negative_case()
    y = D.yardstick(audio, bias, strength)
    _, out, _, _ = _run(eng, audio, bias, strength)
    assert float(out[1].abs().max()) > 1e-4
    _gate("negative strength", (None, out), y, den)


def test_a_small_call_after_the_largest_reuses_the_scratch_cleanly():
    big, small = D.case_inputs((64, 245, "loud_quiet_loud", "flat")), D.case_inputs((1, 3, "mixed", "flat"))
    fresh = Engine(0)
    want = _run(fresh, *small)
    fresh.close()
    e = Engine(0)
    _run(e, *big)
    got = _run(e, *small)
    e.close()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:]


def test_bad_arguments_are_refused_by_the_host_check(eng):
    bias = D.bias("rand2").to(DEV)
    good = D.signal("noise1", 2, 1024, seed=1).to(DEV)
    before = eng.denoise(good, bias, 0.0005)
    cfg = eng.last_cfg()
    for bad in (torch.zeros(1, 512, device=DEV), torch.zeros(2, 1000, device=DEV), torch.zeros(0, 1024, device=DEV)):
        with pytest.raises(EvLibraryError, match="bad arguments"):
            eng.denoise(bad, bias, 0.0005)
        with pytest.raises(EvLibraryError, match="bad arguments"):
            eng.stft_magnitude(bad)
        assert eng.last_cfg() == cfg, "no launch"
    assert torch.equal(eng.denoise(good, bias, 0.0005), before)


def test_denoiser_class_shapes_and_parity():
    from emojivoice_amd.denoiser import Denoiser
    from emojivoice_amd.hifigan import synthetic

    voc = synthetic(DEV)
    den = Denoiser(voc, mode="zeros")
    assert tuple(den.bias_spec.shape) == (1, 513, 1)
    audio = D.signal("mixed", 3, 256 * 21, seed=6)
    bias = den.bias_spec.reshape(-1).cpu()
    strength = 0.0005 / max(1.0, float(bias.max()))                      # whatever the synthetic vocoder's bias is, the rows keep their RMS
    one = den(audio[0].to(DEV), strength=strength)
    many = den(audio.to(DEV), strength=strength)
    assert tuple(one.shape) == (1, 256 * 21) and tuple(many.shape) == (3, 256 * 21)
    assert torch.equal(one[0], many[0])
    y = D.yardstick(audio, bias, strength)
    assert float((y[1].pow(2).mean(1).sqrt() / audio.double().pow(2).mean(1).sqrt()).min()) >= 0.1
    _gate("Denoiser class", (None, many), y, audio)
