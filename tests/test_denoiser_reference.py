"""The denoiser's yardstick and the gates of tests/test_gpu_denoiser.py, without a GPU.

The yardstick (tests/denoiser_ref.py: the reference's torch.stft -> gain -> torch.istft sequence in float64) is pinned to the oracle and to
the committed reference output.  The gates come from the float32 restatement of the engine's method (windowed DFT bases as two matrix
products, overlap-add, envelope division; no engine code), measured per row against the yardstick on exactly denoiser_ref.CASES, the
case list of the GPU module.  Three figures per row (denoiser_ref.row_errors): RMS error over the input's RMS, largest error over the
input's peak, largest magnitude error over the row's largest |X|.

Measured (worst row over the 37 cases; every case prints its own line with -s, DNREF):
                                                             relRMS     relLinf    magnitude
    restatement, blocked (the CPU's matrix product)          3.33e-7    6.48e-7    1.17e-6
    restatement, sequential (one fused term at a time)       5.38e-7    1.41e-6    2.03e-6     <- sets the gates
    torch.stft / istft in float32 (the reference's own)      1.37e-7    2.98e-7    2.83e-7
The sequential order is the least favourable a correct float32 kernel may take, and the gates are 3 x its worst row, the margin the mel,
decoder and vocoder modules use:
    GATE_RMS = 1.61e-6,  GATE_MAX = 4.23e-6,  GATE_MAG = 6.10e-6.
The figures barely move with the shape (relRMS 4.7e-7 at 3 frames, 5.0e-7 at 64 x 516) or with the gain (the pairs of denoiser_ref.PAIRS
against strength 0), so one gate serves every case.  test_restatement_sits_inside_the_gates measures them again on every run and fails
if the restatement leaves 1.5 x gate / 3: the constants cannot go stale.

Denominators come from the input, so a strength that removed most of a row would make the figures look better than they are: every
non-silent row of every case keeps at least 0.1 of its input RMS in the yardstick (asserted; measured 0.79 .. 1.0).

Mutants of the yardstick (symmetric Hann window; reflect padding with the edge sample repeated; the envelope replaced by its interior
constant 1.5; DC and Nyquist doubled in the inverse; the bias shifted by one bin; the gain applied to the power) each miss GATE_MAX on
every row of denoiser_ref.MUTANT_CASES, and GATE_RMS too unless the defect is confined to the first and last 768 samples.  The mutant
cases are quiet (noise at 1e-4): a window that is wrong in analysis and synthesis alike still reconstructs a row the gain hardly touches,
and shows there in the magnitude only (asserted against GATE_MAG).
"""
import numpy as np
import pytest
import torch

import denoiser_ref as D
from oracle import matcha_oracle as O

GATE_RMS, GATE_MAX, GATE_MAG = D.GATE_RMS, D.GATE_MAX, D.GATE_MAG
SEQ_WORST = (5.38e-7, 1.41e-6, 2.03e-6)                          # the sequential restatement's worst row (the table above)
_FWD = {}


def _forward(case, audio, sequential):
    """The restatement's forward transform, shared by the cases of one shape (they differ in bias and strength only)."""
    key = case[:3] + (sequential,)
    if key not in _FWD:
        for k in [k for k in _FWD if k[:3] != key[:3]]:
            del _FWD[k]
        _FWD[key] = D.forward_f32(audio, sequential)
    return _FWD[key]


def test_yardstick_in_float32_is_the_oracle():
    for case in ((3, 21, "mixed", "flat"), (1, 3, "loud_quiet_loud", "voc"), (2, 40, "sines", "flat")):
        audio, bias, strength = D.case_inputs(case)
        mag, out = D.yardstick(audio, bias, strength, torch.float32)
        assert torch.equal(out, O.denoiser(audio, bias[None, :, None], strength=strength)), case
        spec = torch.stft(audio, n_fft=1024, hop_length=256, win_length=1024, window=torch.hann_window(1024), return_complex=True)
        assert torch.equal(mag, torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1))), case


def test_yardstick_reproduces_the_committed_golden(golden):
    audio = torch.from_numpy(golden["g4_wav"]).clamp(-1, 1).squeeze()
    want = golden["g7_denoised"]
    for dtype in (torch.float64, torch.float32):
        _, out = D.yardstick(audio, torch.from_numpy(golden["g7_bias_spec"]), 0.00025, dtype)
        assert tuple(out.shape) == want.shape
        assert float(np.max(np.abs(out.numpy().astype(np.float64) - want))) <= 1e-5           # test_oracle_golden.py's bound


def test_the_gates_are_three_times_the_measured_worst_row():
    for gate, w in zip((GATE_RMS, GATE_MAX, GATE_MAG), SEQ_WORST):
        assert abs(gate - 3 * w) <= 0.005 * gate


def test_envelope_is_what_istft_divides_by():
    env = D.envelope(256 * 8)
    assert float((env[768:-768] - 1.5).abs().max()) <= 1e-12 and float(env.min()) > 0.24 and float(env[0]) < 1.49
    audio, bias, _ = D.case_inputs((2, 8, "noise1", "flat"))
    _, out = D.yardstick(audio, bias, 0.0)
    assert float((out - audio.double()).abs().max()) <= 1e-12, "strength 0 in float64: the identity"


@pytest.mark.parametrize("case", D.CASES, ids=[D.case_id(c) for c in D.CASES])
def test_restatement_sits_inside_the_gates(case):
    audio, bias, strength = D.case_inputs(case)
    y = D.yardstick(audio, bias, strength)
    in_rms, out_rms = audio.double().pow(2).mean(1).sqrt(), y[1].pow(2).mean(1).sqrt()
    kept = float((out_rms / in_rms)[in_rms > 0].min())
    assert kept >= 0.1, "the strength removes too much of a row for a denominator taken from the input"
    figs = {}
    for name, seq in (("blocked", False), ("sequential", True)):
        figs[name] = D.worst(D.row_errors(D.restatement_f32(audio, bias, strength, seq, spec=_forward(case, audio, seq)), y, audio))
    figs["torch float32"] = D.worst(D.row_errors(D.yardstick(audio, bias, strength, torch.float32), y, audio))
    print(f"\nDNREF {D.case_id(case)}: kept {kept:.3f}  " + "  ".join(f"{k} {v[0]:.2e} {v[1]:.2e} {v[2]:.2e}" for k, v in figs.items()))
    for name in ("blocked", "sequential"):
        rms, mx, mg = figs[name]
        assert rms <= GATE_RMS / 3 * 1.5 and mx <= GATE_MAX / 3 * 1.5 and mg <= GATE_MAG / 3 * 1.5, \
            f"the float32 restatement moved ({name}): the gate constants are stale"


def test_negative_strength_on_silence_in_the_restatement():
    """A silent row under a negative strength: clamp(0 - bias * strength, 0) at angle 0, a row that has no input to be measured against.
    test_gpu_denoiser.py takes its denominators from denoiser_ref.silent_frame there; the restatement sits inside the same share of the
    gates under that measure (printed with -s).  The output is small against the frame (the pulse sits where the window is zero), so a
    denominator from the output would not do."""
    audio, bias, strength, den = D.negative_case()
    y = D.yardstick(audio, bias, strength)
    assert float(audio[1].abs().max()) == 0.0 and 1e-4 < float(y[1][1].abs().max()) < float(den[1].abs().max())
    for seq in (False, True):
        rms, mx, _ = D.row_errors((None, D.restatement_f32(audio, bias, strength, seq)[1]), y, den)
        print(f"\nDNREF negative strength, sequential {seq}: per row relRMS {[f'{v:.2e}' for v in rms.tolist()]} relLinf {[f'{v:.2e}' for v in mx.tolist()]}")
        assert float(rms.max()) <= GATE_RMS / 3 * 1.5 and float(mx.max()) <= GATE_MAX / 3 * 1.5, (seq, rms, mx)


MUTANTS = [("symmetric Hann window", dict(symmetric_window=True), True, True),          # (name, switch, misses GATE_RMS, misses GATE_MAG)
           ("edge sample repeated in the reflect padding", dict(edge_repeated=True), False, True),
           ("envelope 1.5 everywhere", dict(flat_envelope=True), False, False),
           ("DC and Nyquist doubled in the inverse", dict(edges_doubled=True), True, False),
           ("bias shifted by one bin", dict(bias_shift=1), True, False),
           ("gain applied to the power", dict(gain_on_power=True), True, False)]


@pytest.mark.parametrize("case", D.MUTANT_CASES, ids=[D.case_id(c) for c in D.MUTANT_CASES])
@pytest.mark.parametrize("name,switch,in_rms,in_mag", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_mutants_miss_the_gates(case, name, switch, in_rms, in_mag):
    audio, bias, strength = D.case_inputs(case)
    y = D.yardstick(audio, bias, strength)
    rms, mx, mg = D.row_errors(D.yardstick(audio, bias, strength, **switch), y, audio)
    print(f"\nDNREF mutant {name} on {D.case_id(case)}: smallest row relRMS {float(rms.min()):.2e} relLinf {float(mx.min()):.2e} mag {float(mg.min()):.2e}")
    assert bool((mx > GATE_MAX).all()), (name, mx)
    if in_rms:
        assert bool((rms > GATE_RMS).all()), (name, rms)
    if in_mag:
        assert bool((mg > GATE_MAG).all()), (name, mg)


def test_symmetric_window_shows_in_the_magnitude_of_loud_rows():
    audio, bias, strength = D.case_inputs((3, 21, "loud_quiet_loud", "flat"))
    y = D.yardstick(audio, bias, strength)
    _, _, mg = D.row_errors(D.yardstick(audio, bias, strength, symmetric_window=True), y, audio)
    assert bool((mg > GATE_MAG).all()), mg


def test_row_errors_compares_a_zero_row_exactly():
    audio = D.signal("loud_zero_loud", 3, 256 * 4, seed=1)
    assert float(audio[1].abs().max()) == 0.0 and float(audio[0].abs().max()) > 1.0
    y = D.yardstick(audio, D.bias("rand2"), 0.0005)
    assert float(y[0][1].abs().max()) == 0.0 and float(y[1][1].abs().max()) == 0.0
    rms, mx, mg = D.row_errors(y, y, audio)
    assert rms.tolist() == [0.0, 0.0, 0.0] and mx.tolist() == [0.0, 0.0, 0.0] and mg.tolist() == [0.0, 0.0, 0.0]
    leak = (y[0].clone(), y[1].clone())
    leak[1][1, 700] = 1e-30
    leak[0][1, 5, 2] = 1e-30
    rms, mx, mg = D.row_errors(leak, y, audio)
    assert rms[1] == float("inf") and mx[1] == float("inf") and mg[1] == float("inf") and float(rms[0]) == 0.0 and float(mg[2]) == 0.0
