"""The CPU side of ev_modulation: the numpy restatement (tests/modulation_ref.py) against a direct least-squares detrend and numpy's FFT, the
documented orders of the sums, the mutants, float64 against longdouble and the decision margin on every case of the device test, the physical
property (a sinusoid's rate and extent come back), the header and the exported symbol, and the argument checks of the audio functions.
"""
import os
import re

import numpy as np
import pytest
import torch

import modulation_ref as R
from emojivoice_amd import _lib, audio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return R.cases()


@pytest.fixture(scope="module")
def results(cases):
    return {name: (R.batch(*c[:3], **c[3]), R.batch(*c[:3], dtype=np.longdouble, **c[3])) for name, c in cases.items()}


# ---- the restatement against numpy ------------------------------------------------------------------------------------------------------------
def test_restatement_against_lstsq_and_fft_on_an_on_grid_case():
    """One run of 128 frames and the grid nu_j = (4 + j) / 128: the frequencies are FFT bins, so P_j = 2 |FFT(w r)[4 + j]|^2 / (sum w)^2 with r
    the residual of numpy's own least-squares line.  Agreement to 1e-12 relative to the largest power: both are float64, the orders differ."""
    g = np.random.default_rng(1)
    l = 128
    t = np.arange(l, dtype=np.float64)
    u = 20.0 + 0.07 * t + 0.6 * np.sin(2 * np.pi * (9.0 / l * t + 0.2)) + 0.2 * g.standard_normal(l)
    nu = R.grid(4.0 / l, 1.0 / l, 32)
    P, b, s2, r, w = R.analyse_run(u, nu)
    A = np.stack([np.ones(l), t], axis=1)
    coef, *_ = np.linalg.lstsq(A, u, rcond=None)
    r_np = u - A @ coef
    w_np = 0.5 - 0.5 * np.cos(np.pi * (2 * t + 1) / l)
    X = np.fft.fft(w_np * r_np)
    P_np = 2.0 * np.abs(X[4: 36]) ** 2 / w_np.sum() ** 2
    assert abs(b - coef[1]) <= 1e-12 and np.max(np.abs(r - r_np)) <= 1e-12 and np.max(np.abs(w - w_np)) <= 1e-15
    assert np.max(np.abs(P - P_np)) <= 1e-12 * P_np.max() and abs(s2 - (r_np ** 2).sum()) <= 1e-12 * s2
    assert np.argmax(P) == 5 and abs(np.sqrt(2.0 * P[5]) - 0.6) < 0.05, "bin 9 holds the sinusoid: half the squared amplitude"
    assert w.min() > 0.0 and np.max(np.abs(w - w[::-1])) < 1e-15, "the window is symmetric and never zero"
    out = R.contour(u, None, l, 4.0 / l, 1.0 / l, 32, 3, 0.0, bands=((0, 32),))
    assert np.array_equal(out["spec"], P) and (out["weight"] == l).all() and out["count"].tolist() == [l, 0, 1, l, 5], "one run pools to itself"
    assert out["stat"][0] == s2 / l and out["stat"][1] == b


def test_the_sums_are_the_documented_orders():
    g = np.random.default_rng(2)
    x = g.standard_normal(200) * 10.0 ** g.integers(-8, 8, size=200)
    slots = [0.0] * 64
    for i, v in enumerate(x):
        slots[i % 64] = slots[i % 64] + v
    for o in (32, 16, 8, 4, 2, 1):
        slots = [slots[i] + slots[i ^ o] for i in range(64)]
    assert R.wave_sum(x) == slots[0]
    T = g.standard_normal((37, 3))
    ch = np.zeros((4, 3))
    for i in range(37):
        ch[i % 4] = ch[i % 4] + T[i]
    assert np.array_equal(R.chain_sum(T), ((ch[0] + ch[1]) + ch[2]) + ch[3])
    assert R.wave_sum([]) == 0.0 and np.array_equal(R.chain_sum(np.zeros((0, 2))), np.zeros(2))


def test_runs_resolution_and_pooling_on_a_hand_case():
    """Two runs of 8 and 16 frames around a gap, a third of 3 frames under min_run = 4: nu = 0.125 and 0.25 with min_cycles = 2 resolve as 8 nu >= 2
    and 16 nu >= 2 say, and the pooled power is the length-weighted mean of the runs' powers."""
    g = np.random.default_rng(3)
    v = g.standard_normal(40)
    m = np.zeros(40, np.uint8)
    m[2: 10], m[12: 28], m[30: 33] = 1, 1, 1
    out = R.contour(v, m, 40, 0.125, 0.125, 2, 4, 2.0)
    nu = R.grid(0.125, 0.125, 2)
    Pa, Pb = R.analyse_run(v[2: 10], nu)[0], R.analyse_run(v[12: 28], nu)[0]
    assert out["count"].tolist() == [27, 0, 2, 24] and out["weight"].tolist() == [16, 24]
    assert out["spec"][0] == (16.0 * Pb[0]) / 16.0 and out["spec"][1] == ((0.0 + 8.0 * Pa[1]) + 16.0 * Pb[1]) / 24.0


# ---- every case of the device test ---------------------------------------------------------------------------------------------------------------------
def test_float64_and_longdouble_agree_on_every_count_weight_and_peak_index(cases, results):
    for name, (r64, rld) in results.items():
        assert np.array_equal(r64["count"], rld["count"]) and np.array_equal(r64["weight"], rld["weight"]), name
        for key in ("spec", "peak", "stat"):
            assert R.err(r64[key], rld[key].astype(np.float64)) <= 1e-3 * R.TOL, (name, key)


def test_every_case_has_a_decision_margin_of_at_least_1e_6(cases, results):
    """Every comparison a peak rests on, of every band of every contour of every case: none is left out."""
    worst = {name: R.decision_margin(cases[name], results[name][0]) for name in cases}
    print("\nmodulation decision margins: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(v >= R.MARGIN for v in worst.values()), worst
    assert sum(np.isfinite(v) for v in worst.values()) >= 10, "most cases decide a peak"


def test_the_cases_cover_what_the_device_test_lists(cases, results):
    assert {c[0].shape[2] for n, c in cases.items() if n.startswith("F")} == {3, 63, 64, 65, 255, 256, 257, 1023} and cases["run4096"][0].shape == (1, 1, 4096)
    assert {c[3]["NM"] for c in cases.values()} >= {1, 3, 64, 65, 128} and {len(c[3]["bands"]) for c in cases.values()} >= {0, 1, 4}
    assert all(R.grid(c[3]["nu0"], c[3]["dnu"], c[3]["NM"])[-1] <= 0.5 and 3 <= c[3]["min_run"] <= c[0].shape[2] for c in cases.values())
    assert len(R.CONTOURS) == 6 and len(R.MASKS) == 6
    seen = set()
    for i in range(len(R.SHAPES)):
        for bk in range(12):
            seen.add((R.CONTOURS[(bk + i) % 6], R.MASKS[((bk + i) // 6 + bk + i) % 6]))
    assert len({c for c, _ in seen}) == 6 and len({m for _, m in seen}) == 6
    v, m, lens, kw = cases["F64"]
    runs = [R.runs_of((m[b, k, : lens[b]] != 0) & np.isfinite(v[b, k, : lens[b]])) for b in range(3) for k in range(4)]
    ls = {l for rs in runs for _, l in rs}
    assert kw["min_run"] in ls and kw["min_run"] - 1 in ls, "a run of exactly min_run and one of min_run - 1"
    for name, c in cases.items():
        if c[2] is not None:
            for b, n in enumerate(c[2]):
                if 0 <= n < c[0].shape[2]:
                    assert np.isnan(c[0][b, :, n:]).all() and (c[1] is None or (c[1][b, :, n:] != 0).all()), "NaN under the mask behind every length"
    r = results["run4096"][0]
    assert r["count"][0, 0, :4].tolist() == [4096, 0, 1, 4096]
    r = results["boundary"][0]
    assert r["weight"][0, 0, 11] == 40 and r["weight"][0, 0, 12] == 72, "nu_12 l = 2 exactly is resolved"
    r = results["nonfinite"][0]
    assert r["count"][0, 0, 1] == 5 and r["count"][1, 1, 1] == 200
    r = results["neighbours-outside"][0]
    assert r["count"][0, 0, 4:].tolist() == [20, -1, -1, 20], "a band of one j whose neighbours lie outside, and bands without a candidate"
    assert any((res[0]["count"][..., 2] > 1).any() for res in results.values())


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_moves_its_named_output_past_tol(cases, results, mutant):
    name, bk, what = R.MUTANT_SHOWS[mutant]
    c = cases[name]
    bad = R.batch(*c[:3], mutant=mutant, **c[3])[what][bk]
    good = results[name][0][what][bk]
    assert R.err(bad, good) > 1e-6 > R.TOL, (mutant, R.err(bad, good))


def test_every_mutant_is_listed():
    assert set(R.MUTANT_SHOWS) == set(R.MUTANTS) and len(R.MUTANTS) == 6


# ---- the physical property -----------------------------------------------------------------------------------------------------------------------------
def test_a_sinusoid_on_a_line_comes_back_with_its_rate_and_extent():
    """A 0.5-unit sinusoid at 4.0, 5.6, 6.13, 7.9 and 11.37 Hz with three phases each, on a line, in one run of 64, 129, 258 or 516 frames at
    86.13 frames per second, on the default grid (1 .. 16 Hz by 0.125 Hz, min_cycles 2).  The committed restatement shows at worst 0.0118 Hz and
    0.843 % (both at 64 frames, 4.0 Hz, phase 0); the gates are twice that."""
    rate = R.AUDIO_RATE
    kw = dict(R.AUDIO_KW, bands=((0, 121),))
    worst_r = worst_e = 0.0
    for l in (64, 129, 258, 516):
        for f in (4.0, 5.6, 6.13, 7.9, 11.37):
            for ph in (0.0, 0.31, 0.77):
                t = np.arange(l) / rate
                v = 30.0 + 0.8 * t + 0.5 * np.sin(2 * np.pi * (f * t + ph))
                pk = R.batch(v[None, None], None, None, **kw)["peak"][0, 0, 0]
                worst_r, worst_e = max(worst_r, abs(pk[0] * rate - f)), max(worst_e, abs(pk[1] - 0.5) / 0.5)
    print(f"\nmodulation physical property: worst rate error {worst_r:.4f} Hz, worst extent error {100 * worst_e:.3f} %")
    assert worst_r <= 0.0236 and worst_e <= 0.01686


def test_a_vibrato_over_six_voiced_runs_with_noise():
    """5.5 Hz, 0.4 semitones, six runs of 55 to 90 frames, noise of 0.03: the committed restatement gives 5.5021 Hz and 0.3963 semitones; the gates
    are twice those errors (0.0042 Hz, 0.0075 semitones)."""
    rate = R.AUDIO_RATE
    g = np.random.default_rng(5)
    F = 516
    t = np.arange(F) / rate
    v = 35.0 + 0.5 * t + 0.4 * np.sin(2 * np.pi * 5.5 * t + 0.3) + 0.03 * g.standard_normal(F)
    m, at = np.zeros(F, np.uint8), 5
    for l in (70, 55, 90, 64, 80, 75):
        m[at: at + l] = 1
        at += l + 8
    r = R.batch(v[None, None], m[None, None], None, **dict(R.AUDIO_KW, bands=((24, 89),)))
    got_rate, got_ext = r["peak"][0, 0, 0, 0] * rate, r["peak"][0, 0, 0, 1]
    print(f"\nmodulation vibrato over six runs: {got_rate:.4f} Hz, {got_ext:.4f} semitones")
    assert r["count"][0, 0, 2] == 6 and abs(got_rate - 5.5) <= 0.0042 and abs(got_ext - 0.4) <= 0.0075


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_ev_modulation():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    assert re.search(r"\bint ev_modulation\(ev_handle \*h,", header) and "ev_modulation" in _lib.EXPORTS
    assert "ev_modulation" in re.search(r"#define EV_ABI_VERSION 4 .*", header).group(0), "the additions list of the ABI line"
    for word in ("RESOLVED", "ANALYSED", "t mod 64", "t mod 4", "((s0 + s1) + s2) + s3", "nu0 + (NM - 1) dnu <= 0.5", "3 <= min_run <= F", "1 <= NM <=\n *   128"):
        assert word in header, word
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, "ev_modulation") and lib.ev_abi_version() == 4


# ---- the audio functions' arguments -----------------------------------------------------------------------------------------------------------------------
def test_modulation_grid():
    nu0, dnu, NM = audio.modulation_grid(22050, 256)
    assert NM == 121 and nu0 == 1.0 / R.AUDIO_RATE and dnu == 0.125 / R.AUDIO_RATE and (nu0, dnu, NM) == tuple(R.AUDIO_KW[k] for k in ("nu0", "dnu", "NM"))
    assert audio.modulation_grid(22050, 256, *audio.MS_DISTANCE_GRID_HZ)[2] == 125
    assert audio.modulation_grid(16000, 160, 2.0, 2.0, 0.5)[2] == 1
    for bad in (dict(step_hz=0.1), dict(fmax_hz=50.0, step_hz=0.5), dict(fmin_hz=0.0), dict(step_hz=float("nan")), dict(fmin_hz=3.0, fmax_hz=2.0)):
        with pytest.raises(ValueError, match="modulation"):
            audio.modulation_grid(22050, 256, **bad)
    with pytest.raises(ValueError, match="modulation_grid"):
        audio.modulation_grid(22050, 0)


def test_modulation_arguments():
    v = torch.zeros(2, 3, 100, dtype=torch.float32)
    shape, grid, bands, min_run = audio.modulation_arguments(v, torch.ones(2, 1, 100, dtype=torch.bool), [100, 20], bands_hz=((4, 12), (2, 8)))
    assert shape == (2, 3, 100) and grid[2] == 121 and bands == [(24, 89), (8, 57)] and min_run == 18
    assert audio.modulation_arguments(torch.zeros(10))[3] == 10, "min_run is held inside 3 .. F"
    assert audio.modulation_bands(((15.95, 30.0),), 1.0, 0.125, 121) == [(120, 121)]
    for kw, word in ((dict(values=torch.zeros(2, 3, 4097)), "F=4097"), (dict(values=torch.zeros(2)), "at least 3"), (dict(values=torch.zeros(2, 2, 2, 9)), "floating tensor"),
                     (dict(values=v, mask=torch.ones(2, 3, 99)), "does not broadcast"), (dict(values=v, lengths=[1, 2, 3]), "2 lengths"),
                     (dict(values=v, bands_hz=((1, 2),) * 5), "at most 4"), (dict(values=v, bands_hz=((20.0, 30.0),)), "holds no frequency"),
                     (dict(values=v, bands_hz=((4.01, 4.02),)), "holds no frequency"), (dict(values=v, min_run=2), "min_run=2"),
                     (dict(values=v, min_run=101), "min_run=101"), (dict(values=v, min_cycles=-1.0), "min_cycles"),
                     (dict(values=v, min_cycles=float("inf")), "min_cycles"), (dict(values=v, frame_rate=20.0), "half the frame rate"),
                     (dict(values=v, step_hz=0.05), "at most 128")):
        with pytest.raises(ValueError, match=re.escape(word)) as e:
            audio.modulation_arguments(**kw)
        assert "modulation" in str(e.value) and "functionals" not in str(e.value)
    with pytest.raises(_lib.EvLibraryError, match="GPU only"):
        audio.modulation(v)


def test_voice_modulation_and_the_distance_reject_wrong_shapes():
    with pytest.raises(ValueError, match=r"\(B, F\) contours"):
        audio.voice_modulation({"f0": torch.zeros(10), "voiced": torch.zeros(10, dtype=torch.bool)}, {})
    au = {"loudness": torch.zeros(2, 9), "spectral_flux": torch.zeros(2, 9), "power": torch.zeros(2, 9), "mfcc": torch.zeros(2, 9, 4),
          "live": torch.ones(2, 9, dtype=torch.bool), "has_previous": torch.ones(2, 9, dtype=torch.bool)}
    with pytest.raises(ValueError, match="same frames"):
        audio.voice_modulation({"f0": torch.zeros(2, 10), "voiced": torch.zeros(2, 10, dtype=torch.bool)}, au)
    with pytest.raises(ValueError, match="modulation_spectrum_distance"):
        audio.modulation_spectrum_distance(torch.zeros(2, 80, 50), torch.zeros(3, 80, 40))
    with pytest.raises(ValueError, match="modulation_spectrum_distance"):
        audio.cepstral_modulation_distance(torch.zeros(2, 13, 50), torch.zeros(2, 12, 40))


def test_the_reports_take_modulation_only_with_a_report():
    import argparse

    from emojivoice_amd import cli

    ns = dict(modulation=True, evaluate_pairs=None, voice_report=None, sample_rate=None, prepare_dataset=None)
    with pytest.raises(AssertionError, match="--modulation"):
        cli.validate_args(argparse.Namespace(**ns))
    cli.validate_args(argparse.Namespace(**dict(ns, voice_report="x.txt", batch_size=2)))
    rows = [{"modulation": {"a": 1.0, "b": None}}, {"modulation": {"a": 3.0, "b": None}}]
    assert cli.modulation_means(rows) == {"modulation": {"a": {"mean": 2.0, "files": 2}, "b": {"mean": None, "files": 0}}}
    vm = {k: torch.tensor([1.5, float("nan")], dtype=torch.float64) for k in audio.VOICE_MODULATION_FIGURES}
    got = cli.modulation_rows(vm)
    assert [tuple(r["modulation"]) for r in got] == [audio.VOICE_MODULATION_FIGURES] * 2
    assert got[0]["modulation"]["tremor_rate_hz"] == 1.5 and got[1]["modulation"]["rhythm_depth"] is None
