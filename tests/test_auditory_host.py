"""CPU-side checks of the auditory path: the numpy restatement (tests/auditory_ref.py) against an independent route (``np.fft.rfft`` of the
padded frames and explicit loops over bands and bins), ``audio.auditory_tables`` and its argument checks, ``audio.auditory_statistics`` and the
report family on hand-made frames, the condition on the inputs of the device tests, the mutants the device tests must tell apart, and the C
ABI's declaration and export.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import auditory_ref as R
from emojivoice_amd import _lib, audio, cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = R.GEOMETRIES + R.EDGE_GEOMETRIES
ALL_IDS = R.IDS + R.EDGE_IDS
_RES = {}


def results(g):
    """(x, lens, float64 results, longdouble results) of rows_for(g): computed once, never modified."""
    if g not in _RES:
        x, lens = R.rows_for(g)
        t = R.tables(g)
        r = (x, lens, R.batch(x, lens, g, t), R.batch(x, lens, g, t, dtype=np.longdouble))
        for part in (r[2], r[3]):
            for v in part.values():
                v.setflags(write=False)
        _RES[g] = r
    return _RES[g]


# ---- the restatement against an independent route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", ALL, ids=ALL_IDS)
def test_restatement_against_fft_and_loops(g):
    x, lens, ref, _ = results(g)
    t = R.tables(g)
    n = lens[0]
    sig = x[0, :n].astype(np.float64)
    nf, NB, off = R.frames(n, g.H), g.nfft // 2 + 1, (g.nfft - g.W) // 2
    fm = R.frame_matrix(sig, g)
    pad = np.zeros((nf, g.nfft))
    pad[:, off:off + g.W] = fm * R.hann(g.W)
    raw = np.abs(np.fft.rfft(pad, axis=1)) ** 2
    got = R.named({k: v[0, :nf] for k, v in ref.items()})
    worst = {k: 0.0 for k in ("power", "bands", "loudness", "mfcc", "spectral_flux", "log_energy")}
    rel = lambda a, b: abs(a - b) / max(abs(b), 1.0)
    for f in range(0, nf, max(1, nf // 40)):
        live = bool((raw[f] > R.POWER_FLOOR).any())
        assert int(got["flags"][f]) == int(live) | (2 if f >= 1 else 0)
        power = math.fsum(raw[f])
        worst["power"] = max(worst["power"], rel(got["power"][f], power))
        E = [math.fsum(raw[f, k] * t["mel_w"][k, m] for k in range(NB)) for m in range(g.n_mel)]
        Ef = [max(e, R.POWER_FLOOR) for e in E]
        loud = math.fsum((t["eq"][m] * Ef[m]) ** R.COMPRESS for m in range(g.n_mel))
        mfcc = [math.fsum(math.log(Ef[m]) * t["dct"][m, i] for m in range(g.n_mel)) for i in range(g.n_ceps)]
        flux = 0.0
        if f >= 1:
            flux = math.sqrt(math.fsum((math.sqrt(raw[f, k]) - math.sqrt(raw[f - 1, k])) ** 2 for k in range(NB)) / NB)
        worst["spectral_flux"] = max(worst["spectral_flux"], rel(got["spectral_flux"][f], flux))
        if not live:
            assert got["loudness"][f] == 0 and got["log_energy"][f] == 0 and not got["mfcc"][f].any() and not got["bands"][f].any()
            continue
        worst["bands"] = max(worst["bands"], max(rel(got["bands"][f, m], E[m]) for m in range(g.n_mel)))
        worst["loudness"] = max(worst["loudness"], rel(got["loudness"][f], loud))
        worst["mfcc"] = max(worst["mfcc"], max(rel(got["mfcc"][f, i], mfcc[i]) for i in range(g.n_ceps)))
        worst["log_energy"] = max(worst["log_energy"], rel(got["log_energy"][f], math.log(max(power, R.POWER_FLOOR))))
    print(f"{g.nfft}/{g.H}/{g.W}: restatement against rfft and loops: {worst}")
    assert max(worst.values()) <= 1e-12                                 # |got - want| <= 1e-12 max(|want|, 1), every figure


@pytest.mark.parametrize("g", ALL, ids=ALL_IDS)
def test_the_inputs_of_the_device_tests_are_well_conditioned(g):
    """The condition of the device tests' comparison rule, on every entry of every frame: none has to be left out."""
    _, _, r64, r80 = results(g)
    worst = {k: R.err(r64[k], r80[k]) for k in ("frame", "mfcc", "bands")}
    print(f"{g.nfft}/{g.H}/{g.W}: float64 against longdouble: {worst}")
    assert np.array_equal(r64["flags"], r80["flags"])
    assert max(worst.values()) <= R.INPUT_TOL


def test_ragged_rows_sit_on_the_tile_seams():
    for g in ALL:
        nf = [R.frames(n, g.H) for n in R.ragged_lens(g.H)]
        assert [v % R.TILE for v in nf] == [14, 0, 1] and max(nf) >= 31, (g, nf)


# ---- audio.auditory_tables ------------------------------------------------------------------------------------------------------------------
def test_auditory_tables_at_the_defaults():
    t = audio.auditory_tables(22050, 1024)
    w, NB = t["mel_w"], 513
    assert w.shape == (NB, 26) and w.dtype == np.float64 and t["eq"].shape == (26,) and t["dct"].shape == (26, 4)
    assert (w >= 0).all() and np.isfinite(w).all()
    assert (w > 0).any(axis=0).all()                                    # no band is empty
    hz = np.arange(NB) * 22050.0 / 1024
    between = (hz >= t["centres_hz"][0]) & (hz <= t["centres_hz"][-1])
    assert between.sum() > 300 and np.max(np.abs(w[between].sum(axis=1) - 1.0)) < 1e-12     # adjacent triangles sum to 1
    assert (t["eq"] > 0).all() and np.isfinite(t["eq"]).all()
    assert (t["k_lo"], t["k_hi"], t["compress"]) == (0, NB, 0.33)
    g = R.GEOMETRIES[3]
    ref = R.tables(g)
    assert np.max(np.abs(w - ref["mel_w"])) < 1e-14 and np.allclose(t["eq"], ref["eq"], rtol=1e-13, atol=0)
    assert np.allclose(t["dct"], ref["dct"], rtol=0, atol=1e-14)
    # Hermansky's curve: 100 Hz lies more than 20 dB under 1 kHz, and the weights rise with the centres up to 4 kHz
    assert audio.equal_loudness(100.0) < 1e-2 * audio.equal_loudness(1000.0) and (np.diff(t["eq"][t["centres_hz"] < 4000.0]) > 0).all()


def test_dct_columns_are_orthogonal_before_liftering():
    d = audio.auditory_tables(22050, 1024, n_ceps=16, lifter=0.0)["dct"]
    assert np.max(np.abs(d.T @ d - np.eye(16))) < 1e-13
    assert np.max(np.abs(d.sum(axis=0))) < 1e-13                        # every column is orthogonal to column 0, the level
    lifted = audio.auditory_tables(22050, 1024, n_ceps=16, lifter=22.0)["dct"]
    i = np.arange(1, 17)
    assert np.allclose(lifted, d * (1.0 + 11.0 * np.sin(np.pi * i / 22.0)), rtol=1e-15, atol=0)


def test_flux_band_in_hz():
    t = audio.auditory_tables(22050, 1024, flux_band=(100.0, 5000.0))
    assert (t["k_lo"], t["k_hi"]) == (5, 233)                           # ceil(100 x 1024 / 22050), ceil(5000 x 1024 / 22050)
    assert audio.auditory_tables(22050, 1024, flux_band=(0.0, 1e6))["k_hi"] == 513


@pytest.mark.parametrize("kw", [dict(n_fft=1000 + 1), dict(n_fft=2048), dict(n_fft=8), dict(sr=0), dict(n_mels=0), dict(n_mels=65), dict(n_ceps=0),
                                dict(n_ceps=17), dict(n_mels=4, n_ceps=4), dict(fmin=-1.0), dict(fmin=9000.0), dict(fmax=12000.0),
                                dict(fmax=float("nan")), dict(lifter=0.5), dict(lifter=float("inf")), dict(flux_band=(500.0, 100.0)),
                                dict(flux_band=(-1.0, None)), dict(flux_band=(11024.9, 11025.0)), dict(n_mels=64, n_fft=128)])
def test_auditory_tables_check_their_arguments_without_a_device(kw):
    args = dict(sr=22050, n_fft=1024)
    args.update(kw)
    with pytest.raises(ValueError, match="auditory_tables"):
        audio.auditory_tables(**args)


# ---- the mutants ------------------------------------------------------------------------------------------------------------------------------
def _mutant_case(name):
    """(x, g, tables): the named case on which the mutant shows."""
    g = R.GEOMETRIES[0]
    if name == "silent_keeps_loudness":
        return np.zeros(400, np.float32), g, R.tables(g)
    if name == "floor_after_log":
        return R.rows_for(g)[0][0, :600], g, R.tables(g, zero_column=2)
    if name == "reflect":
        return R.speech_like(600, seed=3, fs=R.FS) + np.float32(0.01), g, R.tables(g)
    return R.rows_for(g)[0][0, :600], g, R.tables(g)


@pytest.mark.parametrize("name", R.MUTANTS)
def test_each_mutant_moves_its_outputs_and_no_other(name):
    x, g, t = _mutant_case(name)
    ref, mut = R.named(R.row(x, g, t)), R.named(R.row(x, g, t, mutant=name))
    for k in R.OUTPUTS:
        same = np.array_equal(ref[k], mut[k])
        if k in R.MUTANT_MOVES[name]:
            assert not same and R.err(mut[k], ref[k]) > 1e3 * R.TOL, f"{name} leaves {k} where it is"
        else:
            assert same, f"{name} moves {k}"
    if name == "flux_from_frame_minus_one":                             # only frame 0 differs: W > H, so the window before the row reaches into it
        assert g.W > g.H and mut["spectral_flux"][0] > 0 and np.array_equal(mut["spectral_flux"][1:], ref["spectral_flux"][1:])


def test_the_first_silent_frame_has_a_flux_and_no_live_bit():
    g = R.GEOMETRIES[0]
    x = R.going_silent(600, 300)
    r = R.named(R.row(x, g, R.tables(g)))
    silent = np.flatnonzero((r["flags"] & 1) == 0)
    f = int(silent[0])
    assert f >= 2 and r["flags"][f - 1] & 1 and r["spectral_flux"][f] > 0 and r["power"][f] == 0
    assert r["loudness"][f] == 0 and r["log_energy"][f] == 0 and not r["mfcc"][f].any() and not r["bands"][f].any()
    assert r["spectral_flux"][f + 1] == 0 and r["flags"][f + 1] == 2
    one = R.named(R.row(np.full(1, 0.5, np.float32), g, R.tables(g)))
    assert one["flags"].tolist() == [1] and one["spectral_flux"].tolist() == [0.0]


# ---- the statistics and the report family ---------------------------------------------------------------------------------------------------
def _hand_made():
    F = 6
    au = {"loudness": torch.tensor([[1.0, 2.0, 3.0, 0.0, 5.0, 9.0]]), "spectral_flux": torch.tensor([[0.0, 0.5, 1.5, 2.0, 1.0, 9.0]]),
          "power": torch.tensor([[0.1, 0.2, 0.3, 0.0, 0.4, 9.0]]), "log_energy": torch.zeros(1, F),
          "mfcc": torch.arange(F * 4, dtype=torch.float64).reshape(1, F, 4),
          "live": torch.tensor([[True, True, True, False, True, True]]), "has_previous": torch.tensor([[False, True, True, True, True, True]])}
    voiced = torch.tensor([[False, True, True, True, False, True]])
    return au, voiced, [5]


def test_auditory_statistics_on_hand_made_frames():
    au, voiced, n = _hand_made()
    st = audio.auditory_statistics(au, voiced, n)
    assert st["frames"].tolist() == [4]                                 # live and inside: 0, 1, 2, 4
    assert st["used"]["loudness"].tolist() == [4] and st["loudness"].item() == pytest.approx(11.0 / 4)
    assert st["used"]["spectral_flux"].tolist() == [4] and st["spectral_flux"].item() == pytest.approx(5.0 / 4)          # frames 1 .. 4
    assert st["used"]["spectral_flux_voiced"].tolist() == [3] and st["spectral_flux_voiced"].item() == pytest.approx(4.0 / 3)
    assert st["used"]["spectral_flux_unvoiced"].tolist() == [1] and st["spectral_flux_unvoiced"].item() == pytest.approx(1.0)
    assert st["mfcc_2"].item() == pytest.approx((1 + 5 + 9 + 17) / 4) and st["used"]["mfcc_2_voiced"].tolist() == [2]
    assert st["mfcc_2_voiced"].item() == pytest.approx((5 + 9) / 2)
    assert st["used"]["equivalent_level_db"].tolist() == [5] and st["sums"]["equivalent_level_db"].item() == pytest.approx(1.0)
    assert st["equivalent_level_db"].item() == pytest.approx(10 * math.log10(0.2))
    assert tuple(k for k in st["sums"]) == audio.AUDITORY_FIGURES
    one = audio.auditory_statistics({k: v[0] for k, v in au.items()}, voiced[0], n)
    assert one["loudness"].item() == st["loudness"].item()
    with pytest.raises(ValueError, match="auditory_statistics"):
        audio.auditory_statistics(au, voiced[:, :5], n)
    empty = audio.auditory_statistics(au, voiced, [0])
    assert math.isnan(empty["loudness"].item()) and math.isnan(empty["equivalent_level_db"].item()) and empty["frames"].tolist() == [0]


def test_the_report_family_pools_the_level_from_the_power():
    au, voiced, n = _hand_made()
    family = {f.block: f for f in cli.report_families()}["auditory"]
    assert family.figures == audio.AUDITORY_FIGURES and family.frames_key == "auditory_frames" and family.counts == ()
    assert family.report_flag == "auditory" and family.pairs_flag == "auditory"
    rows = cli.family_rows(audio.auditory_statistics(au, voiced, n), family)
    m = cli.family_means(rows, family)
    assert m["equivalent_level_db"] == pytest.approx(10 * math.log10(0.2)) and m["loudness"] == pytest.approx(11.0 / 4) and m["auditory_frames"] == 4
    loud = {"frames": 2, "used": {k: 5 for k in family.figures}, "sums": {k: 10.0 for k in family.figures}}
    both = cli.family_means([rows[0], loud], family)
    assert both["equivalent_level_db"] == pytest.approx(10 * math.log10(11.0 / 10)) and both["auditory_frames"] == 6
    none = cli.family_means([], family)
    assert none == {**{k: None for k in family.figures}, "auditory_frames": 0}
    assert [f.block for f in cli.report_families()][:4] == ["voice", "formants", "perturbation", "harmonics"]
    assert all(f.finish is None for f in cli.report_families()[:4])


def test_cli_flag_is_an_option_of_both_reports():
    p = cli.validate_args
    ns = lambda **kw: type("A", (), dict(dict(sample_rate=None, prepare_dataset=None), **kw))()
    with pytest.raises(AssertionError, match="--auditory is an option of --voice_report and of --evaluate_pairs"):
        p(ns(auditory=True))


def test_auditory_needs_a_device():
    with pytest.raises(Exception):
        audio.auditory(torch.zeros(2000))                               # a CPU tensor: no torch fallback


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_both_calls():
    header = open(os.path.join(REPO, "include", "emojivoice.h")).read()
    for name in ("ev_load_auditory", "ev_auditory"):
        assert re.search(rf"\bint {name}\(ev_handle \*h,", header) and name in _lib.EXPORTS
        assert re.search(rf"{name}\s+<- no counterpart; Eyben et al\. 2016 \(eGeMAPS\) as openSMILE's cMelspec / cMfcc / cPlp / cSpectral", header)
    assert hasattr(_lib.Engine, "load_auditory") and hasattr(_lib.Engine, "auditory")
    assert "not to the digit with openSMILE" in header.replace("NOT", "not")
