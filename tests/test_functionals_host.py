"""The CPU side of ev_functionals: the numpy restatement (tests/functionals_ref.py) against numpy's own percentile, mean and std, float64 against
longdouble on every case of the device test, the mutants, the hand case of the definition, the documented order of the sums, the header and the
exported symbol, audio.functionals' argument checks, and --voice_report --functionals with the device calls stubbed by the restatements.
"""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch

import functionals_ref as R
import voice_stubs
from emojivoice_amd import _lib, audio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return R.cases()


@pytest.fixture(scope="module")
def results(cases):
    return {name: (R.batch(*c), R.batch(*c, dtype=np.longdouble)) for name, c in cases.items()}


# ---- the restatement against numpy ------------------------------------------------------------------------------------------------------------
def test_restatement_against_numpy_on_random_masked_rows_with_ties():
    g = np.random.default_rng(5)
    q = (0.0, 0.05, 0.2, 0.5, 0.8, 0.95, 1.0, 1.0 / 3.0)
    worst = 0.0
    for trial in range(40):
        F = int(g.integers(1, 400))
        v = np.round(20.0 * g.standard_normal(F)) / 4.0 if trial % 2 else 100.0 + np.cumsum(g.standard_normal(F))     # (quarters: many ties)
        mask = (g.uniform(size=F) < 0.7).astype(np.uint8)
        n = int(g.integers(0, F + 1))
        stat, count, _, _ = R.contour(v, mask, n, q)
        u = v[:n][mask[:n] != 0]
        assert count[0] == len(u)
        if not len(u):
            assert not stat[:8].any() and not stat[12:].any()
            continue
        ref = np.concatenate(([u.mean(), u.std(), u.min(), u.max()], np.percentile(u, 100.0 * np.array(q))))
        got = np.concatenate((stat[:4], stat[12:]))
        e = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))
        worst = max(worst, e)
        assert e <= 1e-12, (trial, got, ref)
    print(f"\nfunctionals restatement against numpy: worst relative difference {worst:.3e} (gate 1e-12)")


def test_runs_and_gaps_against_their_lengths():
    flags = np.array([0, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0, 0], np.uint8)          # runs 3, 1, 2; gaps 1, 2, 1, 3 (leading and trailing included)
    stat, count, _, _ = R.contour(np.arange(13.0), flags, 13, ())
    runs, gaps = np.array([3, 1, 2.0]), np.array([1, 2, 1, 3.0])
    assert count[5] == 3 and count[6] == 4 and count[0] == 6 and count[7] == 3
    assert np.allclose(stat[8:12], [runs.mean(), runs.std(), gaps.mean(), gaps.std()], rtol=1e-15, atol=0)
    stat, count, _, _ = R.contour(np.arange(13.0), flags, 9, ())                # the length cuts the last run: runs 3, 1, 1; gaps 1, 2, 1
    assert count[5] == 3 and count[6] == 3 and np.allclose(stat[8:12], [5 / 3, np.std([3, 1, 1]), 4 / 3, np.std([1, 2, 1])], rtol=1e-15, atol=0)
    stat, count, _, _ = R.contour(np.arange(4.0), np.zeros(4, np.uint8), 4, R.Q3)
    assert count.tolist() == [0, 0, 0, 0, 0, 0, 1, 0] and stat[10] == 4.0 and not stat[:10].any() and not stat[11:].any(), "no valid frame: one gap"
    stat, count, _, _ = R.contour(np.arange(4.0), None, 0, R.Q3)
    assert not count.any() and not stat.any(), "a length of 0: nothing at all"


def test_slot_sum_is_the_documented_order():
    g = np.random.default_rng(3)
    for n in (0, 1, 255, 256, 257, 1000, 4096):
        v = g.standard_normal(n) * 10.0 ** g.integers(-8, 8, size=n)
        slots = [0.0] * 256
        for i in range(n):
            slots[i % 256] = slots[i % 256] + v[i]
        groups = []
        for w in range(4):
            lane = slots[64 * w: 64 * w + 64]
            for o in (32, 16, 8, 4, 2, 1):
                lane = [lane[l] + lane[l ^ o] for l in range(64)]
            groups.append(lane[0])
        assert R.slot_sum(v) == ((groups[0] + groups[1]) + groups[2]) + groups[3]
    assert abs(R.slot_sum(np.full(1000, 0.1)) - 100.0) < 1e-12


# ---- the definition's hand case ------------------------------------------------------------------------------------------------------------------
def test_hand_case():
    rise, fall = R.slopes(R.HAND)
    assert rise == [1.0, 3.0, 3.0] and fall == [-1.0, -4.0]
    stat, count, js, t0 = R.contour(R.HAND, None, 9, R.Q3)
    assert count.tolist() == [9, 0, 3, 2, 2, 1, 0, 8]
    assert stat[13] == 2.0 and js[1] == 4 and t0[1], "the median is s_4 = 2"
    assert stat[2] == 1.0 and stat[3] == 5.0 and abs(stat[0] - 22.0 / 9.0) < 1e-15
    assert abs(stat[4] - 7.0 / 3.0) < 1e-15 and abs(stat[5] - np.std([1.0, 3.0, 3.0])) < 1e-15
    assert stat[6] == -2.5 and stat[7] == 1.5 and stat[8] == 9.0 and stat[9] == 0.0 and not stat[10:12].any()
    assert np.allclose(stat[12:], np.percentile(R.HAND, [20, 50, 80]), rtol=1e-15)


def test_gapped_and_nonfinite_cases(cases):
    v, m, lens, q = cases["gapped"]
    stat, count, _, _ = R.contour(v[0, 0], m[0, 0], 7, q)
    assert count.tolist() == [4, 0, 2, 0, 0, 2, 3, 2] and stat[4] == 1.0 and stat[5] == 0.0, "a gap ends a part: (1, 2) and (3, 4) rise on their own"
    v, m, lens, q = cases["nonfinite"]
    stat, count, _, _ = R.contour(v[0, 0], m[0, 0], v.shape[2], q)
    assert count[1] == 5 and count[0] == v.shape[2] - 6, "five non-finite values under the mask are dropped; the sixth lies under a zero byte"
    assert count[5] == 5 and count[6] == 5, "runs 0-4, 6-39, 42-63, 65-89, 91-128; gaps at 5, 40-41, 64, 90, 129"
    assert np.isfinite(stat).all()
    stat, count, _, _ = R.contour(v[1, 1], m[1, 1], v.shape[2], q)
    assert count.tolist() == [0, v.shape[2], 0, 0, 0, 0, 1, 0]


# ---- float64 against longdouble, and the mutants ----------------------------------------------------------------------------------------------------
def test_float64_and_longdouble_agree_on_every_case(cases, results):
    worst = 0.0
    for name, (r64, rld) in results.items():
        assert np.array_equal(r64["count"], rld["count"]), f"{name}: counts"
        e = R.err(r64["stat"], rld["stat"].astype(np.float64))
        worst = max(worst, e)
        assert np.isfinite(r64["stat"]).all() and e <= 1e-12, f"{name}: float64 against longdouble {e:.3e}"
    print(f"\nfunctionals float64 against longdouble: worst {worst:.3e} over {len(results)} cases (gate 1e-12)")


def test_the_cases_cover_what_the_device_test_lists(cases, results):
    assert {f"F{F}" for F in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)} <= set(cases)
    for name, (v, m, lens, q) in cases.items():
        B, K, F = v.shape
        assert F <= 4096 and ((B <= 3 and K <= 4) or name in ("batch516", "lengths")) and (F < 4096 or B == K == 1), name
    assert cases["batch516"][0].shape == (3, 20, 516) and cases["ramp4096"][0].shape == (1, 1, 4096)
    assert results["ramp4096"][0]["count"][0, 0].tolist() == [4096, 0, 0, 1, 0, 1, 0, 4095], "one falling part over all 4096 frames"
    assert cases["lengths"][2] == [0, 1, 65, 66, -1] and not results["lengths"][0]["stat"][[0, 3, 4]].any() and not results["lengths"][0]["count"][[0, 3, 4]].any()
    assert results["lengths"][0]["count"][1, 0].tolist() == [1, 0, 0, 0, 0, 1, 0, 0]
    assert sorted(len(c[3]) for c in cases.values())[0] == 0 and {1, 3, 16} <= {len(c[3]) for c in cases.values()}
    assert {0.0, 1.0, 0.5} <= set(R.Q16) and len(R.Q16) == 16
    assert any(c[1] is None and c[2] is None for c in cases.values())
    ct = np.concatenate([r64["count"].reshape(-1, 8) for r64, _ in results.values()])
    st = np.concatenate([r64["stat"][..., :12].reshape(-1, 12) for r64, _ in results.values()])
    assert ((ct[:, 0] > 1) & (ct[:, 7] == 0)).any(), "an alternating mask: valid frames without an adjacent pair"
    assert ((ct[:, 0] > 2) & (ct[:, 2] + ct[:, 3] == 0) & (ct[:, 7] > 0) & (st[:, 1] == 0)).any(), "a constant contour: no parts"
    assert (ct[:, 0] == 0).any() and (ct[:, 4] > 3).any() and (ct[:, 1] > 0).any()
    t0 = np.concatenate([r64["t0"].reshape(-1) for r64, _ in results.values()])
    assert t0.any() and not t0.all(), "percentiles that are values and percentiles that interpolate"


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_changes_its_named_output_on_its_named_case(cases, results, mutant):
    name, bk, what = R.MUTANT_SHOWS[mutant]
    good = R.output(results[name][0], bk, what)
    bad = R.output(R.batch(*cases[name], mutant=mutant), bk, what)
    print(f"\nfunctionals mutant {mutant}: {what} of {name}{bk} {good} -> {bad}")
    assert bad != good and (what in R.COUNT or abs(float(bad) - float(good)) > 1e-6 * max(1.0, abs(float(good))))


def test_every_mutant_is_listed():
    assert set(R.MUTANT_SHOWS) == set(R.MUTANTS) and len(R.MUTANTS) == 7


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_ev_functionals():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    assert re.search(r"\bint ev_functionals\(ev_handle \*h,", header) and "ev_functionals" in _lib.EXPORTS
    assert "ev_functionals" in re.search(r"#define EV_ABI_VERSION 4 .*", header).group(0), "the additions list of the ABI line"
    for word in ("DROPPED", "ADJACENT", "i mod 256", "s_j + t (s_{min(j+1, k-1)} - s_j)", "N S2 - S1 S1", "u_i >= u_{i+1}", "1 <= F <= 4096"):
        assert word in header, word
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, "ev_functionals") and lib.ev_abi_version() == 4


# ---- audio.functionals' arguments ------------------------------------------------------------------------------------------------------------------------
def test_functional_arguments():
    v = torch.zeros(2, 3, 50, dtype=torch.float32)
    (B, K, F), q = audio.functional_arguments(v, torch.ones(2, 1, 50, dtype=torch.bool), [50, 20])
    assert (B, K, F) == (2, 3, 50) and q.tolist() == [0.2, 0.5, 0.8]
    assert audio.functional_arguments(torch.zeros(7, dtype=torch.float64))[0] == (1, 1, 7)
    assert audio.functional_arguments(torch.zeros(4, 7), percentiles=())[0] == (4, 1, 7)
    for bad, word in ((dict(values=torch.zeros(2, 3, 4, 5)), "values must be"), (dict(values=torch.zeros(2, 5, dtype=torch.int32)), "values must be"),
                      (dict(values=np.zeros((2, 5))), "values must be"), (dict(values=torch.zeros(2, 4097)), "F=4097"),
                      (dict(values=torch.zeros(2, 0)), "F=0"), (dict(values=v, percentiles=(20, 50, 80)), "percentiles"),
                      (dict(values=v, percentiles=(0.5, float("nan"))), "percentiles"), (dict(values=v, percentiles=(-0.1,)), "percentiles"),
                      (dict(values=v, percentiles=[0.5] * 17), "at most 16"), (dict(values=v, mask=torch.ones(2, 3, 49)), "mask"),
                      (dict(values=v, mask=torch.ones(1, 2, 3, 50)), "mask"), (dict(values=v, lengths=[50, 20, 10]), "2 lengths expected")):
        with pytest.raises(ValueError, match=word):
            audio.functional_arguments(**bad)
    with pytest.raises(_lib.EvLibraryError, match="no CPU fallback"):
        audio.functionals(v)
    with pytest.raises(ValueError, match="F=4097"):
        audio.functionals(torch.zeros(1, 4097))
    assert len(audio.FUNCTIONAL_STATISTICS) == 12 and len(audio.FUNCTIONAL_COUNTS) == 8 and set(audio._FUNCTIONAL_BEHIND) == set(audio.FUNCTIONAL_STATISTICS)


# ---- the layers above, with the device calls stubbed by the restatements ----------------------------------------------------------------------------------
ref_functionals = voice_stubs.ref_functionals


def test_voice_functionals_masks_are_those_of_the_statistics_functions(monkeypatch):
    """Hand-made contours on the host: every contour's mean is the mean of its *_statistics function, the slopes are per second, the segments come
    from the voicing's runs and gaps."""
    monkeypatch.setattr(audio, "functionals", ref_functionals)
    g = torch.Generator().manual_seed(4)
    B, F = 3, 60
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    voiced = rnd(B, F) < 0.7
    voiced[2] = False
    pitch = {"f0": (100.0 + 50.0 * rnd(B, F)).float() * voiced, "voiced": voiced}
    n = [60, 41, 30]
    vq = {k: rnd(B, F) for k in audio.VOICE_QUALITY_FIGURES}
    vq["peak_quefrency"] = (rnd(B, F) < 0.8).int() * 90
    fm = {"frequency": 500.0 + 2000.0 * rnd(B, F, 4), "bandwidth": 1000.0 * rnd(B, F, 4), "count": (5.0 * rnd(B, F)).int() - 1}
    pt = {k: rnd(B, F) for k in ("jitter", "rap", "shimmer", "shimmer_db", "r")}
    pt["count"] = (3.0 * rnd(B, F, 4)).int()
    pt["lag"] = (rnd(B, F) < 0.9).int() * 100
    hm = {k: rnd(B, F) for k in audio.HARMONIC_FIGURES}
    hm["flags"] = (32.0 * rnd(B, F)).int()
    vf = audio.voice_functionals(pitch, vq, n, fm=fm, pt=pt, hm=hm)
    assert vf["contours"] == ("f0_semitones",) + audio.VOICE_QUALITY_FIGURES + audio.FORMANT_FIGURES + audio.PERTURBATION_FIGURES + audio.HARMONIC_FIGURES
    sts = (audio.voice_quality_statistics(vq, voiced, n), audio.formant_statistics(fm, voiced, n),
           audio.perturbation_statistics(pt, voiced & (pt["lag"] > 0), n), audio.harmonic_statistics(hm, voiced, n, fm=fm))
    checked = 0
    for st, figs in zip(sts, (audio.VOICE_QUALITY_FIGURES, audio.FORMANT_FIGURES, audio.PERTURBATION_FIGURES, audio.HARMONIC_FIGURES)):
        for k in figs:
            a, b = vf[k]["mean"], st[k]
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and bool(torch.isnan(a[2])), k
            ok = ~torch.isnan(b)
            assert bool(((a[ok] - b[ok]).abs() <= 1e-12 * b[ok].abs()).all()), k
            checked += int(ok.sum())
    assert checked == 2 * 21
    inside = voiced & (torch.arange(F)[None] < torch.tensor(n)[:, None])
    for b in range(2):
        st = 12.0 * torch.log2(pitch["f0"][b][inside[b]].double() / 27.5)
        assert abs(float(vf["f0_semitones"]["mean"][b]) - float(st.mean())) < 1e-12 * float(st.mean())
        assert int(vf["f0_semitones"]["valid"][b]) == int(inside[b].sum())
        runs, gaps, _, _ = R.stretches(inside[b, :n[b]].numpy())
        rate = 22050.0 / 256.0
        seg = vf["segments"]
        assert abs(float(seg["voiced_per_s"][b]) - len(runs) / (n[b] / rate)) < 1e-12 and abs(float(seg["voiced_mean_s"][b]) - np.mean(runs) / rate) < 1e-12
        assert abs(float(seg["unvoiced_sd_s"][b]) - np.std(gaps) / rate) < 1e-12
        raw = ref_functionals(12.0 * torch.log2(torch.where(inside[b], pitch["f0"][b].double(), torch.tensor(27.5, dtype=torch.float64)) / 27.5)[None], inside[b][None], [n[b]])
        assert abs(float(vf["f0_semitones"]["rise_mean"][b]) - rate * float(raw["rise_mean"][0, 0])) < 1e-9, "slopes are per second"
        assert abs(float(vf["f0_semitones"]["peaks_per_s"][b]) - int(raw["peaks"][0, 0]) / (n[b] / rate)) < 1e-12
    assert bool(torch.isnan(vf["f0_semitones"]["mean"][2])) and bool(torch.isnan(vf["segments"]["voiced_mean_s"][2])) and float(vf["segments"]["voiced_per_s"][2]) == 0.0
    assert abs(float(vf["segments"]["unvoiced_mean_s"][2]) - 30 / (22050.0 / 256.0)) < 1e-12, "an unvoiced row is one gap of its own length"
    few = audio.voice_functionals(pitch, vq, n)
    assert few["contours"] == ("f0_semitones",) + audio.VOICE_QUALITY_FIGURES and torch.equal(few["cpp_db"]["sd"][:2], vf["cpp_db"]["sd"][:2])


def test_voice_report_functionals_json_shape_and_validate_args(tmp_path, monkeypatch):
    import perturbation_ref as P
    from emojivoice_amd import cli

    wavs = {"a.wav": P.perturbed_pulses(6000, 120.0, 0.01, 0.05, seed=20), "b.wav": P.perturbed_pulses(5000, 150.0, 0.005, 0.1, seed=21),
            "c.wav": np.zeros(3000, np.float32)}
    flist = voice_stubs.filelist(tmp_path, wavs)
    voice_stubs.base(monkeypatch, wavs)
    monkeypatch.setattr(audio, "functionals", ref_functionals)
    ns = lambda **kw: argparse.Namespace(voice_report=str(flist), batch_size=2, sample_rate=None, prepare_dataset=None, **kw)
    plain = cli.voice_report(cli.validate_args(ns()), "cpu")
    rep = cli.voice_report(cli.validate_args(ns(functionals=True)), "cpu")
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    extra = {"functionals", "segments"}
    assert saved == json.loads(json.dumps(rep)) and set(saved) == set(plain) == {"sample_rate", "hop_length", "files", "speakers", "overall"}
    old = {"path", "speaker", "seconds", "frames", "voiced_frames"} | set(audio.VOICE_QUALITY_FIGURES)
    assert [set(f_) for f_ in plain["files"]] == [old] * 3 and [set(f_) for f_ in saved["files"]] == [old | extra] * 3
    assert set(plain["overall"]) | extra == set(saved["overall"]) == set(saved["speakers"]["7"]) and not extra & set(plain["overall"])
    assert all(saved["files"][i][k] == plain["files"][i][k] for i in range(3) for k in old), "the flag changes none of the other figures"
    contours = ["f0_semitones"] + list(audio.VOICE_QUALITY_FIGURES)
    a, b, c = saved["files"]
    for f_ in saved["files"]:
        assert list(f_["functionals"]) == contours and all(tuple(v) == cli.FUNCTIONAL_REPORT_KEYS for v in f_["functionals"].values())
        assert tuple(f_["segments"]) == cli.SEGMENT_REPORT_KEYS
    assert tuple(cli.FUNCTIONAL_REPORT_KEYS) == ("mean", "sd", "p20", "p50", "p80", "range", "rise_mean", "rise_sd", "fall_mean", "fall_sd", "peaks_per_s")
    assert all(c["functionals"][k][s] is None for k in contours for s in cli.FUNCTIONAL_REPORT_KEYS if s != "peaks_per_s"), "a silent file has nulls"
    assert c["segments"]["voiced_per_s"] == 0.0 and c["segments"]["voiced_mean_s"] is None and c["segments"]["unvoiced_mean_s"] is not None
    for f_ in (a, b):
        for k in audio.VOICE_QUALITY_FIGURES:
            assert abs(f_["functionals"][k]["mean"] - f_[k]) <= 1e-12 * abs(f_[k]), "the functionals' mean is the report's own mean"
        st = f_["functionals"]["f0_semitones"]
        assert st["p20"] <= st["p50"] <= st["p80"] and abs(st["range"] - (st["p80"] - st["p20"])) < 1e-12 and st["sd"] >= 0.0
    assert 12.0 * np.log2(110.0 / 27.5) < a["functionals"]["f0_semitones"]["p50"] < 12.0 * np.log2(130.0 / 27.5)
    s7, s12, ov = saved["speakers"]["7"], saved["speakers"]["12"], saved["overall"]
    for k in contours:
        for s in cli.FUNCTIONAL_REPORT_KEYS:
            va, vb = a["functionals"][k][s], b["functionals"][k][s]
            have = [v for v in (va, vb) if v is not None]
            got = s7["functionals"][k][s]
            assert set(got) == {"mean", "files"} and got["files"] == len(have)
            assert (got["mean"] is None and not have) or abs(got["mean"] - sum(have) / len(have)) <= 1e-12 * max(1.0, abs(got["mean"])), "the plain mean over the files"
            if s != "peaks_per_s":
                assert s12["functionals"][k][s] == {"mean": None, "files": 0} and ov["functionals"][k][s] == got
    assert ov["segments"]["voiced_per_s"]["files"] == 3 and s7["segments"]["voiced_mean_s"]["files"] == 2 and s12["segments"]["voiced_mean_s"] == {"mean": None, "files": 0}
    with pytest.raises(AssertionError, match="--functionals"):
        cli.validate_args(argparse.Namespace(functionals=True, evaluate_pairs="pairs.txt", voice_report=None, batch_size=2, sample_rate=None, prepare_dataset=None))
    with pytest.raises(AssertionError, match="--functionals"):
        cli.validate_args(argparse.Namespace(functionals=True, evaluate_pairs=None, voice_report=None, sample_rate=None, prepare_dataset=None))
    cli.validate_args(ns(functionals=True, formants=True, perturbation=True, harmonics=True, pitch_method="pyin"))


def test_voice_report_with_every_flag_is_the_single_flag_reports_side_by_side(tmp_path, monkeypatch):
    """Every file's, every speaker's and the overall record of a run with all flags is, key for key and in key order, the plain record followed by
    the blocks of --formants, --perturbation, --harmonics and --functionals as each single-flag run writes them (the functionals block gains contours
    with each flag: there the single-flag run's contours are compared), and audio.formants runs once per batch."""
    import perturbation_ref as P
    from emojivoice_amd import cli

    wavs = {"a.wav": P.perturbed_pulses(6000, 120.0, 0.01, 0.05, seed=20), "b.wav": P.perturbed_pulses(5000, 150.0, 0.005, 0.1, seed=21),
            "c.wav": np.zeros(3000, np.float32)}
    flist = voice_stubs.filelist(tmp_path, wavs)
    voice_stubs.base(monkeypatch, wavs)
    _, calls = voice_stubs.flat_formants(monkeypatch)
    voice_stubs.perturbation(monkeypatch)
    voice_stubs.harmonics(monkeypatch)
    monkeypatch.setattr(audio, "functionals", ref_functionals)
    run = lambda **kw: cli.voice_report(cli.validate_args(argparse.Namespace(voice_report=str(flist), batch_size=2, sample_rate=None, prepare_dataset=None, **kw)), "cpu")
    records = lambda rep: rep["files"] + list(rep["speakers"].values()) + [rep["overall"]]
    flags = ("formants", "perturbation", "harmonics", "functionals")
    plain = run()
    single = {flag: run(**{flag: True}) for flag in flags}
    before = calls["formants"]
    every = run(**{flag: True for flag in flags})
    assert calls["formants"] - before == 2, "two batches: the formants are analysed once per batch for --formants, --harmonics and --functionals"
    with open(f"{flist}.voice.json") as f:
        assert json.load(f) == json.loads(json.dumps(every))
    assert list(every) == list(plain) and list(every["speakers"]) == list(plain["speakers"]) == ["7", "12"] and len(records(every)) == 6
    contours = ("f0_semitones",) + audio.VOICE_QUALITY_FIGURES + audio.FORMANT_FIGURES + audio.PERTURBATION_FIGURES + audio.HARMONIC_FIGURES
    for i, (got, base) in enumerate(zip(records(every), records(plain))):
        want = dict(base)
        for flag in flags:
            one = records(single[flag])[i]
            assert list(one)[:len(base)] == list(base) and all(one[k] == base[k] for k in base), "a single flag appends its block to the plain record"
            assert len(one) > len(base) and not (set(one) - set(base)) & set(want), "no two flags write the same key"
            want.update({k: v for k, v in one.items() if k not in base})
        assert list(got) == list(want), i
        assert all(got[k] == want[k] for k in want if k != "functionals"), i
        assert tuple(got["functionals"]) == contours and list(want["functionals"]) == list(contours[:6])
        assert {c: got["functionals"][c] for c in want["functionals"]} == want["functionals"], i
        assert all(tuple(v) == cli.FUNCTIONAL_REPORT_KEYS for v in got["functionals"].values())
    for flag, own in zip(flags[:3], (audio.FORMANT_FIGURES, audio.PERTURBATION_FIGURES, audio.HARMONIC_FIGURES)):    # the contours a flag brings
        both = run(**{flag: True, "functionals": True})
        for got, part in zip(records(every), records(both)):
            assert tuple(part["functionals"]) == contours[:6] + own and all(got["functionals"][c] == part["functionals"][c] for c in own), flag
