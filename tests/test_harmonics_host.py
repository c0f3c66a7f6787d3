"""ev_harmonics on the host: the numpy restatement (tests/harmonics_ref.py) against its mutants and against the closed form on harmonic
complexes, audio.harmonic_statistics, the CLI helpers, the key sets of --voice_report / --evaluate_pairs with and without --harmonics (the
device calls replaced by the restatements), every ValueError, and the header.  No GPU.

Closed form.  A complex of partials h f0 with known amplitudes a_h has H1-H2 = 20 log10(a_1 / a_2) and rel_i = 20 log10(a_{h_i} / a_1).  Measured
on the cases of ``complexes`` (f0 110 / 150 / 220 / 330 Hz at 1024 / 256 / 22050, partials to 4 kHz at a_h = 0.1 / h with a further tilt of 0, 0.5
and 1 dB per harmonic, 1e-4 rms noise, F_i = 520 / 1480 / 2530 Hz; the frames whose window lies inside the row): the restatement's worst H1-H2
error is 0.191 dB (220 Hz: what a parabola through three dB values leaves of a Hann main lobe whose peak lies between two bins) and its worst rel_i
error 0.545 dB (harmonic 23 of 110 Hz under 1 dB of tilt per harmonic, 49 dB under H1).  The gates are twice the measured figures and never
looser than 1 dB: CLOSED_GATE_H1H2 = 0.39 dB, CLOSED_GATE_REL = 1.0 dB (twice 0.545 would be 1.09).
"""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch

import harmonics_ref as R
import voice_stubs
from emojivoice_amd import _lib, audio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = R.GEOMETRIES[3]                                                       # 1024 / 256 / 1024 at 22050 Hz
CLOSED_F0 = (110.0, 150.0, 220.0, 330.0)
CLOSED_TILTS = (0.0, 0.5, 1.0)
CLOSED_GATE_H1H2, CLOSED_GATE_REL = R.CLOSED_GATE_H1H2, R.CLOSED_GATE_REL   # dB: 0.39 (twice the measured 0.191) and 1.0 (twice 0.545 is 1.09)
CLOSED_FORMANTS = (520.0, 1480.0, 2530.0)


def complex_row(f0, tilt_db, n=6000, seed=0):
    """(x float32, a (n_partials,)): partials h f0 <= 4 kHz at amplitude a_h = 0.1 10^(-tilt_db (h - 1) / 20) / h, 1e-4 rms noise."""
    rng = np.random.default_rng(300 + seed)
    t = np.arange(n, dtype=np.float64) / R.FS
    nh = int(4000.0 // f0)
    a = np.array([0.1 * 10.0 ** (-tilt_db * (h - 1) / 20.0) / h for h in range(1, nh + 1)])
    x = sum(a[h - 1] * np.sin(2 * np.pi * h * f0 * t + 0.37 * h * h) for h in range(1, nh + 1)) + 1e-4 * rng.standard_normal(n)
    return x.astype(np.float32), a


def complexes():
    for i, f0 in enumerate(CLOSED_F0):
        for j, tilt in enumerate(CLOSED_TILTS):
            yield f0, tilt, complex_row(f0, tilt, seed=4 * i + j)


def closed_form_errors():
    """(worst H1-H2 error, worst rel_i error) in dB over the cases, over the frames whose window lies inside the row."""
    e12, erel = 0.0, 0.0
    for f0, tilt, (x, a) in complexes():
        nf = R.frames(len(x), G.H)
        period = np.full(nf, R.FS / f0, np.float32)
        formant = np.zeros((nf, 3, 2))
        formant[:, :, 0] = CLOSED_FORMANTS
        r = R.row(x, period, G, formant, np.full(nf, 3, np.int32))
        inner = slice(2, nf - 3)
        assert (r["count"][inner, 1] & 15 == 15).all(), "H1-H2 and the three rel_i are valid on every inner frame"
        e12 = max(e12, np.abs(r["frame"][inner, 0] - 20 * np.log10(a[0] / a[1])).max())
        for i, F in enumerate(CLOSED_FORMANTS):
            h = int(r["hidx"][inner, i][0])
            assert (r["hidx"][inner, i] == h).all() and abs(h - F / f0) <= 0.5 + 1e-3, "the harmonic nearest F_i"
            erel = max(erel, np.abs(r["frame"][inner, 2 + i] - 20 * np.log10(a[h - 1] / a[0])).max())
    return float(e12), float(erel)


def test_restatement_against_the_closed_form_on_harmonic_complexes():
    e12, erel = closed_form_errors()
    print(f"\nharmonics closed form: worst H1-H2 error {e12:.3f} dB (gate {CLOSED_GATE_H1H2}), worst rel_i error {erel:.3f} dB (gate {CLOSED_GATE_REL})")
    assert CLOSED_GATE_H1H2 <= 1.0 and CLOSED_GATE_REL <= 1.0
    assert e12 <= CLOSED_GATE_H1H2 and erel <= CLOSED_GATE_REL


def test_unresolved_spacing_is_what_the_limit_says():
    """At 3.25 bins between harmonics (f0 70 Hz at 1024 / 22050) the merged peaks put H1-H2 off by more than at 4.1 bins up: the evidence for
    min_spacing = 4."""
    def worst(f0, g):
        x, a = complex_row(f0, 0.0, seed=50)
        nf = R.frames(len(x), g.H)
        r = R.row(x, np.full(nf, R.FS / f0, np.float32), g)
        return np.abs(r["frame"][2:nf - 3, 0] - 20 * np.log10(a[0] / a[1])).max()
    loose = G._replace(min_spacing=2.0)
    e325, e41 = worst(70.0, loose), worst(88.3, loose)
    print(f"\nharmonics resolution: H1-H2 error {e325:.2f} dB at 3.25 bins, {e41:.2f} dB at 4.1 bins")
    assert e325 > 2 * e41 and e41 <= 0.5
    x, _ = complex_row(70.0, 0.0, seed=50)
    r = R.row(x, np.full(R.frames(len(x), G.H), R.FS / 70.0, np.float32), G)
    assert not r["count"].any() and not r["frame"][:, :7].any() and (r["frame"][:, 7] > 3.2).all(), "UNRESOLVED keeps v alone"


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------------
def test_each_mutant_moves_a_figure():
    x, lens, period, formant, fcount = R.case(G)
    base = R.batch(x, lens, period, G, formant, fcount)
    xt, T = R.tie_row(G)
    pt = np.full((1, R.frames(len(xt), G.H)), T, np.float32)
    base_t = R.batch(xt[None], None, pt, G)
    assert (base_t["margin"] == 0).any(), "the tie row holds ties"
    assert len(R.MUTANTS) >= 6
    for m in R.MUTANTS:
        o, ot = R.batch(x, lens, period, G, formant, fcount, mutant=m), R.batch(xt[None], None, pt, G, mutant=m)
        moved = max(np.abs(o[k] - base[k]).max() for k in ("frame", "harm"))
        moved_t = max(np.abs(ot[k] - base_t[k]).max() for k in ("frame", "harm"))
        print(f"harmonics mutant {m}: moves a figure by {moved:.3e} on the ragged rows, {moved_t:.3e} on the tie row")
        assert max(moved, moved_t) > 1e-6, m


def test_conditions_hold_on_every_case_of_the_gpu_tests():
    """What tests/test_gpu_harmonics.py asserts first, here on the CPU: float64 against longdouble, equal decisions, margins, roundings; and
    the census the issue asks of the rows."""
    lanes = np.zeros(5, np.int64)
    worst = np.inf
    for g in R.GEOMETRIES + R.EDGE_GEOMETRIES:
        x, lens, period, formant, fcount = R.case(g)
        assert [R.frames(n, g.H) % 16 for n in lens] == [15, 0, 1] and (x[0, lens[0]:] == R.GARBAGE).all()
        _, rep = R.conditions(x, lens, period, g, formant, fcount)
        print(f"harmonics {tuple(g)[:5]}: {rep}")
        assert rep["input_err"] <= R.INPUT_TOL and rep["decisions_equal"]
        assert rep["min_margin"] >= R.MIN_PEAK_MARGIN and rep["min_rounding"] >= R.MIN_ROUND_MARGIN
        assert rep["voiced"] and rep["unvoiced"] and rep["unresolved"] and rep["silent"]
        lanes += rep["lanes"]
        worst = min(worst, rep["min_margin"])
    assert lanes[0] and lanes[1] and lanes[4], "lanes with 0, 1 and 4 harmonics"
    cut = [R.conditions(*R.case(g)[:3], g, *R.case(g)[3:])[1] for g in R.GEOMETRIES[2:4]]
    assert any(c["cut_by_n_harm"] for c in cut) and any(c["cut_by_nyquist"] for c in cut)
    print(f"harmonics: the smallest margin over all cases {worst:.2e} dB")


def test_invariances_of_the_restatement():
    x, lens, period, formant, fcount = R.case(R.GEOMETRIES[0])
    g = R.GEOMETRIES[0]
    full = R.batch(x, lens, period, g, formant, fcount)
    nof = R.batch(x, lens, period, g)
    for i in (0, 5, 6, 7):
        assert np.array_equal(full["frame"][..., i], nof["frame"][..., i])
    assert not nof["frame"][..., 1:5].any() and np.array_equal(nof["count"][..., 1], full["count"][..., 1] & 1) and np.array_equal(nof["harm"], full["harm"])
    assert (full["count"][..., 1] & 16).any() and (full["count"][..., 1] & 2).any()
    n = lens[0]
    nf = R.frames(n, g.H)
    alone = R.batch(x[:1, :n], None, period[:1, :nf], g, formant[:1, :nf], fcount[:1, :nf])
    assert all(np.array_equal(alone[k][0], full[k][0, :nf]) for k in ("frame", "count", "harm"))
    assert not full["frame"][0, nf:].any() and not full["count"][0, nf:].any()
    bad = R.batch(x, [0, x.shape[1] + 1, lens[2]], period, g, formant, fcount)
    assert not bad["frame"][:2].any() and not bad["count"][:2].any() and np.array_equal(bad["frame"][2], full["frame"][2])


# ---- the host side -----------------------------------------------------------------------------------------------------------------------------------
def _hand_made(B=3, F=40, seed=5):
    g = np.random.default_rng(seed)
    hm = {k: torch.from_numpy(g.uniform(-20.0, 20.0, (B, F))) for k in audio.HARMONIC_FIGURES}
    hm["flags"] = torch.from_numpy(g.integers(0, 32, (B, F)).astype(np.int32))
    voiced = g.random((B, F)) < 0.7
    voiced[2] = False
    fm = {"bandwidth": torch.from_numpy(g.uniform(50.0, 1200.0, (B, F, 4)))}
    return hm, voiced, fm


def test_harmonic_statistics_against_hand_made_tensors():
    hm, voiced, fm = _hand_made()
    B, F = voiced.shape
    lens = [40, 23, 40]
    use = voiced & (np.arange(F)[None, :] < np.array(lens)[:, None])
    flags, bw = hm["flags"].numpy(), fm["bandwidth"].numpy()
    bit = {"h1_h2_db": 1, "f1_rel_db": 2, "f2_rel_db": 4, "f3_rel_db": 8, "h1_a3_db": 16}
    col = {"f1_rel_db": 0, "f2_rel_db": 1, "f3_rel_db": 2, "h1_a3_db": 2}
    assert tuple(audio.HARMONIC_FIGURES) == ("h1_h2_db", "h1_a3_db", "f1_rel_db", "f2_rel_db", "f3_rel_db")
    for with_fm in (False, True):
        st = audio.harmonic_statistics(hm, torch.from_numpy(voiced), lengths=lens, fm=fm if with_fm else None, max_bandwidth=700.0)
        assert st["frames"].tolist() == use.sum(axis=1).tolist() and st["frames"].dtype == torch.int64 and st["frames"][2] == 0
        for name in audio.HARMONIC_FIGURES:
            ok = use & ((flags & bit[name]) != 0)
            if with_fm and name in col:
                ok &= bw[:, :, col[name]] <= 700.0
            v = hm[name].numpy()
            assert st["used"][name].tolist() == ok.sum(axis=1).tolist()
            assert st[name].dtype == torch.float64 and torch.isnan(st[name][2]) and float(st["sums"][name][2]) == 0.0
            for b in range(2):
                assert abs(float(st[name][b]) - v[b][ok[b]].mean()) < 1e-9 and abs(float(st["sums"][name][b]) - v[b][ok[b]].sum()) < 1e-8
            assert (ok.sum(axis=1) < use.sum(axis=1))[:2].all(), "frames without the figure's flag are left out"
    one = audio.harmonic_statistics({k: v[0] for k, v in hm.items()}, torch.from_numpy(voiced[0]))
    assert one["frames"].tolist() == [int(voiced[0].sum())]


def test_every_value_error():
    hm, voiced, fm = _hand_made()
    with pytest.raises(ValueError, match="harmonic_statistics"):
        audio.harmonic_statistics(hm, torch.from_numpy(voiced[:, :5]))
    with pytest.raises(ValueError, match="harmonic_statistics"):
        audio.harmonic_statistics(hm, torch.from_numpy(voiced), lengths=[1, 2])
    with pytest.raises(ValueError, match="bandwidths"):
        audio.harmonic_statistics(hm, torch.from_numpy(voiced), fm={"bandwidth": fm["bandwidth"][:, :, :2]})
    with pytest.raises(ValueError, match="bandwidths"):
        audio.harmonic_statistics(hm, torch.from_numpy(voiced), fm={"bandwidth": fm["bandwidth"][:, :7]})
    for kw, word in ((dict(n_harm=0), "n_harm"), (dict(n_harm=65), "n_harm"), (dict(search=0.0), "search"), (dict(search=0.51), "search"),
                     (dict(min_spacing=1.9), "min_spacing"), (dict(min_spacing=float("inf")), "min_spacing"), (dict(min_spacing=float("nan")), "min_spacing"),
                     (dict(a3_range=-0.1), "a3_range"), (dict(a3_range=0.6), "a3_range")):
        with pytest.raises(ValueError, match=word):
            audio.harmonic_arguments(**kw)
    audio.harmonic_arguments()
    with pytest.raises(ValueError, match="harmonics: y must be"):
        audio.harmonics(np.zeros(100, np.float32))
    with pytest.raises(ValueError, match="harmonics: y must be"):
        audio.harmonics(torch.zeros(2, 3, 4))
    with pytest.raises(_lib.EvLibraryError, match="harmonics runs on a ROCm GPU only"):
        audio.harmonics(torch.zeros(100))


def test_cli_helpers_on_hand_made_rows():
    from emojivoice_amd import cli

    figs = audio.HARMONIC_FIGURES
    st = {"frames": torch.tensor([5, 0]), "used": {k: torch.tensor([i + 1, 0]) for i, k in enumerate(figs)},
          "sums": {k: torch.tensor([2.0 * (i + 1), 0.0], dtype=torch.float64) for i, k in enumerate(figs)}}
    family = {f.block: f for f in cli.report_families()}["harmonics"]
    assert family.figures == figs and family.frames_key == "harmonic_frames" and family.counts == ()
    rows = cli.family_rows(st, family)
    assert rows == [{"frames": 5, "used": {k: i + 1 for i, k in enumerate(figs)}, "sums": {k: 2.0 * (i + 1) for i, k in enumerate(figs)}},
                    {"frames": 0, "used": {k: 0 for k in figs}, "sums": {k: 0.0 for k in figs}}]
    assert cli.family_means(rows[:1], family) == {**{k: 2.0 for k in figs}, "harmonic_frames": 5}
    assert cli.family_means(rows[1:], family) == {**{k: None for k in figs}, "harmonic_frames": 0}
    other = {"frames": 3, "used": {k: 1 for k in figs}, "sums": {k: -4.0 for k in figs}}
    m = cli.family_means([rows[0], other, rows[1]], family)
    assert m["harmonic_frames"] == 8 and all(abs(m[k] - (2.0 * (i + 1) - 4.0) / (i + 2)) < 1e-12 for i, k in enumerate(figs))
    assert cli.family_means([], family) == {**{k: None for k in figs}, "harmonic_frames": 0}


def test_cli_helpers_on_hand_made_formant_rows():
    """The same hand-made case for the formants family: unconverged_frames is summed, and f_i and b_i share used[:, i]."""
    from emojivoice_amd import cli

    figs = audio.FORMANT_FIGURES
    family = {f.block: f for f in cli.report_families()}["formants"]
    assert family.figures == figs and family.frames_key == "formant_frames" and family.counts == ("unconverged_frames",)
    st = {"frames": torch.tensor([5, 0]), "unconverged_frames": torch.tensor([2, 1]), "used": torch.tensor([[1, 2, 4], [0, 0, 0]]),
          "sums": {k: torch.tensor([3.0 * (i + 1), 0.0], dtype=torch.float64) for i, k in enumerate(figs)}}
    used = {k: (1, 2, 4)[int(k[1]) - 1] for k in figs}
    rows = cli.family_rows(st, family)
    assert rows == [{"frames": 5, "unconverged_frames": 2, "used": used, "sums": {k: 3.0 * (i + 1) for i, k in enumerate(figs)}},
                    {"frames": 0, "unconverged_frames": 1, "used": {k: 0 for k in figs}, "sums": {k: 0.0 for k in figs}}]
    assert used["f2_hz"] == used["b2_hz"] == 2 and used["f3_hz"] == used["b3_hz"] == 4
    one = cli.family_means(rows[:1], family)
    assert one == {**{k: 3.0 * (i + 1) / used[k] for i, k in enumerate(figs)}, "formant_frames": 5, "unconverged_frames": 2}
    assert list(one) == list(figs) + ["formant_frames", "unconverged_frames"], "the order of the report's keys"
    assert cli.family_means(rows[1:], family) == {**{k: None for k in figs}, "formant_frames": 0, "unconverged_frames": 1}
    other = {"frames": 3, "unconverged_frames": 4, "used": {k: 1 for k in figs}, "sums": {k: -4.0 for k in figs}}
    m = cli.family_means([rows[0], other, rows[1]], family)
    assert m["formant_frames"] == 8 and m["unconverged_frames"] == 7
    assert all(abs(m[k] - (3.0 * (i + 1) - 4.0) / (used[k] + 1)) < 1e-12 for i, k in enumerate(figs))
    assert cli.family_means([], family) == {**{k: None for k in figs}, "formant_frames": 0, "unconverged_frames": 0}


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_ev_harmonics():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    assert re.search(r"\bint ev_load_harmonics\(ev_handle \*h,", header) and re.search(r"\bint ev_harmonics\(ev_handle \*h,", header)
    assert "ev_load_harmonics" in _lib.EXPORTS and "ev_harmonics" in _lib.EXPORTS
    assert "ev_load_harmonics, ev_harmonics" in re.search(r"#define EV_ABI_VERSION 4 .*", header).group(0), "the additions list of the ABI line"
    for word in ("UNVOICED", "SILENT", "UNRESOLVED", "min_spacing", "a3_range", "the lowest k of a tie", "Hanson 1997", "160 KiB"):
        assert word in header
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, "ev_harmonics") and hasattr(lib, "ev_load_harmonics") and lib.ev_abi_version() == 4


def test_kernel_uses_no_scratch():
    import importlib.util

    spec = importlib.util.spec_from_file_location("code_object", os.path.join(REPO, "tools", "code_object.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain is not installed")
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    k = [k for k in co.kernels(_lib.LIB_PATH) if k["demangled"].startswith("harmonics_kernel(")]
    assert len(k) == 1 and k[0]["vgpr_spill_count"] == 0 and k[0]["private_segment_fixed_size"] == 0 and k[0]["group_segment_fixed_size"] == 0, k


# ---- the CLI, with the device calls stubbed by the restatements ------------------------------------------------------------------------------------------
HARM_KEYS = set(audio.HARMONIC_FIGURES) | {"harmonic_frames"}


def _stubs(monkeypatch, wavs):
    fake_yin = voice_stubs.base(monkeypatch, wavs)
    fake_formants, calls = voice_stubs.flat_formants(monkeypatch)
    return fake_yin, fake_formants, voice_stubs.harmonics(monkeypatch), calls


def _wavs():
    return {"a.wav": complex_row(150.0, 0.0, n=6000, seed=1)[0], "b.wav": complex_row(220.0, 1.0, n=5000, seed=2)[0], "c.wav": np.zeros(3000, np.float32)}


def test_voice_report_harmonics_json_shape_and_validate_args(tmp_path, monkeypatch):
    from emojivoice_amd import cli

    wavs = _wavs()
    flist = voice_stubs.filelist(tmp_path, wavs)
    fake_yin, fake_fm, fake_hm, calls = _stubs(monkeypatch, wavs)
    ns = lambda **kw: argparse.Namespace(voice_report=str(flist), batch_size=2, sample_rate=None, prepare_dataset=None, **kw)
    plain = cli.voice_report(cli.validate_args(ns()), "cpu")
    assert calls["formants"] == 0
    rep = cli.voice_report(cli.validate_args(ns(harmonics=True)), "cpu")
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    figs = set(audio.HARMONIC_FIGURES)
    assert HARM_KEYS == {"h1_h2_db", "h1_a3_db", "f1_rel_db", "f2_rel_db", "f3_rel_db", "harmonic_frames"}
    assert saved == json.loads(json.dumps(rep)) and set(saved) == set(plain) == {"sample_rate", "hop_length", "files", "speakers", "overall"}
    old = {"path", "speaker", "seconds", "frames", "voiced_frames"} | set(audio.VOICE_QUALITY_FIGURES)
    assert [set(f_) for f_ in plain["files"]] == [old] * 3 and [set(f_) for f_ in saved["files"]] == [old | HARM_KEYS] * 3
    assert set(plain["overall"]) | HARM_KEYS == set(saved["overall"]) == set(saved["speakers"]["7"]) and not HARM_KEYS & set(plain["overall"])
    assert all(saved["files"][i][k] == plain["files"][i][k] for i in range(3) for k in old), "the flag changes none of the other figures"
    a, b, c = saved["files"]
    assert c["harmonic_frames"] == 0 and all(c[k] is None for k in figs) and a["harmonic_frames"] > 3 and b["harmonic_frames"] > 3
    assert abs(a["h1_h2_db"] - 20 * np.log10(2.0)) < 0.5 and abs(b["h1_h2_db"] - (20 * np.log10(2.0) + 1.0)) < 0.5, "1 / h, and 1 dB of tilt more"
    stats = {}
    for name in ("a.wav", "b.wav"):
        y = torch.from_numpy(wavs[name])[None]
        n = len(wavs[name])
        fm = fake_fm(y, lengths=[n])
        stats[name] = audio.harmonic_statistics(fake_hm(y, lengths=[n], formants=fm), fake_yin(y, lengths=[n])["voiced"], [R.frames(n, 256)], fm=fm)
    assert a["harmonic_frames"] == int(stats["a.wav"]["frames"][0])
    assert int(stats["a.wav"]["used"]["f2_rel_db"][0]) < int(stats["a.wav"]["used"]["f1_rel_db"][0]), "the bandwidth gate reaches the report"
    for k in figs:
        assert abs(a[k] - float(stats["a.wav"][k][0])) < 1e-9
        na, nb = int(stats["a.wav"]["used"][k][0]), int(stats["b.wav"]["used"][k][0])
        pooled = (a[k] * na + b[k] * nb) / (na + nb)
        assert abs(saved["speakers"]["7"][k] - pooled) < 1e-9 and saved["overall"][k] == saved["speakers"]["7"][k] and saved["speakers"]["12"][k] is None
    assert saved["speakers"]["7"]["harmonic_frames"] == a["harmonic_frames"] + b["harmonic_frames"] == saved["overall"]["harmonic_frames"]
    n0 = calls["formants"]
    both = cli.voice_report(cli.validate_args(ns(harmonics=True, formants=True)), "cpu")
    assert calls["formants"] - n0 == 2, "two batches: with --formants the formants are analysed once per batch for both"
    assert all(both["files"][i][k] == saved["files"][i][k] for i in range(3) for k in HARM_KEYS) and "f1_hz" in both["files"][0]
    with pytest.raises(AssertionError, match="--harmonics"):
        cli.validate_args(argparse.Namespace(harmonics=True, evaluate_pairs=None, voice_report=None, sample_rate=None, prepare_dataset=None))
    cli.validate_args(argparse.Namespace(harmonics=True, evaluate_pairs="pairs.txt", voice_report=None, batch_size=2, sample_rate=None, prepare_dataset=None))


def test_evaluate_pairs_harmonics_key_sets(tmp_path, monkeypatch):
    from emojivoice_amd import cli

    wavs = _wavs()
    _stubs(monkeypatch, wavs)
    whole = lambda w: w[: len(w) // 256 * 256]                            # (wav_at_rate hands out whole hops)
    monkeypatch.setattr(cli, "wav_at_rate", lambda path, sr, device: torch.from_numpy(whole(wavs[os.path.basename(str(path))])).unsqueeze(0))
    monkeypatch.setattr(audio, "mel_spectrogram", lambda w, *a, **k: torch.zeros(1, 80, w.shape[1] // 256))
    monkeypatch.setattr(audio, "mel_cepstrum", lambda mel, n=13: torch.zeros(1, n, mel.shape[2]))
    monkeypatch.setattr(audio, "dtw", lambda a, b, fa, fb, metric: {"cost": torch.zeros(a.shape[0], dtype=torch.float64),
                                                                     "steps": torch.ones(a.shape[0], dtype=torch.int32),
                                                                     "path": torch.zeros(a.shape[0], 1, 2, dtype=torch.int32)})
    monkeypatch.setattr(audio, "f0_errors", lambda *a: {"rmse_cents": [None] * a[0].shape[0], "voicing_error": torch.zeros(a[0].shape[0]),
                                                        "voiced_pairs": torch.zeros(a[0].shape[0], dtype=torch.int64)})
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("a.wav|b.wav|7\nb.wav|a.wav|7\na.wav|c.wav|12\n", encoding="utf-8")
    ns = lambda **kw: argparse.Namespace(evaluate_pairs=str(pairs), batch_size=2, sample_rate=None, prepare_dataset=None, voice_report=None, **kw)
    plain = cli.evaluate_pairs(cli.validate_args(ns()), "cpu")
    rep = cli.evaluate_pairs(cli.validate_args(ns(harmonics=True)), "cpu")
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    figs = set(audio.HARMONIC_FIGURES)
    assert all("harmonics" not in p for p in plain["pairs"]) and "harmonics" not in plain["overall"]
    assert [set(p) - {"harmonics"} for p in saved["pairs"]] == [set(p) for p in plain["pairs"]], "without the flag the key sets are the old ones"
    assert set(saved["overall"]) - {"harmonics"} == set(plain["overall"]) and set(saved) == set(plain)
    p0, p1, p2 = saved["pairs"]
    for p in saved["pairs"]:
        assert set(p["harmonics"]) == {"recorded", "synthesised", "delta"} and all(set(p["harmonics"][k]) == figs for k in p["harmonics"])
    for k in figs:
        assert abs(p0["harmonics"]["delta"][k] - (p0["harmonics"]["synthesised"][k] - p0["harmonics"]["recorded"][k])) < 1e-9
        assert abs(p0["harmonics"]["delta"][k] + p1["harmonics"]["delta"][k]) < 1e-9, "the swapped pair has the opposite deltas"
        assert p2["harmonics"]["synthesised"][k] is None and p2["harmonics"]["delta"][k] is None and isinstance(p2["harmonics"]["recorded"][k], float)
        s7 = saved["speakers"]["7"]["harmonics"][k]
        assert set(s7) == {"mean_delta", "mean_abs_delta"} and abs(s7["mean_delta"]) < 1e-9 and abs(s7["mean_abs_delta"] - abs(p0["harmonics"]["delta"][k])) < 1e-9
        assert saved["speakers"]["12"]["harmonics"][k] == {"mean_delta": None, "mean_abs_delta": None}
    assert abs(p0["harmonics"]["delta"]["h1_h2_db"] - 1.0) < 0.5, "b.wav has 1 dB of tilt per harmonic more"
