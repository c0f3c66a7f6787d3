"""CPU-side checks of the formant path: the numpy restatement (tests/formants_ref.py) against ``numpy.roots`` and a known all-pole signal, the
conditions on the inputs of the device tests, the mutants the device tests must tell apart, ``audio.formant_window``, the decimation and
frame-alignment rule, ``audio.formant_statistics``, the C ABI's declaration and export, and the ``--formants`` JSON shapes with the device
calls stubbed by the restatement.
"""
import os
import re

import numpy as np
import pytest
import torch

import formants_ref as R
import voice_stubs
from emojivoice_amd import _lib, audio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = R.GEOMETRIES[0]
_CASES = {}


def both(key, x, lens, g):
    """(float64 results, longdouble results) of a device case: computed once, never modified."""
    if key not in _CASES:
        r = (R.batch(x, lens, g), R.batch(x, lens, g, dtype=np.longdouble))
        for part in r:
            for v in part:
                v.setflags(write=False)
        _CASES[key] = r
    return _CASES[key]


def rows(g):
    x, lens = R.rows_for(g)
    return (x, lens) + both(("rows", g), x, lens, g)


# ---- the restatement against independent routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GEOMETRIES + R.EDGE_GEOMETRIES, ids=R.IDS + R.EDGE_IDS)
def test_restatement_roots_against_numpy_roots(g):
    """The Aberth-Ehrlich roots of the restatement's own coefficients and ``numpy.roots`` (the companion matrix's eigenvalues) of the same
    coefficients are the same sets within 1e-10, frame by frame."""
    x, lens, (lpc, _, ct, it, _), _ = rows(g)
    a = np.concatenate([np.ones(lpc.shape[:2] + (1,)), lpc[..., :g.order]], axis=-1)[it > 0]
    z, iters = R.aberth(a, np.float64)
    assert (iters > 0).all()
    worst = 0.0
    for f in range(0, a.shape[0], max(1, a.shape[0] // 60)):
        want = np.roots(a[f])
        d = np.abs(z[f][:, None] - want[None, :])
        worst = max(worst, float(d.min(axis=1).max()), float(d.min(axis=0).max()))
    print(f"\nformants restatement {g[:4]}: Aberth-Ehrlich against numpy.roots, as sets, at worst {worst:.3e} (gate 1e-10); iterations at most {int(iters.max())}")
    assert worst <= 1e-10


def test_a_known_all_pole_signal():
    """White noise through the all-pole filter with poles at 500 Hz / 80 Hz and 1500 Hz / 120 Hz, sr 8000, W 512, H 128, order 4, no
    pre-emphasis: the medians over the frames inside the row of |F1 - 500| / 500 and |F2 - 1500| / 1500 are 2.47 % and 1.19 % with this
    restatement (worst single frames 18 % and 5.3 %: one frame of noise is a rough estimate).  The gates are TWICE those medians: they are
    derived from the restatement itself, not from a published figure, and hold the definition in place (a wrong window, order or band rule
    moves the medians by far more)."""
    g = R.geometry(8000, 512, 128, 4, pre=0.0)
    x = R.pole_noise(8000, 8000, ((500.0, 80.0), (1500.0, 120.0)))
    _, fm, ct, it, _ = R.row(x, g)
    assert (ct == 2).all() and it.max() <= R.MAX_REF_ITERS
    w = slice(2, len(ct) - 2)
    e1, e2 = np.abs(fm[w, 0, 0] - 500.0) / 500.0, np.abs(fm[w, 1, 0] - 1500.0) / 1500.0
    print(f"\nformants, known poles: median |F1 - 500| / 500 {np.median(e1):.4f} (gate 0.0494), |F2 - 1500| / 1500 {np.median(e2):.4f} (gate 0.0238); "
          f"worst frames {e1.max():.3f} / {e2.max():.3f}; median bandwidths {np.median(fm[w, 0, 1]):.1f} / {np.median(fm[w, 1, 1]):.1f} Hz")
    assert np.median(e1) <= 0.0494 and np.median(e2) <= 0.0238


# ---- the conditions on the inputs of the device tests -------------------------------------------------------------------------------------------
def conditions(r64, rld, what):
    (lpc, fm, ct, it, mg), (lpcl, fml, ctl, itl, _) = r64, rld
    e_l, e_f = R.err(lpc, lpcl), R.err(fm, fml)
    print(f"\nformants {what}: float64 against longdouble d_lpc {e_l:.1e} d_formant {e_f:.1e} (gate {R.INPUT_TOL:g}); iterations at most "
          f"{int(max(it.max(), itl.max()))} (gate {R.MAX_REF_ITERS}); smallest band margin {mg.min():.3e} Hz (gate {R.MIN_FREQ_MARGIN:g}); "
          f"counts {np.bincount(ct.ravel() + 1).tolist()} from -1")
    assert max(e_l, e_f) <= R.INPUT_TOL and np.array_equal(ct, ctl)
    assert it.min() >= 0 and itl.min() >= 0 and max(it.max(), itl.max()) <= R.MAX_REF_ITERS
    assert mg.min() >= R.MIN_FREQ_MARGIN


@pytest.mark.parametrize("g", R.GEOMETRIES + R.EDGE_GEOMETRIES, ids=R.IDS + R.EDGE_IDS)
def test_device_rows_hold_the_input_conditions(g):
    """For the rows the device tests run: the comparison leaves out no frame; the frame counts are 3, 0, 1 modulo 4; no row passes 8000 samples."""
    x, lens, r64, rld = rows(g)
    assert [R.frames(n, g.H) % 4 for n in lens] == [3, 0, 1] and 2500 <= min(lens) and max(lens) <= 8000
    conditions(r64, rld, f"{g[:4]} lens {lens}")
    assert (r64[2][0, :R.frames(lens[0], g.H)] > 0).mean() > 0.5


def test_the_other_device_cases_hold_the_input_conditions():
    g = SMALL
    x, lens = R.rows_for(g)
    L = x.shape[1]
    hole = x[0].copy()
    hole[700:1500] = 0.0
    xd = np.concatenate([x, np.zeros((1, L), np.float32), hole[None], x[:1], x[:1], x[:1]])
    ld = lens + [2000, lens[0], 0, -3, L + 1]
    r64, rld = both("degenerate", xd, ld, g)
    conditions(r64, rld, "degenerate rows")
    assert not r64[2][3].any() and not r64[2][4, 700 // g.H + 3:1500 // g.H - 3].any() and not r64[0][5:].any()
    for i, (xs, ls) in enumerate(((x[:2], [1, lens[1]]), (x[:2, :1], None), (np.full((1, 1), 0.5, np.float32), None))):
        conditions(*both(("one", i), xs, ls, g), f"a row of one sample, case {i}")
    quiet = np.full((1, 1), 1e-6, np.float32)
    assert not R.batch(quiet, None, g)[0].any() and R.batch(quiet, None, g, floor=1e-300)[0][0, 0, -1] < 0.01 * R.POWER_FLOOR
    for gg in (SMALL, R.GEOMETRIES[2]):
        sig = [R.edge_signal(n, gg.W, seed=i) for i, n in enumerate((3000, 3000 + gg.H // 2 + 1))]
        xe, _, le = R.padded([(s, s) for s in sig])
        r64, rld = both(("edge", gg), xe, le, gg)
        conditions(r64, rld, f"edges {gg[:4]}")
        for b, n in enumerate(le):
            bad = R.row(xe[b, :n], gg, mutant="reflect")[0]
            for f in (0, R.frames(n, gg.H) - 1):
                assert np.abs(bad[f] - r64[0][b, f]).max() > 1e-6, "the reflect mutant shows at both ends"


def test_the_audio_case_holds_the_input_conditions():
    """audio.formants' rows (4000 / 2600 / 700 samples at 22050 Hz), decimated here by scipy's resample_poly, which the device resampler follows."""
    from scipy.signal import resample_poly

    lens = [4000, 2600, 700]
    xr = np.zeros((3, 2000), np.float32)
    for i, n in enumerate(lens):
        xr[i, :-(-n // 2)] = resample_poly(R.speech_like(n, seed=18 * i, fs=22050).astype(np.float64), 1, 2)
    g = R.geometry(11025.0, 512, 128, 13)
    conditions(*both("audio", xr, [-(-n // 2) for n in lens], g), "audio.formants' rows at 11025 Hz")


def test_a_pure_tone_does_not_hold_them():
    """Why the device test of the 147 Hz tone only asks for convergence: a sinusoid has rank 2, an order-10 predictor of it is ill-conditioned."""
    g = R.GEOMETRIES[2]
    x = R.tone(4000, g.sr)[None]
    a, b = R.batch(x, None, g), R.batch(x, None, g, dtype=np.longdouble)
    e = max(R.err(a[0], b[0]), R.err(a[1], b[1]))
    print(f"\nformants, 147 Hz tone: float64 against longdouble {e:.3e}; iterations at most {int(a[3].max())}")
    assert e > R.INPUT_TOL and (a[2] >= 0).all() and a[3].max() <= R.MAX_ITERS


# ---- the mutants ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_shows_on_a_small_geometry(mutant):
    moved = []
    for g in R.GEOMETRIES[:2]:
        x, lens, (_, fm, ct, _, _), _ = rows(g)
        _, fmm, ctm, _, _ = R.batch(x, lens, g, mutant=mutant)
        moved.append((float(np.abs(fmm - fm).max()), int((ctm != ct).sum())))
    print(f"\nformants mutant {mutant}: (largest move of a formant entry in Hz, frames whose count moves) on the two small geometries {moved}")
    assert all(d > 1e-6 for d, _ in moved)


# ---- the window, the decimation, the statistics -------------------------------------------------------------------------------------------------------
def test_formant_window():
    for W in (8, 24, 512, 1024):
        w = audio.formant_window(W)
        assert w.dtype == np.float64 and w.shape == (W,) and np.array_equal(w, R.formant_window(W))
        assert np.allclose(w, w[::-1], rtol=0, atol=1e-15) and w.min() > 0 and w.max() < 1 and np.argmax(w) in (W // 2 - 1, W // 2)
    j, W = 100, 512
    want = (np.exp(-48.0 * ((j + 0.5) / W - 0.5) ** 2) - np.exp(-12.0)) / (1.0 - np.exp(-12.0))
    assert abs(audio.formant_window(W)[j] - want) < 1e-16
    edge = (np.exp(-48.0 * (0.5 / 512 - 0.5) ** 2) - np.exp(-12.0)) / (1.0 - np.exp(-12.0))
    assert abs(audio.formant_window(512)[0] - edge) < 1e-18 and edge < 1e-6, "the window ends just above zero"


def test_decimation_and_frame_alignment():
    g = audio.formant_geometry()
    assert (g["d"], g["sr"], g["W"], g["H"], g["order"]) == (2, 11025.0, 512, 128, 13) and abs(g["pre"] - np.exp(-2 * np.pi * 50 / 11025)) < 1e-15
    assert audio.formant_geometry(44100)["d"] == 4 and audio.formant_geometry(44100)["sr"] == 11025.0 and audio.formant_geometry(16000)["d"] == 1
    assert audio.formant_geometry(16000)["order"] == 18 and audio.formant_geometry(22050, 5000.0)["d"] == 2 and audio.formant_geometry(22050, order=10)["order"] == 10
    for bad in (dict(hop_length=255), dict(frame_length=1023), dict(sr=44100, hop_length=258)):
        with pytest.raises(ValueError, match="multiples"):
            audio.formant_geometry(**bad)
    for d, hop in ((2, 256), (4, 256), (2, 6), (3, 9)):
        for L in list(range(1, 40)) + [4000, 4001, 2600, 700, 16383]:
            assert R.frames(-(-L // d), hop // d) == R.frames(L, hop), "ceil(ceil(L / d) / (H / d)) = ceil(L / H)"


def test_formant_statistics_against_numpy():
    g = np.random.default_rng(7)
    B, F = 3, 50
    freq = np.sort(g.uniform(200.0, 5000.0, (B, F, 4)), axis=-1)
    band = g.uniform(30.0, 1000.0, (B, F, 4))
    count = g.integers(-1, 5, (B, F)).astype(np.int32)
    voiced = g.random((B, F)) < 0.7
    voiced[2] = False
    lens = [50, 31, 50]
    fm = {"frequency": torch.from_numpy(freq), "bandwidth": torch.from_numpy(band), "count": torch.from_numpy(count)}
    st = audio.formant_statistics(fm, torch.from_numpy(voiced), lengths=lens)
    inside = np.arange(F)[None, :] < np.array(lens)[:, None]
    use = voiced & inside & (count >= 3)
    assert st["frames"].tolist() == use.sum(axis=1).tolist() and st["frames"].dtype == torch.int64 and st["frames"][2] == 0
    assert st["unconverged_frames"].tolist() == (inside & (count < 0)).sum(axis=1).tolist() and sum(st["unconverged_frames"].tolist()) > 0
    for i in range(3):
        ok = use & (band[:, :, i] <= 700.0)
        assert st["used"][:, i].tolist() == ok.sum(axis=1).tolist() and (ok.sum(axis=1) < use.sum(axis=1))[:2].all(), "the bandwidth rule leaves frames out"
        for name, v in ((f"f{i + 1}_hz", freq[:, :, i]), (f"b{i + 1}_hz", band[:, :, i])):
            assert st[name].dtype == torch.float64 and torch.isnan(st[name][2]) and float(st["sums"][name][2]) == 0.0
            for b in range(2):
                assert abs(float(st[name][b]) - v[b][ok[b]].mean()) < 1e-10 and abs(float(st["sums"][name][b]) - v[b][ok[b]].sum()) < 1e-9
    wide = audio.formant_statistics(fm, torch.from_numpy(voiced), lengths=lens, max_bandwidth=1e9)
    assert wide["used"][:, 0].tolist() == use.sum(axis=1).tolist()
    one = audio.formant_statistics({k: v[0] for k, v in fm.items()}, torch.from_numpy(voiced[0]))
    assert one["frames"].tolist() == [int((voiced[0] & (count[0] >= 3)).sum())]
    assert tuple(audio.FORMANT_FIGURES) == ("f1_hz", "f2_hz", "f3_hz", "b1_hz", "b2_hz", "b3_hz")
    with pytest.raises(ValueError, match="formant_statistics"):
        audio.formant_statistics(fm, torch.from_numpy(voiced[:, :5]))
    with pytest.raises(ValueError, match="formant_statistics"):
        audio.formant_statistics(fm, torch.from_numpy(voiced), lengths=[1, 2])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_ev_formants():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    for name in ("ev_load_formants", "ev_formants"):
        assert re.search(rf"\bint {name}\(ev_handle \*h,", header) and name in _lib.EXPORTS
        assert name in re.search(r"#define EV_ABI_VERSION 4 .*", header).group(0), "the additions list of the ABI line"
    assert "#define EV_ABI_VERSION 4" in header
    for word in ("Burg", "Aberth-Ehrlich", "UNCONVERGED", "SILENT", "2^-30"):
        assert word in header
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, "ev_load_formants") and hasattr(lib, "ev_formants") and lib.ev_abi_version() == 4


# ---- the CLI, with the device calls stubbed by the restatement --------------------------------------------------------------------------------------
def test_voice_report_formants_json_shape_and_validate_args(tmp_path, monkeypatch):
    import argparse
    import json

    from emojivoice_amd import cli

    wavs = {"a.wav": R.speech_like(6000, seed=20, fs=22050), "b.wav": R.speech_like(5000, seed=21, fs=22050), "c.wav": np.zeros(3000, np.float32)}
    flist = voice_stubs.filelist(tmp_path, wavs)
    fake_yin, fake_formants = voice_stubs.base(monkeypatch, wavs), voice_stubs.formants(monkeypatch)
    ns = lambda **kw: argparse.Namespace(voice_report=str(flist), batch_size=2, sample_rate=None, prepare_dataset=None, **kw)
    plain = cli.voice_report(cli.validate_args(ns()), "cpu")
    rep = cli.voice_report(cli.validate_args(ns(formants=True)), "cpu")
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    figs = set(audio.FORMANT_FIGURES)
    extra = figs | {"formant_frames", "unconverged_frames"}
    assert saved == json.loads(json.dumps(rep)) and set(saved) == set(plain) == {"sample_rate", "hop_length", "files", "speakers", "overall"}
    old = {"path", "speaker", "seconds", "frames", "voiced_frames"} | set(audio.VOICE_QUALITY_FIGURES)
    assert [set(f_) for f_ in plain["files"]] == [old] * 3 and [set(f_) for f_ in saved["files"]] == [old | extra] * 3
    assert set(plain["overall"]) | extra == set(saved["overall"]) == set(saved["speakers"]["7"]) and not extra & set(plain["overall"])
    assert all(saved["files"][i][k] == plain["files"][i][k] for i in range(3) for k in old), "the flag changes none of the other figures"
    a, b, c = saved["files"]
    assert c["formant_frames"] == 0 and all(c[k] is None for k in figs) and a["formant_frames"] > 3 and b["formant_frames"] > 3
    y = torch.from_numpy(wavs["a.wav"])[None]
    st = audio.formant_statistics(fake_formants(y, lengths=[6000]), fake_yin(y, lengths=[6000])["voiced"], [24])
    assert a["formant_frames"] == int(st["frames"][0]) and a["unconverged_frames"] == 0
    for k in figs:
        assert abs(a[k] - float(st[k][0])) < 1e-9
    used = {}
    for name in ("a.wav", "b.wav"):
        y = torch.from_numpy(wavs[name])[None]
        n = len(wavs[name])
        s = audio.formant_statistics(fake_formants(y, lengths=[n]), fake_yin(y, lengths=[n])["voiced"], [R.frames(n, 256)])
        used[name] = s["used"][0].tolist()
    for k in figs:
        i = int(k[1]) - 1
        pooled = (a[k] * used["a.wav"][i] + b[k] * used["b.wav"][i]) / (used["a.wav"][i] + used["b.wav"][i])
        assert abs(saved["speakers"]["7"][k] - pooled) < 1e-9 and saved["overall"][k] == saved["speakers"]["7"][k] and saved["speakers"]["12"][k] is None
    assert saved["speakers"]["7"]["formant_frames"] == a["formant_frames"] + b["formant_frames"] == saved["overall"]["formant_frames"]
    with pytest.raises(AssertionError, match="--formants"):
        cli.validate_args(argparse.Namespace(formants=True, evaluate_pairs=None, voice_report=None, sample_rate=None, prepare_dataset=None))
    cli.validate_args(argparse.Namespace(formants=True, evaluate_pairs="pairs.txt", voice_report=None, batch_size=2, sample_rate=None, prepare_dataset=None))
