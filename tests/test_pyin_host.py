"""Probabilistic YIN without a GPU: the numpy float64 restatement (tests/pyin_ref.py) against brute force and against mutants of itself, the
host tables of ``audio``, the declarations of ``ev_pyin_observe`` / ``ev_pyin_decode``, the code object, the reports' ``--pitch_method``,
the fragile share of every input tests/test_gpu_pyin.py runs, and what the method is worth against per-frame YIN.

WORTH, measured here on ``hard_row`` (a 3-harmonic glide from 110 to 220 Hz over 16384 samples with a component of 0.35 at HALF the pitch,
white noise of 0.05 and a 40 ms dip to 2 % of the level; 58 interior frames; gross error = f0 more than 20 % off, or a wrong voicing
decision).  Against the glide itself: per-frame YIN 58 gross errors, pYIN 58: no difference, because a component of 0.35 at half the pitch
makes half the glide the waveform's TRUE fundamental and both trackers find it.  Against that fundamental, on the 49 interior frames where
it lies inside the search range: YIN 8 (the frames of the dip, dropped), pYIN 3 (the Viterbi pass bridges all but its centre).  The row
was built once, from the description, and not tuned.
"""
import argparse
import itertools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pitch_ref as P
import pyin_ref as Y
from emojivoice_amd import _lib, audio, cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 22050
_CASES = {}


def case(name):
    """(x, lens, kw, observation) of a GPU test input, observed once."""
    if name not in _CASES:
        x, lens, kw = {"std": Y.std_case, "small": Y.small_case}[name]()
        _CASES[name] = (x, lens, kw, Y.observe(x, lens, **kw))
    return _CASES[name]


# ---- the Viterbi pass -------------------------------------------------------------------------------------------------------------------------
def brute_force(obs, pv, tables):
    """Every path scored by path_score; among the best the one that is smallest read from its END (the end state is the lowest of greatest
    delta, and every step back takes the lowest predecessor that attains it)."""
    S, F = 2 * tables["n_bins"], len(pv)
    best, arg = -np.inf, None
    for path in itertools.product(range(S), repeat=F):
        sc = Y.path_score(path, obs, pv, tables)
        if sc > best or (sc == best and path[::-1] < arg[::-1]):
            best, arg = sc, path
    return np.array(arg, np.int32), best


@pytest.mark.parametrize("n_bins,R,seed", [(2, 0, 0), (2, 1, 1), (3, 0, 2), (3, 1, 3), (3, 1, 4)])
def test_viterbi_against_brute_force(n_bins, R, seed):
    obs, pv, tables = Y.random_model(n_bins, R, 4, seed)
    want, score = brute_force(obs, pv, tables)
    for fn in (Y.viterbi, Y.viterbi_fast):
        got, ll = fn(obs, pv, tables)
        assert np.array_equal(got, want) and ll == score, fn.__name__
    assert Y.path_score(want, obs, pv, tables) == score


def test_viterbi_fast_is_viterbi():
    obs, pv, tables = Y.random_model(7, 2, 9, 11)
    a, b = Y.viterbi(obs, pv, tables), Y.viterbi_fast(obs, pv, tables)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_mutant_ties_to_the_higher_state_is_caught():
    tables = Y.transition_tables(3, 1)
    obs, pv = np.zeros((4, 3)), np.zeros(4)                              # every unvoiced state ties with the others at every frame
    want, _ = brute_force(obs, pv, tables)
    assert np.array_equal(Y.viterbi(obs, pv, tables)[0], want)
    assert not np.array_equal(Y.viterbi(obs, pv, tables, lowest_on_ties=False)[0], want)


def test_mutant_untruncated_Z_is_caught():
    for nb, R in ((3, 1), (49, 3), (385, 25), (5, 9)):
        t = Y.transition_tables(nb, R)
        i, j = np.arange(nb)[None, :], np.arange(nb)[:, None]
        d = np.abs(i - j)
        a = np.where(d <= R, np.exp(t["log_tri"][np.minimum(d, R)] - t["log_Z"][:, None]), 0.0)
        assert np.allclose(a.sum(axis=1), 1.0, atol=1e-12), "every row of the transition sums to one"
        bad = Y.transition_tables(nb, R, truncate=False)
        ab = np.where(d <= R, np.exp(bad["log_tri"][np.minimum(d, R)] - bad["log_Z"][:, None]), 0.0)
        assert abs(ab.sum(axis=1)[0] - 1.0) > 1e-3
        lt, lz, ls, lw = audio.pyin_transition(nb, R, 0.01)
        assert np.array_equal(lt, t["log_tri"]) and np.array_equal(lz, t["log_Z"]) and ls == t["log_stay"] and lw == t["log_switch"]
    obs, pv, tables = Y.random_model(3, 1, 4, 3)
    obs[:, 0] += 0.2
    assert Y.viterbi(obs, pv, tables)[1] != Y.viterbi(obs, pv, Y.transition_tables(3, 1, truncate=False))[1]
    assert Y.transition_radius(22050, 256, 120) == 25 == audio.pyin_transition_radius(22050, 256, 120)
    assert Y.bins_of(65.0, 600.0, 0.1) == (120, 385) == audio.pyin_bins(65.0, 600.0, 0.1)
    assert Y.bins_of(100.0, 400.0, 0.5) == (24, 49) and Y.transition_radius(22050, 128, 24) == 3


# ---- the prior --------------------------------------------------------------------------------------------------------------------------------
def test_threshold_prior():
    w = audio.pyin_threshold_prior(100, (2, 18))
    assert w.shape == (100,) and w.dtype == np.float64 and np.all(w >= 0) and abs(w.sum() - 1.0) <= 1e-14
    assert np.allclose(w, Y.threshold_prior(100, (2, 18)), rtol=0, atol=1e-14)
    assert np.allclose(audio.pyin_threshold_prior(7, (1, 1)), 1 / 7, atol=1e-15), "Beta(1, 1) is uniform"
    try:
        from scipy.stats import beta
    except ImportError:
        beta = None
    if beta is not None:
        for n, ab in ((100, (2, 18)), (128, (3, 5)), (10, (2.5, 7.5))):
            want = np.diff(beta.cdf(np.arange(n + 1) / n, *ab))
            assert np.allclose(audio.pyin_threshold_prior(n, ab), want, rtol=0, atol=1e-13), (n, ab)
    for bad in ((0, (2, 18)), (129, (2, 18)), (100, (0, 18))):
        with pytest.raises(ValueError):
            audio.pyin_threshold_prior(*bad)


# ---- the observation --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["std", "small"])
def test_observation_is_a_sub_distribution_and_few_frames_are_fragile(name):
    x, lens, kw, o = case(name)
    nf = [P.frame_count(n, kw["hop_length"]) for n in lens]
    total = sum(nf)
    fragile = int(o["fragile"].sum())
    print(f"\nPYIN {name}: frames {total} fragile {fragile} max pv before the clip {float(o['pv_raw'].max()):.15f}")
    assert np.all(o["obs"] >= 0) and float(o["pv_raw"].max()) <= 1 + 1e-12
    assert fragile <= 0.02 * total, "the GPU test's input must leave at most 2 % of its frames to the fragile rule (change the seed)"
    for b, n in enumerate(nf):
        assert not o["obs"][b, n:].any() and not o["pv"][b, n:].any(), "frames past the row"
    assert float(o["pv"].max()) > 0.9, "the tones are seen as voiced"


def test_silence_has_no_trough_and_mutant_le_is_caught():
    x = np.zeros((1, 2048), np.float32)
    kw = Y.geometry(22050, 65.0, 600.0, 1024, 256, 0.1)
    o = Y.observe(x, None, **kw)
    assert not o["obs"].any() and not o["pv"].any() and not o["fragile"].any()
    m = Y.observe(x, None, strict=False, **kw)
    assert m["pv"].min() > 0, "<= for < makes every lag of a silent frame a trough"
    r = Y.pitch_pyin(x)
    assert not r["voiced"].any() and not r["f0"].any() and np.all(r["states"] >= 385)


def test_mutant_without_the_no_trough_mass_is_caught():
    g = np.random.default_rng(0)
    x = (0.1 * g.standard_normal(4096)).astype(np.float32)
    kw = Y.geometry(22050, 65.0, 600.0, 1024, 256, 0.1)
    a, b = Y.observe(x, None, **kw), Y.observe(x, None, no_trough=False, **kw)
    gap = a["pv_raw"] - b["pv_raw"]
    print(f"\nPYIN noise: pv with the no-trough mass {a['pv_raw'][0, 4:8]}, without {b['pv_raw'][0, 4:8]}")
    assert np.all(gap > 1e-4) and np.all(gap <= 0.01 + 1e-12), "the global minimum gains at most no_trough_prob"


def test_bad_rows_and_short_rows():
    x = np.full((3, 1000), P.GARBAGE, np.float32)
    x[1, :300] = P.harmonic_tone(200.0, 300)
    r = Y.pitch_pyin(x, lengths=[0, 300, 1001])
    assert np.all(r["states"][0] == -1) and np.all(r["states"][2] == -1) and np.all(r["states"][1, :2] >= 0) and np.all(r["states"][1, 2:] == -1)
    assert not r["voiced"][0].any() and not r["voiced_prob"][[0, 2]].any()


# ---- what the method is worth -------------------------------------------------------------------------------------------------------------------
def hard_row(n=16384, sr=SR, seed=0):
    t = np.arange(n) / sr
    T = n / sr
    f = 110.0 + (220.0 - 110.0) * t / T
    phase = 2 * np.pi * (110.0 * t + 0.5 * (220.0 - 110.0) * t * t / T)
    y = np.sin(phase) + 0.5 * np.sin(2 * phase + 0.3) + 0.25 * np.sin(3 * phase + 0.6) + 0.35 * np.sin(0.5 * phase + 0.2)
    y = 0.3 * y
    dip0 = n // 2
    y[dip0: dip0 + int(0.040 * sr)] *= 0.02
    y = y + 0.05 * np.random.default_rng(seed).standard_normal(n)
    return y.astype(np.float32), f


def test_pyin_makes_no_more_gross_errors_than_yin():
    y, f_true = hard_row()
    n, H = len(y), 256
    F = P.frame_count(n, H)
    it = P.interior_frames(F, n)
    centre = np.minimum(np.arange(F) * H + H // 2, n - 1)
    truth = f_true[centre]
    r = P.pitch_yin(y, None, 1024, H, 36, 340, 0.1)
    f_yin, v_yin = P.f0_from_period(r["period"], SR)[0], r["lag"][0] > 0
    q = Y.pitch_pyin(y)
    f_pyin, v_pyin = q["f0"][0], q["voiced"][0]

    def gross(f, v, truth, frames):
        wrong = ~v | (np.abs(np.where(v, f, truth) / truth - 1.0) > 0.2)   # (every frame of the row is voiced in truth)
        return int(wrong[frames].sum())

    # (a) against the glide the row was built around; (b) against the waveform's own period: the component at half the pitch makes HALF the
    # glide the true fundamental, on the interior frames where that lies inside the search range (>= fmin = 65 Hz)
    in_range = it & (truth / 2 >= 65.0)
    a_yin, a_pyin = gross(f_yin, v_yin, truth, it), gross(f_pyin, v_pyin, truth, it)
    b_yin, b_pyin = gross(f_yin, v_yin, truth / 2, in_range), gross(f_pyin, v_pyin, truth / 2, in_range)
    print(f"\nPYIN worth: interior frames {int(it.sum())}: gross errors against the glide YIN {a_yin} pYIN {a_pyin}; "
          f"against half the glide ({int(in_range.sum())} frames in range) YIN {b_yin} pYIN {b_pyin}")
    assert a_pyin <= a_yin and b_pyin <= b_yin


# ---- the reports --------------------------------------------------------------------------------------------------------------------------------
def test_prosody_report_pitch_method(tmp_path, monkeypatch):
    (tmp_path / "a.wav").write_bytes(b"")
    flist = tmp_path / "filelist.txt"
    flist.write_text(f"{tmp_path / 'a.wav'}|7|first\n", encoding="utf-8")
    used = []

    def fake_load(path, sr=22050, device="cuda"):
        return torch.from_numpy(P.harmonic_tone(110.0, 4096)).unsqueeze(0)

    def fake_yin(y, sr=22050, fmin=65.0, fmax=600.0, frame_length=1024, hop_length=256, threshold=0.1, lengths=None):
        used.append("yin")
        r = P.pitch_yin(y.numpy(), lengths, frame_length, hop_length, 36, 340, threshold)
        return {"f0": torch.from_numpy(P.f0_from_period(r["period"], sr)).float(), "voiced": torch.from_numpy(r["lag"] > 0),
                "aperiodicity": torch.from_numpy(r["cmnd"]).float()}

    def fake_pyin(y, sr=22050, hop_length=256, lengths=None, **kw):
        used.append("pyin")
        r = Y.pitch_pyin(y.numpy(), sr, hop_length=hop_length, lengths=lengths)
        return {"f0": torch.from_numpy(r["f0"]).float(), "voiced": torch.from_numpy(r["voiced"]), "voiced_prob": torch.from_numpy(r["voiced_prob"]).float()}

    monkeypatch.setattr(audio, "load_audio", fake_load)
    monkeypatch.setattr(audio, "pitch_yin", fake_yin)
    monkeypatch.setattr(audio, "pitch_pyin", fake_pyin)
    base = dict(prosody_report=str(flist), batch_size=3, sample_rate=None, prepare_dataset=None)
    cli.prosody_report(cli.validate_args(argparse.Namespace(**base)), "cpu")
    plain = (tmp_path / "filelist.txt.prosody.json").read_bytes()
    cli.prosody_report(cli.validate_args(argparse.Namespace(pitch_method="yin", **base)), "cpu")
    assert (tmp_path / "filelist.txt.prosody.json").read_bytes() == plain, "the default writes what it wrote without the flag"
    assert "pitch_method" not in json.loads(plain)
    rep = cli.prosody_report(cli.validate_args(argparse.Namespace(pitch_method="pyin", **base)), "cpu")
    assert used == ["yin", "yin", "pyin"]
    saved = json.loads((tmp_path / "filelist.txt.prosody.json").read_text())
    assert saved["pitch_method"] == "pyin" and set(saved) == set(json.loads(plain)) | {"pitch_method"} and saved == json.loads(json.dumps(rep))
    assert saved["files"][0]["f0_median"] == pytest.approx(110.0, rel=2 ** (1 / 120) - 1), "within one bin of the tone"


def test_audio_pitch_pyin_arguments():
    with pytest.raises(_lib.EvLibraryError, match="GPU"):
        audio.pitch_pyin(torch.zeros(4000))
    with pytest.raises(ValueError):
        audio.pitch_pyin(torch.zeros(1, 2, 3))
    with pytest.raises(ValueError):
        audio.pyin_transition(385, 25, 0.0)
    with pytest.raises(ValueError):
        audio.pyin_bins(600.0, 65.0)


# ---- the declarations and the code object -------------------------------------------------------------------------------------------------------
DECLARED = {
    "ev_pyin_observe": ["ev_handle *h", "const float *d_x", "const int32_t *d_len", "int B", "int L", "int frame_length", "int hop_length", "int tau_min",
                        "int tau_max", "double sr", "double fmin", "int bins_per_octave", "int n_bins", "const double *w", "int n_thr",
                        "double boltzmann", "double no_trough_prob", "double *d_obs", "double *d_pv", "void *stream"],
    "ev_pyin_decode": ["ev_handle *h", "const double *d_obs", "const double *d_pv", "const int32_t *d_len", "int B", "int L", "int hop_length",
                       "int n_bins", "int R", "const double *log_tri", "const double *log_Z", "double log_stay", "double log_switch",
                       "uint8_t *d_back", "int32_t *d_state", "double *d_loglik", "void *stream"],
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_header_declares_and_library_exports(name):
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared in include/emojivoice.h"
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == DECLARED[name]
    assert re.search(r"\*\s+%s\s+<-\s+no counterpart; librosa\.pyin is the model" % name, header)
    assert re.search(r"#define\s+EV_ABI_VERSION\s+4\b.*%s" % name, header), "the ABI line's additions list"
    assert name in _lib.EXPORTS and hasattr(_lib.Engine, name[3:])
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert len(getattr(lib, name).argtypes) == len(DECLARED[name])
    nm = "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        syms = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\sT\s+%s\b" % name, syms)


def test_the_kernels_have_no_scratch():
    import importlib.util

    spec = importlib.util.spec_from_file_location("code_object", os.path.join(REPO, "tools", "code_object.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain is not installed")
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    all_kernels = co.kernels(_lib.LIB_PATH)
    for name, vgprs in (("pyin_observe_kernel", 128), ("pyin_decode_kernel", 128)):
        ks = [k for k in all_kernels if k["demangled"].startswith(name)]
        assert len(ks) == 1, f"{name}: one kernel, one launch"
        k = ks[0]
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= vgprs, k
