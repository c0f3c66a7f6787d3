"""ev_functionals on the MI355X, through the C ABI, and what stands on it (audio.functionals, audio.voice_functionals, --voice_report
--functionals).

Yardstick: tests/functionals_ref.py, the numpy restatement of the definition in include/emojivoice.h, in float64 (adding in the device's order)
and in longdouble.  The rule of every comparison (``check``):
  * d_count EQUAL;
  * min, max and every percentile whose t is 0 EQUAL to the restatement as values (-0 equals +0);
  * every other entry of d_stat within 1e-9 max(|ref|, 1): the project's float64 margin.
Every decision is a comparison of input values or of one IEEE product formed identically on both sides, so no frame and no contour is left out.
Observed on the MI355X: every entry of d_stat and d_count EQUAL to the float64 restatement on every case, worst error 0 against the gate of 1e-9
(the restatement adds in the device's order; the square root is the only library function); float64 against longdouble 5.1e-14 at worst (the
4096-frame ramp); voice_functionals' 63 means within 2.6e-16 relative of the *_statistics functions (gate 1e-12) and its f0_semitones percentiles
within 6.4e-6 semitones of prosody_statistics (gate 1e-4).  Every case prints its worst figure; DESIGN section 3.23 records them.  Every raw call
writes into buffers with 64-element sentinel margins (tests/analysis_gpu.py); NaN under a mask of ones lies behind every row's length, so a read behind it would show as a
dropped frame.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import functionals_ref as R
import perturbation_ref as P
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

_REF, _CASES = {}, {}


def case(name):
    if not _CASES:
        _CASES.update(R.cases())
    return _CASES[name]


def ref_of(key, v, mask, lens, q):
    """The restatements' results (float64, longdouble), computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: (R.batch(v, mask, lens, q), R.batch(v, mask, lens, q, dtype=np.longdouble)))


def raw(eng, v, mask, lens, q, null=(), **kw):
    """ev_functionals into guarded buffers: (rc, stat (B, K, 12 + NQ), count (B, K, 8)) on the host; an argument named in ``null`` is passed as
    NULL; ``kw`` overrides B, K, F or NQ as passed to the library.  A failed call must have written nothing."""
    v = torch.as_tensor(np.asarray(v, dtype=np.float64)).to(DEV).contiguous()
    Bx, Kx, Fx = v.shape
    qa = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1))
    NQx = len(qa)
    d_mask = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.uint8)).to(DEV).contiguous()
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"stat": ((Bx, Kx, 12 + NQx), torch.float64), "count": ((Bx, Kx, 8), torch.int32)}, null)
    rc = eng.lib.ev_functionals(eng.h, None if "v" in null else v.data_ptr(), None if d_mask is None else d_mask.data_ptr(),
                                None if d_len is None else d_len.data_ptr(), kw.get("B", Bx), kw.get("K", Kx), kw.get("F", Fx),
                                None if "q" in null or not NQx else qa.ctypes.data, kw.get("NQ", NQx), out.ptr("stat"), out.ptr("count"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    st, ct = dev
    r64, rld = ref
    assert np.array_equal(r64["count"], rld["count"]), f"{what}: the float64 and longdouble restatements disagree on a count"
    rs = r64["stat"]
    errs = [R.err(st[..., i], rs[..., i]) for i in range(12)]
    exact = np.zeros(rs.shape, bool)
    exact[..., 2:4] = True
    exact[..., 12:] = r64["t0"]
    pe = R.err(st[..., 12:], rs[..., 12:])
    print(f"\nfunctionals {what}: worst d_stat err {max(errs + [pe]):.3e} ({', '.join(f'{n} {e:.1e}' for n, e in zip(R.STAT, errs))}, percentiles {pe:.1e}; "
          f"gate {R.TOL:g})  float64 against longdouble {R.err(rs, rld['stat'].astype(np.float64)):.3e}  counts differing {int((ct != r64['count']).sum())}  "
          f"exact entries differing {int((st[exact] != rs[exact]).sum())} of {int(exact.sum())}  contours {ct.shape[0] * ct.shape[1]}, "
          f"valid frames {int(r64['count'][..., 0].sum())}, parts {int(r64['count'][..., 2:4].sum())}, peaks {int(r64['count'][..., 4].sum())}, "
          f"dropped {int(r64['count'][..., 1].sum())}")
    assert np.array_equal(ct, r64["count"]), f"{what}: d_count"
    assert np.isfinite(st).all(), f"{what}: d_stat is finite"
    assert np.array_equal(st[exact], rs[exact]), f"{what}: min, max and the percentiles with t == 0 are values of the contour"
    assert max(errs + [pe]) <= R.TOL, f"{what}: d_stat"
    empty = r64["count"][..., 0] == 0
    assert not st[empty][:, :8].any() and not st[empty][:, 12:].any(), f"{what}: exact zeros without a valid frame"


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


def run_case(eng, name):
    v, mask, lens, q = case(name)
    rc, *dev = raw(eng, v, mask, lens, q)
    assert rc == 0, err_of(eng)
    ref = ref_of(name, v, mask, lens, q)
    check(dev, ref, f"{name} {v.shape} lens {lens} NQ {len(q)}")
    return v, mask, lens, q, dev, ref


# ---- 1. every case against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", R.SHAPES)
def test_shapes_against_the_restatement(eng, F):
    """(3, 4, F) with lengths F, F - 1 and (F + 1) / 2: the contour kinds (walk, integers with plateaus, constant, signed zeros, ramp) and the mask
    kinds (ones, random runs, alternating, zeros) cycle over the contours; F around one and four tiles of 256 and around a wave of 64."""
    run_case(eng, f"F{F}")


def test_one_falling_ramp_over_4096_frames(eng):
    """One part across every wave, slot and tile: the max-scan must carry its start over all of them; the sort reverses 4096 values; NQ = 16."""
    v, mask, lens, q, (st, ct), _ = run_case(eng, "ramp4096")
    assert ct[0, 0].tolist() == [4096, 0, 0, 1, 0, 1, 0, 4095] and st[0, 0, 7] == 0.0 and st[0, 0, 6] == (v[0, 0, -1] - v[0, 0, 0]) / 4095.0
    assert st[0, 0, 12] == v[0, 0, -1] and st[0, 0, 13] == v[0, 0, 0], "q = 0 and q = 1 are min and max"


def test_twenty_contours_of_516_frames(eng):
    run_case(eng, "batch516")


def test_lengths_0_1_F_and_the_two_bad_ones(eng):
    v, mask, lens, q, (st, ct), _ = run_case(eng, "lengths")
    assert lens == [0, 1, 65, 66, -1]
    for b in (0, 3, 4):
        assert not st[b].any() and not ct[b].any(), "d_len 0, F + 1 and -1: rows of zeros"
    assert ct[1, 0].tolist() == [1, 0, 0, 0, 0, 1, 0, 0] and st[1, 0, 0] == st[1, 0, 2] == st[1, 0, 3] == st[1, 0, 13] == v[1, 0, 0] and st[1, 0, 1] == 0.0
    assert ct[2, 0, 0] == 65


@pytest.mark.parametrize("name", ("null-mask-null-lengths-nq0", "nq1", "nq16"))
def test_null_mask_null_lengths_and_the_numbers_of_percentiles(eng, name):
    v, mask, lens, q, (st, ct), _ = run_case(eng, name)
    assert st.shape[2] == 12 + len(q)


def test_non_finite_values_under_the_mask_are_dropped_and_counted(eng):
    v, mask, lens, q, (st, ct), _ = run_case(eng, "nonfinite")
    assert ct[0, 0, 1] == 5 and ct[0, 0, 5] == 5 and ct[0, 0, 6] == 5 and ct[0, 0, 0] == v.shape[2] - 6
    assert ct[1, 1].tolist() == [0, v.shape[2], 0, 0, 0, 0, 1, 0] and st[1, 1, 10] == v.shape[2]


@pytest.mark.parametrize("name", ("hand", "gapped"))
def test_hand_cases(eng, name):
    v, mask, lens, q, (st, ct), _ = run_case(eng, name)
    if name == "hand":
        assert ct[0, 0].tolist() == [9, 0, 3, 2, 2, 1, 0, 8] and st[0, 0, 13] == 2.0 and st[0, 0, 6] == -2.5 and st[0, 0, 7] == 1.5
    else:
        assert ct[0, 0].tolist() == [4, 0, 2, 0, 0, 2, 3, 2] and st[0, 0, 4] == 1.0


def test_the_mutants_differ_from_the_device(eng):
    """What the host test shows of the restatement holds of the device: on its named case the device sides with the definition, not the mutant."""
    for mutant, (name, bk, what) in R.MUTANT_SHOWS.items():
        v, mask, lens, q = case(name)
        rc, st, ct = raw(eng, v, mask, lens, q)
        assert rc == 0
        got = R.output({"stat": st, "count": ct}, bk, what)
        bad = R.output(R.batch(v, mask, lens, q, mutant=mutant), bk, what)
        good = R.output(ref_of(name, v, mask, lens, q)[0], bk, what)
        assert abs(float(got) - float(good)) <= 1e-9 and abs(float(got) - float(bad)) > 1e-6, (mutant, got, good, bad)


# ---- 2. the identities -------------------------------------------------------------------------------------------------------------------------------
def test_alone_in_a_batch_at_another_k_as_a_prefix_twice_and_under_every_arithmetic_give_the_same_bits(eng):
    g = np.random.default_rng(21)
    F = 257
    c, cm = R.make_contour("walk", F, g), R.make_mask("runs", F, g)
    q = R.Q3
    n0 = eng.alloc_count()
    rc, *alone = raw(eng, c[None, None], cm[None, None], None, q)
    assert rc == 0, err_of(eng)
    check(alone, ref_of("identity", c[None, None], cm[None, None], None, q), "the identity contour alone")
    assert alone[1][0, 0, 2] > 3 and alone[1][0, 0, 6] > 3
    rc, *again = raw(eng, c[None, None], cm[None, None], None, q)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    vb, mb = R.make(3, 4, F, seed=22)
    vb[1, 2], mb[1, 2] = c, cm
    vb[2, 0], mb[2, 0] = c, cm
    rc, *batch = raw(eng, vb, mb, None, q)
    assert rc == 0
    Fp = 400
    vp, mp = R.make(2, 3, Fp, seed=23, lens=[Fp, F])
    vp[1, 1, :F], mp[1, 1, :F] = c, cm                                   # (NaN under mask 1 lies behind d_len = 257)
    assert np.isnan(vp[1, 1, F:]).all() and (mp[1, 1, F:] == 1).all()
    rc, *prefix = raw(eng, vp, mp, [Fp, F], q)
    assert rc == 0
    for what, other, at in (("inside a batch", batch, (1, 2)), ("at another k", batch, (2, 0)), ("the d_len prefix of a longer F", prefix, (1, 1))):
        for i, out in enumerate(("d_stat", "d_count")):
            assert np.array_equal(alone[i][0, 0], other[i][at]), f"{out}: alone against {what}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 3, 6):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, vb, mb, None, q)
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0, "ev_alloc_count never moves"


def test_no_allocation_and_capturable():
    e = Engine(0)
    v, mask, lens, q = case("F257")
    vd = torch.from_numpy(v).to(DEV)
    md = torch.from_numpy(mask).to(DEV)
    n0 = e.alloc_count()
    ref = e.functionals(vd, md, lens, q)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        e.functionals(vd, md, ld, q)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = e.functionals(vd, md, ld, q)
        for t in out:
            t.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b), "the replay equals the eager call"
    r64 = ref_of("F257", v, mask, lens, q)[0]
    assert np.array_equal(out[1].cpu().numpy(), r64["count"])
    assert e.alloc_count() == n0
    e.close()


# ---- 3. limits -----------------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
BAD_CALL = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("K=", dict(K=0)), ("K=", dict(K=65536)), ("F=", dict(F=0)), ("F=", dict(F=4097)),
    ("NQ=", dict(NQ=-1)), ("NQ=", dict(NQ=17)), ("q[1]", dict(q=(0.5, NAN, 0.2))), ("q[0]", dict(q=(INF,))), ("q[2]", dict(q=(0.5, 0.2, -1e-9))),
    ("q[0]", dict(q=(1.0000001,))), ("q must", dict(null=("q",))), ("d_v", dict(null=("v",))), ("d_stat", dict(null=("stat",))),
    ("d_count", dict(null=("count",))),
]


@pytest.mark.parametrize("word,kw", BAD_CALL, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_fails_with_a_message_naming_it_and_writes_nothing(eng, word, kw):
    kw = dict(kw)
    q = kw.pop("q", R.Q3)
    z = np.zeros((2, 2, 16))
    rc, *_ = raw(eng, z, None, None, q, **kw)                            # (a failed call writes nothing: raw checks that)
    msg = err_of(eng)
    assert rc != 0 and "ev_functionals" in msg and word in msg, msg


# ---- 4. audio.functionals -------------------------------------------------------------------------------------------------------------------------------
def test_audio_functionals_on_three_ragged_rows():
    g = np.random.default_rng(31)
    F, lens = 300, [300, 120, 7]
    v = np.stack([np.stack([R.make_contour(kind, F, g) for kind in ("walk", "integers")]) for _ in range(3)]).astype(np.float32)
    mask = np.stack([R.make_mask(kind, F, g) for kind in ("runs", "ones", "zeros")])[:, None, :] != 0      # (3, 1, F): one mask per row
    vd, md = torch.from_numpy(v).to(DEV), torch.from_numpy(mask).to(DEV)
    eng = audio._trim_engine(vd.device)
    out = audio.functionals(vd, md, lens)
    n0 = eng.alloc_count()
    out2 = audio.functionals(vd, md, lens)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0, "no allocation"
    assert all(torch.equal(out[k], out2[k]) or bool(torch.isnan(out[k]).any()) for k in out)
    full = np.broadcast_to(mask, v.shape)
    ref = ref_of("audio", v.astype(np.float64), full.astype(np.uint8), lens, R.Q3)
    ct = np.stack([out[k].cpu().numpy() for k in audio.FUNCTIONAL_COUNTS], axis=-1)
    st = np.concatenate([np.stack([out[k].cpu().numpy() for k in audio.FUNCTIONAL_STATISTICS], axis=-1), out["percentiles"].cpu().numpy()], axis=-1)
    assert st.dtype == np.float64 and ct.dtype == np.int32 and st.shape == (3, 2, 15) and out["range"].shape == (3, 2)
    behind = np.array([audio._FUNCTIONAL_BEHIND[k] for k in audio.FUNCTIONAL_STATISTICS] + [0, 0, 0])
    none = np.take(ct, behind, axis=-1) == 0
    assert np.array_equal(np.isnan(st), none), "NaN exactly where the count behind a statistic is 0"
    assert none[2][:, :10].all() and not none[2][:, 10:12].any() and not none[0, :, :4].any(), "a row under a mask of zeros is one gap and nothing else"
    check((np.where(none, 0.0, st), ct), ref, "audio.functionals (3, 2, 300) float32, lengths 300 / 120 / 7")
    rng = out["range"].cpu().numpy()
    assert np.array_equal(rng[:2], st[:2, :, 14] - st[:2, :, 12]) and np.isnan(rng[2]).all()
    one = audio.functionals(vd[0, 0], md[0, 0])
    assert one["mean"].shape == (1, 1) and torch.equal(one["mean"][0, 0], out["mean"][0, 0]) and torch.equal(one["percentiles"][0, 0], out["percentiles"][0, 0])
    two = audio.functionals(vd[:, 1], md[:, 0], lens, percentiles=())
    assert two["sd"].shape == (3, 1) and torch.equal(two["sd"][:2, 0], out["sd"][:2, 1]) and two["percentiles"].shape == (3, 1, 0) and bool(torch.isnan(two["range"]).all())


def test_voice_functionals_ties_to_the_statistics_functions():
    """Pulse rows like perturbation_ref.audio_rows(), long enough for percentiles: every contour's mean is the mean of its *_statistics function
    (1e-12 relative), and the f0_semitones percentiles are prosody_statistics' through 12 log2(. / 27.5) (1e-4 semitones: that path is float32)."""
    spec = ((12000, 120.0, 0.01, 0.05), (9000, 180.0, 0.005, 0.02), (3000, 100.0, 0.0, 0.0))
    x, lens = P.padded([P.perturbed_pulses(n, f0, j, s, seed=11 + i, noise=1e-3) for i, (n, f0, j, s) in enumerate(spec)])
    x[np.arange(x.shape[1])[None, :] >= np.array(lens)[:, None]] = 0.0
    xd = torch.from_numpy(x).to(DEV)
    fl = [P.frames(n, 256) for n in lens]
    pitch = audio.pitch_yin(xd, lengths=lens)
    vq = audio.voice_quality(xd, lengths=lens)
    fm = audio.formants(xd, lengths=lens)
    pt = audio.perturbation(xd, lengths=lens)
    hm = audio.harmonics(xd, lengths=lens, formants=fm)
    voiced = pitch["voiced"]
    vf = audio.voice_functionals(pitch, vq, fl, fm=fm, pt=pt, hm=hm, percentiles=(0.05, 0.5, 0.95))
    assert vf["contours"] == ("f0_semitones",) + audio.VOICE_QUALITY_FIGURES + audio.FORMANT_FIGURES + audio.PERTURBATION_FIGURES + audio.HARMONIC_FIGURES
    sts = (audio.voice_quality_statistics(vq, voiced, fl), audio.formant_statistics(fm, voiced, fl),
           audio.perturbation_statistics(pt, voiced & (pt["lag"] > 0), fl), audio.harmonic_statistics(hm, voiced, fl, fm=fm))
    worst, checked = 0.0, 0
    for st, figs in zip(sts, (audio.VOICE_QUALITY_FIGURES, audio.FORMANT_FIGURES, audio.PERTURBATION_FIGURES, audio.HARMONIC_FIGURES)):
        for k in figs:
            a, b = vf[k]["mean"].cpu().numpy(), st[k].cpu().numpy()
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
            ok = ~np.isnan(b)
            if ok.any():
                worst = max(worst, float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))))
            checked += int(ok.sum())
    pr = audio.prosody_statistics(pitch["f0"], voiced, fl)
    want = 12.0 * np.log2(np.stack([pr[k].double().cpu().numpy() for k in ("f0_p05", "f0_median", "f0_p95")], axis=-1) / 27.5)
    got = vf["f0_semitones"]["percentiles"].cpu().numpy()
    dst = float(np.max(np.abs(got - want)))
    print(f"\nfunctionals voice_functionals: {checked} means against the statistics functions, worst relative difference {worst:.3e} (gate 1e-12); "
          f"f0_semitones percentiles against prosody_statistics {dst:.3e} semitones (gate 1e-4); medians {got[:, 1].round(2).tolist()}, "
          f"voiced segments per second {vf['segments']['voiced_per_s'].cpu().numpy().round(2).tolist()}")
    assert checked >= 2 * 15 and worst <= 1e-12
    assert np.isfinite(want).all() and dst <= 1e-4
    assert abs(got[0, 1] - 12.0 * np.log2(120.0 / 27.5)) < 0.5 and abs(got[1, 1] - 12.0 * np.log2(180.0 / 27.5)) < 0.5
    seg = {k: v.cpu().numpy() for k, v in vf["segments"].items()}
    assert (seg["voiced_per_s"] > 0).all() and (seg["voiced_mean_s"] > 0.02).all() and np.isfinite(seg["voiced_sd_s"]).all()
    assert int(vf["f0_semitones"]["valid"][0]) == int(pr["voiced_fraction"][0] * fl[0] + 0.5)


# ---- 5. the CLI -----------------------------------------------------------------------------------------------------------------------------------------
def swept_pulses(n, f_lo, f_hi, sr=22050):
    """n samples of perturbation_ref's pulse with the pitch moving linearly from f_lo to f_hi Hz; float32, peak about 0.5."""
    onsets, t = [], 0.37 * sr / f_lo
    while t < n:
        onsets.append(t)
        t += sr / (f_lo + (f_hi - f_lo) * t / n)
    d = np.arange(n, dtype=np.float64)[:, None] - np.array(onsets)[None, :]
    return (0.5 * np.where(d > 0, P.pulse(np.maximum(d, 0.0), sr), 0.0).sum(axis=1)).astype(np.float32)


def _wavs(tmp_path):
    from emojivoice_amd import cli

    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    sig = [swept_pulses(16000, 115.0, 130.0), swept_pulses(19000, 100.0, 190.0),
           (0.01 * np.random.default_rng(22).standard_normal(3000)).astype(np.float32)]      # (noise alone: no voiced frame)
    for name, y in zip(names, sig):
        cli.write_wav_pcm16(tmp_path / name, y, 22050)
    return cli, names


def test_voice_report_with_functionals(tmp_path):
    cli, names = _wavs(tmp_path)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{tmp_path / name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    plain = cli.cli(["--voice_report", str(flist), "--batch_size", "2"])
    rep = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--functionals"])
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    extra = {"functionals", "segments"}
    assert [set(f_) - extra for f_ in saved["files"]] == [set(f_) for f_ in plain["files"]] and not extra & set(plain["files"][0])
    assert set(saved["overall"]) - extra == set(plain["overall"]) and not extra & set(plain["overall"]) and set(saved) == set(plain)
    assert all(saved["files"][i][k] == plain["files"][i][k] for i in range(3) for k in plain["files"][i]), "the flag changes none of the other figures"
    contours = ["f0_semitones"] + list(audio.VOICE_QUALITY_FIGURES)
    a, b, c = saved["files"]
    for f_ in saved["files"]:
        assert list(f_["functionals"]) == contours and all(tuple(v) == cli.FUNCTIONAL_REPORT_KEYS for v in f_["functionals"].values())
        assert tuple(f_["segments"]) == cli.SEGMENT_REPORT_KEYS
    fa, fb = a["functionals"]["f0_semitones"], b["functionals"]["f0_semitones"]
    print(f"\nfunctionals --voice_report --functionals: f0_semitones {fa} / {fb}; segments {a['segments']} / {b['segments']} / {c['segments']}")
    assert all(c["functionals"][k][s] is None for k in contours for s in ("mean", "sd", "p20", "p50", "p80", "range", "rise_mean", "fall_sd")), "noise: nulls"
    assert c["segments"]["voiced_mean_s"] is None and c["segments"]["voiced_per_s"] == 0.0 and c["voiced_frames"] == 0
    assert all(isinstance(f_[k], float) for f_ in (fa, fb) for k in ("mean", "sd", "p20", "p50", "p80", "range", "peaks_per_s"))
    assert fb["range"] > fa["range"] > 0.0 and fb["sd"] > fa["sd"] > 0.0, "the wider pitch sweep has the larger range and sd"
    assert abs(fa["range"] - 0.6 * 12.0 * np.log2(130.0 / 115.0)) < 0.5 and 2.0 < fb["range"] < 12.0 * np.log2(190.0 / 100.0)    # (b's slow start is unvoiced)
    assert fb["rise_mean"] is not None and fb["rise_mean"] > 0.0
    for f_ in (a, b):
        for k in audio.VOICE_QUALITY_FIGURES:
            assert abs(f_["functionals"][k]["mean"] - f_[k]) <= 1e-12 * abs(f_[k]), "the functionals' mean is the report's own mean"
    s7, s12 = saved["speakers"]["7"], saved["speakers"]["12"]
    got = s7["functionals"]["f0_semitones"]["range"]
    assert got["files"] == 2 and abs(got["mean"] - 0.5 * (fa["range"] + fb["range"])) < 1e-12 and saved["overall"]["functionals"]["f0_semitones"]["range"] == got
    assert s12["functionals"]["f0_semitones"]["p50"] == {"mean": None, "files": 0} and saved["overall"]["segments"]["voiced_per_s"]["files"] == 3
    every = cli.cli(["--voice_report", str(flist), "--batch_size", "3", "--functionals", "--formants", "--perturbation", "--harmonics"])
    want = contours + list(audio.FORMANT_FIGURES) + list(audio.PERTURBATION_FIGURES) + list(audio.HARMONIC_FIGURES)
    assert [list(f_["functionals"]) for f_ in every["files"]] == [want] * 3 and list(every["overall"]["functionals"]) == want
    for k in audio.FORMANT_FIGURES + audio.PERTURBATION_FIGURES + audio.HARMONIC_FIGURES:
        for f_ in every["files"][:2]:
            assert (f_[k] is None and f_["functionals"][k]["mean"] is None) or abs(f_["functionals"][k]["mean"] - f_[k]) <= 1e-12 * abs(f_[k]), k
    assert every["files"][1]["functionals"]["f0_semitones"] == fb, "one batch of three or batches of two: the same figures"


def test_functionals_without_voice_report_is_rejected():
    import argparse

    from emojivoice_amd import cli

    with pytest.raises(AssertionError, match="--functionals"):
        cli.validate_args(argparse.Namespace(functionals=True, evaluate_pairs=None, voice_report=None, sample_rate=None, prepare_dataset=None))
