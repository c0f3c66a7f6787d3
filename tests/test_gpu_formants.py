"""ev_load_formants / ev_formants on the MI355X, through the C ABI, and what stands on them (audio.formants, audio.formant_statistics,
--voice_report --formants, --evaluate_pairs --formants).

Yardstick: tests/formants_ref.py, the numpy float64 restatement of the definition in include/emojivoice.h (Burg's lattice, the Aberth-Ehrlich
iteration under the same stop rule, the band and rank rules).  The device sums in one fixed order of its own, so it differs from the restatement
by float64 rounding.  The rule of every comparison (``check``):
  * first, conditions on the INPUT, not on the device: the float64 and the longdouble restatements agree within 1e-11 max(|ref|, 1) on every
    coefficient, frequency and bandwidth and give equal counts, both converge within 32 iterations on every frame, and every root's frequency
    keeps 1e-3 Hz from both band edges, so no frame is left out of the comparison;
  * d_count EQUAL;
  * every entry of d_lpc and d_formant within 1e-9 max(|ref|, 1): the project's float64 margin (tests/test_gpu_voice_quality.py).
Observed on the MI355X: d_lpc 2.1e-14, frequency 3.1e-14 and bandwidth 4.4e-14 at worst over all cases, every count equal, at most 15 iterations.
Every case prints its worst figure, DESIGN section 3.20 records them; the gate stays at 1e-9.  Every raw call writes into buffers with sentinel
margins (tests/analysis_gpu.py); 50.0 sits behind every row's length.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import formants_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

SMALL = R.GEOMETRIES[0]
BIG = R.GEOMETRIES[3]
_REF = {}


def ref_of(key, x, lens, g):
    """The restatements' results (float64: lpc, formant, count, iters, margin; longdouble: the same five), computed once per case and never
    modified."""
    return A.frozen(_REF, key, lambda: R.batch(x, lens, g) + R.batch(x, lens, g, dtype=np.longdouble))


def load(eng, g, null=False, window=None, **kw):
    """ev_load_formants with the geometry's arguments; ``kw`` overrides one, ``null`` passes the window as NULL."""
    a = dict(W=g.W, H=g.H, order=g.order, pre=g.pre, sr=g.sr, f_lo=g.f_lo, nform=g.nform)
    a.update(kw)
    w = np.ascontiguousarray(R.formant_window(max(a["W"], 1)) if window is None else window, dtype=np.float64)
    return eng.lib.ev_load_formants(eng.h, None if null else w.ctypes.data, a["W"], a["H"], a["order"], float(a["pre"]), float(a["sr"]), float(a["f_lo"]),
                                    a["nform"])


def raw(eng, g, x, lens, floor=R.POWER_FLOOR, B=None, L=None, null=()):
    """ev_formants into guarded buffers: (rc, lpc (B, NF, p + 2), formant (B, NF, nform, 2), count (B, NF)) on the host; an output named in
    ``null`` is passed as NULL and comes back None.  ``B`` / ``L`` override the shape passed to the library."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    NF = R.frames(Lx, g.H)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"lpc": ((Bx, NF, g.order + 2), torch.float64), "formant": ((Bx, NF, g.nform, 2), torch.float64), "count": ((Bx, NF), torch.int32)},
                    null)
    rc = eng.lib.ev_formants(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, float(floor),
                             out.ptr("lpc"), out.ptr("formant"), out.ptr("count"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    lpc, fm, ct = dev
    rl, rf, rc, ri, mg, ll, lf, lc, li, _ = ref
    e_in = max(R.err(rl, ll), R.err(rf, lf))
    assert e_in <= R.INPUT_TOL, f"{what}: the float64 and longdouble restatements differ by {e_in:.3e}, over {R.INPUT_TOL:g}: the input is ill-conditioned"
    assert np.array_equal(rc, lc), f"{what}: the float64 and longdouble restatements disagree on a count"
    assert ri.min() >= 0 and li.min() >= 0 and max(ri.max(), li.max()) <= R.MAX_REF_ITERS, f"{what}: a restatement needs {max(ri.max(), li.max())} iterations"
    assert mg.min() >= R.MIN_FREQ_MARGIN, f"{what}: a root {mg.min():.3e} Hz from a band edge, under {R.MIN_FREQ_MARGIN:g}"
    e_l = R.err(lpc, rl) if lpc is not None else 0.0
    e_f, e_b = R.err(fm[..., 0], rf[..., 0]), R.err(fm[..., 1], rf[..., 1])
    print(f"\nformants {what}: d_lpc err {e_l:.3e}  frequency err {e_f:.3e}  bandwidth err {e_b:.3e} (gate {R.TOL:g})  restatement float64 against "
          f"longdouble {e_in:.3e}  iterations at most {int(ri.max())}  smallest band margin {mg.min():.3e} Hz  counts differing {int((ct != rc).sum())}  "
          f"silent or empty frames {int((ri == 0).sum())} of {ri.size}  counts {np.bincount(rc.ravel() + 1).tolist()} from -1")
    assert np.array_equal(ct, rc), f"{what}: d_count"
    assert e_l <= R.TOL, f"{what}: d_lpc"
    assert max(e_f, e_b) <= R.TOL, f"{what}: d_formant"
    assert not fm[ri == 0].any() and (lpc is None or not lpc[ri == 0].any()), f"{what}: exact zeros on silent and empty frames"
    assert np.isfinite(fm).all() and (lpc is None or np.isfinite(lpc).all())


def engine_with(g):
    return A.engine_with(load, g)


@pytest.fixture(scope="module")
def engines():
    yield from A.engines_on_demand(engine_with)


@pytest.fixture(scope="module")
def small(engines):
    return engines(SMALL)


# ---- 1. the six geometries --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GEOMETRIES + R.EDGE_GEOMETRIES, ids=R.IDS + R.EDGE_IDS)
def test_geometry_against_the_restatement(engines, g):
    """Four frames to a workgroup: the rows' frame counts leave 3, 0 and 1.  The edge geometries: W = 8 (56 lanes hold no sample, order 2: one
    pair of roots), W = 70 (two samples in 6 lanes, one in 58), hops that are no multiple of anything."""
    x, lens = R.rows_for(g)
    ref = ref_of(("rows", g), x, lens, g)
    nfs = [R.frames(n, g.H) for n in lens]
    assert [n % 4 for n in nfs] == [3, 0, 1] and max(lens) <= 8000
    eng = engines(g)
    rc, *dev = raw(eng, g, x, lens)
    assert rc == 0, err_of(eng)
    check(dev, ref, f"{g[:4]} lens {lens}")
    for b in range(3):
        assert not dev[0][b, nfs[b]:].any() and not dev[1][b, nfs[b]:].any() and not dev[2][b, nfs[b]:].any(), "zeros past the row's own frames"
        assert (dev[2][b, :nfs[b]] > 0).sum() > nfs[b] // 2, "most frames have formants"
    f = dev[1][..., 0]
    later = np.arange(1, g.nform)[None, None, :] < dev[2][..., None]
    assert (f[..., 1:][later] > f[..., :-1][later]).all() and (f[..., 0][dev[2] > 0] > g.f_lo).all(), "ascending frequencies inside the band"
    full = dev[2] == dev[2].max()
    print(f"formants {g[:4]}: mean frequencies over the {int(full.sum())} frames with {dev[2].max()} formants {np.round(f[full].mean(axis=0), 1).tolist()}")


# ---- 2. invariance ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", (SMALL, BIG, R.EDGE_GEOMETRIES[1]), ids=(R.IDS[0], R.IDS[3], R.EDGE_IDS[1]))
def test_row_alone_in_a_batch_as_a_prefix_and_without_lpc_give_the_same_bits(engines, g):
    eng = engines(g)
    x, lens = R.rows_for(g, seed=40)
    n = lens[0]
    c = x[0, :n].copy()
    rc, *alone = raw(eng, g, c[None], None)
    assert rc == 0, err_of(eng)
    rc, *again = raw(eng, g, c[None], None)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    rc, none, f2, c2 = raw(eng, g, c[None], None, null=("lpc",))
    assert rc == 0 and none is None and np.array_equal(f2, alone[1]) and np.array_equal(c2, alone[2]), "d_lpc = NULL"
    xb, _, lb = R.padded([(x[2, :lens[2]],) * 2, (c, c), (x[1, :lens[1]],) * 2])
    rc, *batch = raw(eng, g, xb, lb)
    assert rc == 0
    xp, _, lp = R.padded([(x[1, :lens[1]],) * 2, (c, c)], L=n + 1235)
    xp[1, n:] = -7.5e3                                                   # other garbage than in the batch of three
    rc, *prefix = raw(eng, g, xp, lp)
    assert rc == 0
    nf = R.frames(n, g.H)
    assert (alone[2][0] > 0).any()
    for name, other in (("inside a batch", batch), ("the prefix of a padded row", prefix)):
        for i, out in enumerate(("d_lpc", "d_formant", "d_count")):
            assert np.array_equal(alone[i][0, :nf], other[i][1, :nf]) and not other[i][1, nf:].any(), f"{out}: alone against {name}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 3, 6):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, g, xb, lb)
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


# ---- 3. degenerate inputs -----------------------------------------------------------------------------------------------------------------------
def test_silent_frames_and_bad_rows(small):
    g = SMALL
    x, lens = R.rows_for(g)
    L = x.shape[1]
    hole = x[0].copy()
    hole[700:1500] = 0.0                                                 # digital silence in the middle of a row
    x = np.concatenate([x, np.zeros((1, L), np.float32), hole[None], x[:1], x[:1], x[:1]])
    lens = lens + [2000, lens[0], 0, -3, L + 1]
    rc, lpc, fm, ct = raw(small, g, x, lens)
    assert rc == 0, err_of(small)
    ref = ref_of("degenerate", x, lens, g)
    check((lpc, fm, ct), ref, "a zero row, a row with a silent middle and bad rows beside good ones")
    assert not lpc[3].any() and not fm[3].any() and not ct[3].any(), "a zero row: every frame is silent"
    mid = slice(700 // g.H + 3, 1500 // g.H - 3)
    assert not lpc[4, mid].any() and not fm[4, mid].any() and not ct[4, mid].any() and (ct[4, :40] > 0).any()
    for b in (5, 6, 7):
        assert not lpc[b].any() and not fm[b].any() and not ct[b].any(), "len 0, len < 0, len > L: rows of zeros"


def test_a_row_of_one_sample_has_one_frame(small):
    """One sample under the floor (1e-6: E0 = 1.3e-13) is a silent frame: count 0, zeros.  One sample over it is, after the pre-emphasis, the
    two-tap response {w, -pre w'}: by the definition a frame like any other, whose all-pole model has roots inside the band (the restatement
    gives count 2 at 24 / 10 / order 4), so it is held to the restatement like every frame; nothing is non-finite in either."""
    g = SMALL
    x, lens = R.rows_for(g)
    quiet = x[:2].copy()
    quiet[0, 0] = 1e-6
    for xs, ls in ((quiet, [1, lens[1]]), (quiet[:1, :1], None)):
        rc, lpc, fm, ct = raw(small, g, xs, ls)
        assert rc == 0, err_of(small)
        assert not ct[0].any() and not fm[0].any() and not lpc[0].any(), "under the floor: a silent frame"
        assert np.isfinite(lpc).all() and np.isfinite(fm).all()
    assert ct.shape == (1, 1)
    for i, (xs, ls) in enumerate(((x[:2], [1, lens[1]]), (x[:2, :1], None), (np.full((1, 1), 0.5, np.float32), None))):
        rc, lpc, fm, ct = raw(small, g, xs, ls)
        assert rc == 0, err_of(small)
        check((lpc, fm, ct), ref_of(("one sample", i), xs, ls, g), f"a row of one sample, case {i}")
        assert not ct[0, 1:].any() and not fm[0, 1:].any() and not lpc[0, 1:].any()
        print(f"formants, a row of one sample: count {ct[0, 0]}, E0 {lpc[0, 0, -1]:.3e}, formants {fm[0, 0].ravel().round(2).tolist()}")


def test_a_pure_tone_converges_with_finite_outputs(engines):
    """A 147 Hz tone is rank-deficient for an order-10 predictor: the restatements differ by 5e-11 there, over the input condition, so only
    convergence and finiteness are held."""
    g = R.GEOMETRIES[2]
    x = R.tone(4000, g.sr)[None]
    rc, lpc, fm, ct = raw(engines(g), g, x, None)
    assert rc == 0
    print(f"\nformants, 147 Hz tone: counts {np.bincount(ct.ravel() + 1).tolist()} from -1; lowest formant {fm[0, 2:-2, 0, 0].min():.2f} .. {fm[0, 2:-2, 0, 0].max():.2f} Hz")
    assert (ct >= 1).all() and np.isfinite(lpc).all() and np.isfinite(fm).all()


# ---- 4. the edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", (SMALL, R.GEOMETRIES[2]), ids=(R.IDS[0], R.IDS[2]))
def test_zeros_outside_the_row_at_both_ends(engines, g):
    """A signal that is zero except inside its first and last W / 2 samples: staging with a reflection instead of zeros would show in the first
    and last frames."""
    eng = engines(g)
    sig = [R.edge_signal(n, g.W, seed=i) for i, n in enumerate((3000, 3000 + g.H // 2 + 1))]
    x, _, lens = R.padded([(s, s) for s in sig])
    ref = ref_of(("edge", g), x, lens, g)
    rc, *dev = raw(eng, g, x, lens)
    assert rc == 0, err_of(eng)
    check(dev, ref, f"edges {g[:4]} lens {lens}")
    for b, n in enumerate(lens):
        nf = R.frames(n, g.H)
        bad = R.row(x[b, :n], g, mutant="reflect")[0]
        for f in (0, nf - 1):
            moved = np.abs(bad[f] - ref[0][b, f]).max()
            assert moved > 1e-6, f"row {b} frame {f}: the reflect mutant would not show ({moved:.3e})"
            assert R.err(dev[0][b, f], ref[0][b, f]) <= R.TOL


# ---- 5. limits and loading ----------------------------------------------------------------------------------------------------------------------
BAD_CALL = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)), ("power_floor", dict(floor=0.0)), ("power_floor", dict(floor=-1e-7)),
    ("power_floor", dict(floor=float("inf"))), ("power_floor", dict(floor=float("nan"))),
    ("d_formant", dict(null=("formant",))), ("d_count", dict(null=("count",))), ("d_x", dict(null=("x",))),
]


@pytest.mark.parametrize("word,kw", BAD_CALL, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_of_ev_formants_fails_with_a_message_naming_it(small, word, kw):
    z = np.zeros((2, 256), np.float32)
    rc, *_ = raw(small, SMALL, z, None, **kw)                             # (a failed call writes nothing: raw checks that)
    msg = err_of(small)
    assert rc != 0 and "ev_formants" in msg and word in msg, msg


def _with(a, i, v):
    a = np.array(a, copy=True)
    a.reshape(-1)[i] = v
    return a


BAD_LOAD = [
    ("order=", dict(order=1)), ("order=", dict(order=33, W=128)), ("W=", dict(W=7, order=2)), ("W=", dict(W=1025)), ("W=", dict(W=8, order=4)),
    ("W=", dict(W=64, order=32)), ("H=", dict(H=0)), ("H=", dict(H=513)), ("n_formants=", dict(nform=0)), ("n_formants=", dict(nform=17)),
    ("pre_emphasis=", dict(pre=-0.1)), ("pre_emphasis=", dict(pre=1.0)), ("pre_emphasis=", dict(pre=float("nan"))),
    ("sr=", dict(sr=0.0)), ("sr=", dict(sr=float("inf"))), ("sr=", dict(sr=float("nan"))),
    ("f_lo=", dict(f_lo=0.0)), ("f_lo=", dict(f_lo=500.0)), ("f_lo=", dict(f_lo=float("nan"))),
    ("window[5]", dict(window=_with(R.formant_window(24), 5, float("nan")))), ("window[23]", dict(window=_with(R.formant_window(24), 23, float("inf")))),
    ("window", dict(null=True)),
]


@pytest.mark.parametrize("word,kw", BAD_LOAD, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_LOAD)])
def test_each_limit_of_ev_load_formants_fails_with_a_message_naming_it(small, word, kw):
    n0 = small.alloc_count()
    rc = load(small, SMALL, **kw)
    msg = err_of(small)
    assert rc != 0 and "ev_load_formants" in msg and word in msg, msg
    assert small.alloc_count() == n0
    x, lens = R.rows_for(SMALL)                                           # the tables loaded before are still the ones in use
    ref = ref_of(("rows", SMALL), x, lens, SMALL)
    rc, lpc, fm, ct = raw(small, SMALL, x[:1], lens[:1])
    nf = R.frames(lens[0], SMALL.H)
    assert rc == 0 and np.array_equal(ct[0, :nf], ref[2][0, :nf]) and R.err(fm[0, :nf], ref[1][0, :nf]) <= R.TOL and R.err(lpc[0, :nf], ref[0][0, :nf]) <= R.TOL


def test_a_call_before_a_load_fails_loading_again_replaces_the_tables_and_calls_allocate_nothing():
    e = Engine(0)
    try:
        z = np.zeros((1, 256), np.float32)
        rc, *_ = raw(e, SMALL, z, None)
        assert rc != 0 and "ev_load_formants" in err_of(e)
        n0 = e.alloc_count()
        assert load(e, R.GEOMETRIES[2]) == 0, err_of(e)
        assert e.alloc_count() == n0 + 1, "the window is one device block that counts in ev_alloc_count"
        assert load(e, SMALL) == 0 and e.alloc_count() == n0 + 2
        x, lens = R.rows_for(SMALL)
        rc, *dev = raw(e, SMALL, x, lens)
        assert rc == 0, err_of(e)
        check(dev, ref_of(("rows", SMALL), x, lens, SMALL), "after loading twice")
        n1 = e.alloc_count()
        assert n1 == n0 + 2, "a call allocates nothing"
        rc, *dev2 = raw(e, SMALL, x, lens)
        torch.cuda.synchronize()
        assert rc == 0 and e.alloc_count() == n1 and all(np.array_equal(a, b) for a, b in zip(dev, dev2)), "a second call at the same shape allocates nothing"
    finally:
        e.close()


# ---- 6. audio.formants ------------------------------------------------------------------------------------------------------------------------------
def test_audio_formants_on_three_ragged_rows():
    lens = [4000, 2600, 700]
    sig = [R.speech_like(n, seed=18 * i, fs=22050) for i, n in enumerate(lens)]    # (seeds whose rows open with sound)
    x, _, _ = R.padded([(s, s) for s in sig])
    xd = torch.from_numpy(x).to(DEV)
    out = audio.formants(xd, lengths=lens)
    geo = audio.formant_geometry()
    assert (geo["d"], geo["sr"], geo["W"], geo["H"], geo["order"]) == (2, 11025.0, 512, 128, 13)
    eng = audio._formant_engine(xd.device, geo["sr"], geo["W"], geo["H"], geo["order"], 4, 50.0, geo["pre"])
    n0 = eng.alloc_count()
    out2 = audio.formants(xd, lengths=lens)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0 and eng is audio._formant_engine(xd.device, geo["sr"], geo["W"], geo["H"], geo["order"], 4, 50.0, geo["pre"]), \
        "one cached engine, no allocation"
    F = R.frames(x.shape[1], 256)
    assert out["frequency"].shape == out["bandwidth"].shape == (3, F, 4) and out["frequency"].dtype == torch.float64
    assert out["count"].shape == out["gain"].shape == (3, F) and out["count"].dtype == torch.int32 and out["lpc"].shape == (3, F, 13)
    assert all(torch.equal(out[k], out2[k]) for k in out)
    # the restatement at the decimated rate, on the rows the device's own resampler made
    dl = [-(-n // 2) for n in lens]
    xr = audio.resample(xd, 2, 1, lens).cpu().numpy()
    g = R.geometry(11025.0, 512, 128, 13, pre=geo["pre"])
    ref = ref_of("audio", xr, dl, g)
    assert R.frames(xr.shape[1], 128) == F and [R.frames(n, 128) for n in dl] == [R.frames(n, 256) for n in lens], "the frames line up"
    lpc = np.concatenate([out["lpc"].cpu().numpy(), out["gain"].cpu().numpy()[..., None], ref[0][..., -1:]], axis=-1)
    fm = np.stack([out["frequency"].cpu().numpy(), out["bandwidth"].cpu().numpy()], axis=-1)
    check((lpc, fm, out["count"].cpu().numpy()), ref, "audio.formants 4000 / 2600 / 700 samples at 22050 Hz")
    pitch = audio.pitch_yin(xd, lengths=lens)
    assert pitch["voiced"].shape == out["count"].shape, "the frames line up with pitch_yin"
    fl = [R.frames(n, 256) for n in lens]
    st = audio.formant_statistics(out, pitch["voiced"], lengths=fl)
    voiced, ct = pitch["voiced"].cpu().numpy(), out["count"].cpu().numpy()
    use = voiced & (ct >= 3) & (np.arange(F)[None, :] < np.array(fl)[:, None])
    assert st["frames"].cpu().tolist() == use.sum(axis=1).tolist() and use[0].sum() > 3 and st["unconverged_frames"].cpu().tolist() == [0, 0, 0]
    for i in range(3):
        ok = use & (fm[..., i, 1] <= 700.0)
        for b in range(3):
            for name, v in ((f"f{i + 1}_hz", fm[b, :, i, 0]), (f"b{i + 1}_hz", fm[b, :, i, 1])):
                got = float(st[name][b])
                assert (np.isnan(got) and not ok[b].any()) or abs(got - v[ok[b]].mean()) <= 1e-12 * max(1.0, abs(v[ok[b]].mean())), (name, b)
    one = audio.formants(xd[0, :lens[0]])
    nf = R.frames(lens[0], 256)
    assert one["frequency"].shape == (1, nf, 4) and torch.equal(one["frequency"][0], out["frequency"][0, :nf]), "a 1-D input is the same row"
    print(f"formants, speech-like rows: {[{k: round(float(st[k][b]), 1) for k in audio.FORMANT_FIGURES} for b in range(3)]}")
    with pytest.raises(ValueError, match="multiples"):
        audio.formants(xd, hop_length=255)


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------------------
def _wavs(tmp_path, short):
    from emojivoice_amd import cli

    sr = 22050
    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    for i, name in enumerate(names):
        cli.write_wav_pcm16(tmp_path / name, R.speech_like((16000, 19000, short)[i], seed=20 + i, fs=sr), sr)
    return cli, names


FORMANT_KEYS = set(audio.FORMANT_FIGURES) | {"formant_frames", "unconverged_frames"}


def test_voice_report_with_formants(tmp_path):
    cli, names = _wavs(tmp_path, 300)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{tmp_path / name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    plain = cli.cli(["--voice_report", str(flist), "--batch_size", "2"])
    rep = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--formants"])
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert [set(f_) - FORMANT_KEYS for f_ in saved["files"]] == [set(f_) for f_ in plain["files"]] and not FORMANT_KEYS & set(plain["files"][0])
    assert set(saved["overall"]) - FORMANT_KEYS == set(plain["overall"]) and not FORMANT_KEYS & set(plain["overall"])
    assert all(FORMANT_KEYS <= set(f_) for f_ in saved["files"]) and FORMANT_KEYS <= set(saved["overall"]) and FORMANT_KEYS <= set(saved["speakers"]["7"])
    a, b, c = saved["files"]
    print(f"\nformants --voice_report --formants: {[[f_[k] for k in ('formant_frames',) + audio.FORMANT_FIGURES] for f_ in saved['files']]}")
    assert a["formant_frames"] > 5 and b["formant_frames"] > 5 and c["formant_frames"] == 0 and all(c[k] is None for k in audio.FORMANT_FIGURES)
    assert all(f_["unconverged_frames"] == 0 for f_ in saved["files"])
    assert all(isinstance(f_[k], float) and np.isfinite(f_[k]) for f_ in (a, b) for k in audio.FORMANT_FIGURES)
    assert 150.0 < a["f1_hz"] < a["f2_hz"] < a["f3_hz"] < 5500.0
    s7 = saved["speakers"]["7"]
    assert s7["formant_frames"] == a["formant_frames"] + b["formant_frames"] == saved["overall"]["formant_frames"]
    lo, hi = min(a["f1_hz"], b["f1_hz"]), max(a["f1_hz"], b["f1_hz"])
    assert lo - 1e-9 <= s7["f1_hz"] <= hi + 1e-9 and saved["overall"]["f1_hz"] == s7["f1_hz"] and saved["speakers"]["12"]["f1_hz"] is None


def test_evaluate_pairs_with_formants(tmp_path):
    cli, names = _wavs(tmp_path, 600)
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(f"{tmp_path / 'a.wav'}|{tmp_path / 'b.wav'}|7\n{tmp_path / 'b.wav'}|{tmp_path / 'a.wav'}|7\n{tmp_path / 'a.wav'}|{tmp_path / 'c.wav'}|12\n",
                     encoding="utf-8")
    plain = cli.cli(["--evaluate_pairs", str(pairs)])
    rep = cli.cli(["--evaluate_pairs", str(pairs), "--formants"])
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    figs = set(audio.FORMANT_FIGURES)
    assert all("formants" not in p for p in plain["pairs"]) and "formants" not in plain["overall"]
    assert [set(p) - {"formants"} for p in saved["pairs"]] == [set(p) for p in plain["pairs"]], "without the flag the key sets are the old ones"
    assert set(saved["overall"]) - {"formants"} == set(plain["overall"]) and set(saved) == set(plain)
    p0, p1, p2 = saved["pairs"]
    for p in saved["pairs"]:
        assert set(p["formants"]) == {"recorded", "synthesised", "delta"} and all(set(p["formants"][k]) == figs for k in p["formants"])
    for k in figs:
        assert abs(p0["formants"]["delta"][k] - (p0["formants"]["synthesised"][k] - p0["formants"]["recorded"][k])) < 1e-9
        assert abs(p0["formants"]["delta"][k] + p1["formants"]["delta"][k]) < 1e-9, "the swapped pair has the opposite deltas"
        assert p2["formants"]["synthesised"][k] is None and p2["formants"]["delta"][k] is None and isinstance(p2["formants"]["recorded"][k], float)
        s7 = saved["speakers"]["7"]["formants"][k]
        assert set(s7) == {"mean_delta", "mean_abs_delta"} and abs(s7["mean_delta"]) < 1e-9 and abs(s7["mean_abs_delta"] - abs(p0["formants"]["delta"][k])) < 1e-9
        assert saved["speakers"]["12"]["formants"][k] == {"mean_delta": None, "mean_abs_delta": None}
        assert abs(saved["overall"]["formants"][k]["mean_abs_delta"] - s7["mean_abs_delta"]) < 1e-9
