"""ev_load_voice_quality / ev_voice_quality on the MI355X, through the C ABI, and what stands on them (audio.voice_quality,
audio.voice_quality_statistics, --voice_report, --evaluate_pairs --voice_quality).

Yardstick: tests/voice_quality_ref.py, the numpy float64 restatement of the definition in include/emojivoice.h (two matrix products with the
same basis formulas).  The device sums in the matrix instruction's own order, so it differs from the restatement by float64 rounding.  The rule
of every comparison (``check``):
  * first, conditions on the INPUT, not on the device: the float64 and the longdouble restatements agree within 1e-11 max(|ref|, 1) on every
    entry and on every q*, and every non-silent frame's two largest cepstral values of the search range lie at least 1e-6 apart (at worst
    7.5e-13 and 6.2e-5 for the rows below), so no frame is left out of the comparison;
  * d_peak EQUAL;
  * every entry of d_frame and d_cepstrum within 1e-9 max(|ref|, 1): the project's float64 margin (tests/test_gpu_stoi.py,
    tests/test_gpu_loudness.py, tests/test_gpu_stft_dist.py), four orders above float64 order effects.
Observed on the MI355X: d_frame 5.1e-13 (slope_0_500 at 1024 / 256 / 1024) and d_cepstrum 8.8e-14 at worst over all cases, every q* equal.
Every case prints its worst figure, DESIGN section 3.19 records them; the gate stays at 1e-9.  Every raw call writes into buffers with sentinel
margins (tests/analysis_gpu.py); 50.0 sits behind every row's length.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import voice_quality_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

SMALL = R.GEOMETRIES[0]                  # 64 / 10 / 24: NB = 33, NQ = 29
BIG = R.GEOMETRIES[3]
_REF = {}


def ref_of(key, x, lens, g):
    """The restatements' results (float64: frame, peak, cepstrum, margin; longdouble: frame, peak, cepstrum), computed once per case and never
    modified."""
    return A.frozen(_REF, key, lambda: R.batch(x, lens, g) + R.batch(x, lens, g, dtype=np.longdouble)[:3])


def load(eng, g, null=(), **kw):
    """ev_load_voice_quality with the geometry's tables; ``kw`` overrides an argument, ``null`` names tables passed as NULL."""
    t = R.tables(g)
    a = dict(W=g.W, H=g.H, nfft=g.nfft, q_fit=g.q_fit, q_min=g.q_min, q_max=g.q_max, q_mean=t["q_mean"])
    a.update({k: v for k, v in kw.items() if k in a})
    arr = {}
    for name, dt in (("window", np.float64), ("twiddle", np.float64), ("bands", np.int32), ("slope_w", np.float64), ("fit_w", np.float64)):
        default = R.hann(a["W"]) if name == "window" else R.twiddle(a["nfft"]) if name == "twiddle" else t[name]
        arr[name] = np.ascontiguousarray(kw.get(name, default), dtype=dt)
    p = lambda name: None if name in null else arr[name].ctypes.data
    return eng.lib.ev_load_voice_quality(eng.h, p("window"), p("twiddle"), a["W"], a["H"], a["nfft"], p("bands"), p("slope_w"), a["q_fit"], a["q_min"],
                                         a["q_max"], p("fit_w"), float(a["q_mean"]))


def raw(eng, g, x, lens, floor=R.POWER_FLOOR, B=None, L=None, null=()):
    """ev_voice_quality into guarded buffers: (rc, frame (B, NF, 8), peak (B, NF), cepstrum (B, NF, NQ)) on the host; an output named in
    ``null`` is passed as NULL and comes back None.  ``B`` / ``L`` override the shape passed to the library."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    NF, NQ = R.frames(Lx, g.H), g.q_max - g.q_fit + 1
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"frame": ((Bx, NF, 8), torch.float64), "peak": ((Bx, NF), torch.int32), "cepstrum": ((Bx, NF, NQ), torch.float64)}, null)
    rc = eng.lib.ev_voice_quality(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, float(floor),
                                  out.ptr("frame"), out.ptr("peak"), out.ptr("cepstrum"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    frame, peak, cep = dev
    rf, rp, rc, mg, lf, lp, lc = ref
    e_in = max(R.err(rf, lf), R.err(rc, lc))
    assert e_in <= R.INPUT_TOL, f"{what}: the float64 and longdouble restatements differ by {e_in:.3e}, over {R.INPUT_TOL:g}: the input is ill-conditioned"
    assert np.array_equal(rp, lp), f"{what}: the float64 and longdouble restatements disagree on a q*"
    assert mg.min() >= R.MIN_PEAK_MARGIN, f"{what}: a peak margin of {mg.min():.3e}, under {R.MIN_PEAK_MARGIN:g}"
    per = [R.err(frame[..., i], rf[..., i]) for i in range(8)]
    e_c = R.err(cep, rc) if cep is not None else 0.0
    print(f"\nvoice quality {what}: d_frame err per figure {[f'{e:.1e}' for e in per]}  d_cepstrum err {e_c:.3e} (gate {R.TOL:g})  restatement float64 "
          f"against longdouble {e_in:.3e}  smallest peak margin {mg.min():.3e}  q* differing {int((peak != rp).sum())}  silent or empty frames "
          f"{int((rp == 0).sum())} of {rp.size}")
    assert np.array_equal(peak, rp), f"{what}: d_peak"
    assert max(per) <= R.TOL, f"{what}: d_frame"
    assert e_c <= R.TOL, f"{what}: d_cepstrum"
    assert not frame[rp == 0][:, [0, 1, 2, 3, 4, 6, 7]].any() and (cep is None or not cep[rp == 0].any()), f"{what}: exact zeros on silent and empty frames"


def engine_with(g):
    return A.engine_with(load, g)


@pytest.fixture(scope="module")
def engines():
    yield from A.engines_on_demand(engine_with)


@pytest.fixture(scope="module")
def small(engines):
    return engines(SMALL)


# ---- 1. the four geometries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GEOMETRIES, ids=R.IDS)
def test_geometry_against_the_restatement(engines, g):
    x, lens = R.rows_for(g)
    ref = ref_of(("rows", g), x, lens, g)
    nfs = [R.frames(n, g.H) for n in lens]
    assert [n % 16 for n in nfs] == [15, 0, 1]
    eng = engines(g)
    rc, *dev = raw(eng, g, x, lens)
    assert rc == 0, err_of(eng)
    check(dev, ref, f"{g[:6]} lens {lens}")
    for b in range(3):
        assert not dev[0][b, nfs[b]:].any() and not dev[1][b, nfs[b]:].any() and not dev[2][b, nfs[b]:].any(), "zeros past the row's own frames"
        assert (dev[1][b, :nfs[b]] > 0).sum() > nfs[b] // 2, "most frames are not silent"
    means = [np.round(dev[0][b, :nfs[b]][dev[1][b, :nfs[b]] > 0][:, :5].mean(axis=0), 3).tolist() for b in range(3)]
    print(f"voice quality {g[:6]}: mean cpp / alpha / hammarberg / slope0 / slope1 over the non-silent frames of each row {means}")


@pytest.mark.parametrize("g", R.EDGE_GEOMETRIES, ids=[f"{g.nfft}-{g.H}-{g.W}" for g in R.EDGE_GEOMETRIES])
def test_edge_geometry_against_the_restatement(engines, g):
    """The same check where the skew walk and the K loops take their rare paths: H < 4, a skew of 3, W / 4 = 3 and W / 4 = 4 (one whole round), one bin tile (waves
    1-3 hand over their identities), three phase-2 steps, half a quefrency tile."""
    test_geometry_against_the_restatement(engines, g)


# ---- 2. invariance ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", (SMALL, BIG), ids=(R.IDS[0], R.IDS[3]))
def test_row_alone_in_a_batch_as_a_prefix_and_without_cepstrum_give_the_same_bits(engines, g):
    eng = engines(g)
    x, lens = R.rows_for(g, seed=40)
    n = lens[0]
    c = x[0, :n].copy()
    rc, *alone = raw(eng, g, c[None], None)
    assert rc == 0, err_of(eng)
    rc, *again = raw(eng, g, c[None], None)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    rc, f2, p2, none = raw(eng, g, c[None], None, null=("cepstrum",))
    assert rc == 0 and none is None and np.array_equal(f2, alone[0]) and np.array_equal(p2, alone[1]), "d_cepstrum = NULL"
    xb, _, lb = R.padded([(x[2, :lens[2]],) * 2, (c, c), (x[1, :lens[1]],) * 2])
    rc, *batch = raw(eng, g, xb, lb)
    assert rc == 0
    xp, _, lp = R.padded([(x[1, :lens[1]],) * 2, (c, c)], L=n + 1235)
    xp[1, n:] = -7.5e3                                                   # other garbage than in the batch of three
    rc, *prefix = raw(eng, g, xp, lp)
    assert rc == 0
    nf = R.frames(n, g.H)
    assert (alone[1][0] > 0).any()
    for name, other in (("inside a batch", batch), ("the prefix of a padded row", prefix)):
        for i, out in enumerate(("d_frame", "d_peak", "d_cepstrum")):
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
    NB = g.nfft // 2 + 1
    x, lens = R.rows_for(g)
    L = x.shape[1]
    hole = x[0].copy()
    hole[700:1500] = 0.0                                                 # digital silence in the middle of a row
    x = np.concatenate([x, np.zeros((1, L), np.float32), hole[None], x[:1], x[:1], x[:1]])
    lens = lens + [2000, lens[0], 0, -3, L + 1]
    rc, frame, peak, cep = raw(small, g, x, lens)
    assert rc == 0, err_of(small)
    ref = ref_of("degenerate", x, lens, g)
    check((frame, peak, cep), ref, "a zero row, a row with a silent middle and bad rows beside good ones")
    nfz = R.frames(2000, g.H)
    assert not peak[3].any() and not cep[3].any() and not frame[3][:, [0, 1, 2, 3, 4, 6, 7]].any(), "a zero row: every frame is silent"
    assert (frame[3, :nfz, 5] == frame[3, 0, 5]).all() and abs(frame[3, 0, 5] - NB * R.POWER_FLOOR) < 1e-18 and not frame[3, nfz:].any(), "NB clamped bins"
    mid = slice(700 // g.H + 2, 1500 // g.H - 2)
    assert not peak[4, mid].any() and not cep[4, mid].any() and (frame[4, mid, 5] > 0).all() and (peak[4, :60] > 0).all()
    for b in (5, 6, 7):
        assert not frame[b].any() and not peak[b].any() and not cep[b].any(), "len 0, len < 0, len > L: rows of zeros"


def test_a_row_of_one_sample_has_one_frame(small):
    """One sample is an impulse: a flat spectrum, whose cepstrum past q = 0 is summation noise (about 1e-15) and whose peak is arbitrary, so
    the figures that hang on q* are held to that noise and the others to the restatement."""
    g = SMALL
    x, lens = R.rows_for(g)
    for xs, ls in ((x[:2], [1, lens[1]]), (x[:2, :1], None)):            # a row of 1 sample beside a good row; L = 1: NF = 1
        rc, frame, peak, cep = raw(small, g, xs, ls)
        assert rc == 0, err_of(small)
        want = R.batch(xs, ls, g)[0]
        assert g.q_min <= peak[0, 0] <= g.q_max and not peak[0, 1:].any() and not frame[0, 1:].any() and not cep[0, 1:].any()
        assert R.err(frame[0, 0, 1:6], want[0, 0, 1:6]) <= R.TOL and frame[0, 0, 5] > (g.nfft // 2 + 1) * R.POWER_FLOOR
        assert np.abs(cep[0, 0]).max() < 1e-12 and np.abs(frame[0, 0, [0, 6, 7]]).max() < 1e-12
    assert frame.shape == (2, 1, 8)


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
    check(dev, ref, f"edges {g[:6]} lens {lens}")
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
    ("d_frame", dict(null=("frame",))), ("d_peak", dict(null=("peak",))), ("d_x", dict(null=("x",))),
]


@pytest.mark.parametrize("word,kw", BAD_CALL, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_of_ev_voice_quality_fails_with_a_message_naming_it(small, word, kw):
    z = np.zeros((2, 256), np.float32)
    rc, *_ = raw(small, SMALL, z, None, **kw)                             # (a failed call writes nothing: raw checks that)
    msg = err_of(small)
    assert rc != 0 and "ev_voice_quality" in msg and word in msg, msg


def _with(a, i, v):
    a = np.array(a, copy=True)
    a.reshape(-1)[i] = v
    return a


_T = R.tables(SMALL)
BAD_LOAD = [
    ("nfft=", dict(nfft=14, W=12)), ("nfft=", dict(nfft=1026, W=1024)), ("nfft=", dict(nfft=65, W=25)), ("W=", dict(W=2)), ("W=", dict(W=68)), ("W=", dict(W=26)),
    ("nfft - W", dict(nfft=66, W=25)), ("H=", dict(H=0)), ("H=", dict(H=513)),
    ("bands[0]", dict(bands=_with(_T["bands"], 0, -1))), ("bands[1]", dict(bands=_with(_T["bands"], 3, 34))), ("bands[2]", dict(bands=_with(_T["bands"], 5, 0))),
    ("bands[3]", dict(bands=_with(_T["bands"], 6, 20))), ("bands[4]", dict(bands=_with(_T["bands"], 9, 1))), ("bands[5]", dict(bands=_with(_T["bands"], 10, 10))),
    ("q_fit=", dict(q_fit=0)), ("q_fit=", dict(q_fit=5)), ("q_min=", dict(q_min=31)), ("q_max=", dict(q_max=33)), ("q_fit=", dict(q_fit=2, q_min=2, q_max=2)),
    ("window[5]", dict(window=_with(R.hann(24), 5, float("nan")))), ("twiddle[15]", dict(twiddle=_with(R.twiddle(64), 15, float("inf")))),
    ("slope_w[40]", dict(slope_w=_with(_T["slope_w"], 40, float("nan")))), ("fit_w[3]", dict(fit_w=_with(_T["fit_w"], 3, float("-inf")))),
    ("q_mean", dict(q_mean=float("nan"))),
    ("non-null", dict(null=("window",))), ("non-null", dict(null=("twiddle",))), ("non-null", dict(null=("bands",))), ("non-null", dict(null=("slope_w",))),
    ("non-null", dict(null=("fit_w",))),
]


@pytest.mark.parametrize("word,kw", BAD_LOAD, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_LOAD)])
def test_each_limit_of_ev_load_voice_quality_fails_with_a_message_naming_it(small, word, kw):
    kw = dict(kw)
    null = kw.pop("null", ())
    if "q_max" in kw and "fit_w" not in kw:                               # (a table as long as the quefrency range asks for)
        kw["fit_w"] = np.zeros(max(kw["q_max"] - kw.get("q_fit", SMALL.q_fit) + 1, 1))
    if "q_fit" in kw and "fit_w" not in kw:
        kw["fit_w"] = np.zeros(max(kw.get("q_max", SMALL.q_max) - kw["q_fit"] + 1, 1))
    n0 = small.alloc_count()
    rc = load(small, SMALL, null=null, **kw)
    msg = err_of(small)
    assert rc != 0 and "ev_load_voice_quality" in msg and word in msg, msg
    assert small.alloc_count() == n0
    x, lens = R.rows_for(SMALL)                                           # the tables loaded before are still the ones in use
    ref = ref_of(("rows", SMALL), x, lens, SMALL)
    rc, frame, peak, _ = raw(small, SMALL, x[:1], lens[:1])
    nf = R.frames(lens[0], SMALL.H)
    assert rc == 0 and np.array_equal(peak[0, :nf], ref[1][0, :nf]) and R.err(frame[0, :nf], ref[0][0, :nf]) <= R.TOL


def test_a_call_before_a_load_fails_loading_again_replaces_the_tables_and_calls_allocate_nothing():
    e = Engine(0)
    try:
        z = np.zeros((1, 256), np.float32)
        rc, *_ = raw(e, SMALL, z, None)
        assert rc != 0 and "ev_load_voice_quality" in err_of(e)
        n0 = e.alloc_count()
        assert load(e, R.GEOMETRIES[2]) == 0, err_of(e)
        assert e.alloc_count() == n0 + 1, "the tables are one device block that counts in ev_alloc_count"
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


# ---- 6. audio.voice_quality -----------------------------------------------------------------------------------------------------------------------
def test_audio_voice_quality_on_three_ragged_rows():
    lens = [4000, 2600, 700]
    sig = [R.speech_like(n, seed=30 + i, fs=R.FS) for i, n in enumerate(lens)]
    x, _, _ = R.padded([(s, s) for s in sig])
    xd = torch.from_numpy(x).to(DEV)
    t = audio.voice_quality_tables(22050, 1024, 65.0, 600.0)
    g = R.Geometry(1024, 256, 1024, t["q_fit"], t["q_min"], t["q_max"], BIG.bands, 22050)
    out = audio.voice_quality(xd, lengths=lens)
    eng = audio._voice_quality_engine(xd.device, 22050, 1024, 256, 65.0, 600.0)
    n0 = eng.alloc_count()
    out2 = audio.voice_quality(xd, lengths=lens)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0 and eng is audio._voice_quality_engine(xd.device, 22050, 1024, 256, 65.0, 600.0), "one cached engine, no allocation"
    ref = ref_of("audio", x, lens, g)
    F = R.frames(x.shape[1], 256)
    keys = audio.VOICE_QUALITY_FIGURES + ("power",)
    for k in keys:
        assert out[k].dtype == torch.float64 and out[k].shape == (3, F) and torch.equal(out[k], out2[k]), k
    frame = np.stack([out[k].cpu().numpy() for k in keys] + [ref[0][..., 6], ref[0][..., 7]], axis=-1)
    peak = out["peak_quefrency"].cpu().numpy()
    assert out["peak_quefrency"].dtype == torch.int32 and out["cepstral_f0"].dtype == torch.float32
    check((frame, peak, None), ref, "audio.voice_quality 4000 / 2600 / 700 samples")
    f0 = out["cepstral_f0"].cpu().numpy()
    want = np.where(peak > 0, 22050.0 / np.maximum(peak, 1), 0.0)
    assert not f0[peak == 0].any() and np.abs(f0 - want).max() <= 2.0 ** -23 * want.max(), "sr / q*, to float32 rounding"
    one = audio.voice_quality(xd[0, :lens[0]])
    nf = R.frames(lens[0], 256)
    assert one["cpp_db"].shape == (1, nf) and torch.equal(one["cpp_db"][0], out["cpp_db"][0, :nf]), "a 1-D input is the same row"


def test_a_147_hz_tone_and_the_statistics_under_pitch_yin_s_mask():
    n = 16384
    tone = torch.from_numpy(R.harmonic_tone(n)).to(DEV)
    x = torch.stack([tone, torch.zeros_like(tone)])
    x[1, :5000] = torch.from_numpy(R.speech_like(5000, seed=3, fs=R.FS)).to(DEV)
    lens = [n, 5000]
    vq = audio.voice_quality(x, lengths=lens)
    whole = slice(2, n // 256 - 2)
    assert (vq["peak_quefrency"][0, whole] == 150).all() and ((vq["cepstral_f0"][0, whole] - 22050.0 / 150.0).abs() <= 147.0 * 2.0 ** -23).all()
    pitch = audio.pitch_yin(x, lengths=lens)
    assert pitch["voiced"].shape == vq["cpp_db"].shape, "the frames line up"
    fl = [R.frames(v, 256) for v in lens]
    st = audio.voice_quality_statistics(vq, pitch["voiced"], lengths=fl)
    voiced, peak = pitch["voiced"].cpu().numpy(), vq["peak_quefrency"].cpu().numpy()
    use = voiced & (peak > 0) & (np.arange(peak.shape[1])[None, :] < np.array(fl)[:, None])
    assert st["frames"].cpu().tolist() == use.sum(axis=1).tolist() and use[0].sum() > 50 and use[1].sum() > 3
    for k in audio.VOICE_QUALITY_FIGURES:
        v = vq[k].cpu().numpy()
        for b in range(2):
            assert abs(float(st[k][b]) - v[b][use[b]].mean()) <= 1e-12 * max(1.0, abs(v[b][use[b]].mean())), (k, b)
    none = audio.voice_quality_statistics(vq, torch.zeros_like(pitch["voiced"]))
    assert none["frames"].tolist() == [0, 0] and all(torch.isnan(none[k]).all() for k in audio.VOICE_QUALITY_FIGURES)
    print(f"\nvoice quality, 147 Hz tone: cpp {float(st['cpp_db'][0]):.3f} dB over {int(st['frames'][0])} voiced frames; speech-like row: "
          f"{ {k: round(float(st[k][1]), 3) for k in audio.VOICE_QUALITY_FIGURES} }")


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------------------
def _wavs(tmp_path, short):
    from emojivoice_amd import cli

    sr = 22050
    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    for i, name in enumerate(names):
        cli.write_wav_pcm16(tmp_path / name, R.speech_like((16000, 19000, short)[i], seed=20 + i, fs=sr), sr)
    return cli, names


def test_voice_report(tmp_path):
    cli, names = _wavs(tmp_path, 300)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{tmp_path / name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    rep = cli.cli(["--voice_report", str(flist), "--batch_size", "2"])
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    figs = set(audio.VOICE_QUALITY_FIGURES)
    assert [set(f_) for f_ in saved["files"]] == [{"path", "speaker", "seconds", "frames", "voiced_frames"} | figs] * 3
    a, b, c = saved["files"]
    print(f"\nvoice quality --voice_report: {[[f_['voiced_frames']] + [f_[k] for k in audio.VOICE_QUALITY_FIGURES] for f_ in saved['files']]}")
    assert a["frames"] == 63 and b["frames"] == 75 and c["frames"] == 2 and a["voiced_frames"] > 5 and b["voiced_frames"] > 5
    assert c["voiced_frames"] == 0 and all(c[k] is None for k in figs), "300 samples: no voiced frame"
    assert all(isinstance(f_[k], float) and np.isfinite(f_[k]) for f_ in (a, b) for k in figs)
    s7, s12 = saved["speakers"]["7"], saved["speakers"]["12"]
    assert set(s7) == {"files", "voiced_frames"} | figs == set(saved["overall"])
    assert s7["files"] == 2 and s7["voiced_frames"] == a["voiced_frames"] + b["voiced_frames"] == saved["overall"]["voiced_frames"] and saved["overall"]["files"] == 3
    for k in figs:
        pooled = (a[k] * a["voiced_frames"] + b[k] * b["voiced_frames"]) / (a["voiced_frames"] + b["voiced_frames"])
        assert abs(s7[k] - pooled) <= 1e-9 * max(1.0, abs(pooled)) and saved["overall"][k] == s7[k] and s12[k] is None
    assert s12["voiced_frames"] == 0 and s12["files"] == 1


def test_evaluate_pairs_with_voice_quality(tmp_path):
    cli, names = _wavs(tmp_path, 600)                                    # (600 samples: the shortest a mel takes, still no voiced frame)
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(f"{tmp_path / 'a.wav'}|{tmp_path / 'b.wav'}|7\n{tmp_path / 'b.wav'}|{tmp_path / 'a.wav'}|7\n{tmp_path / 'a.wav'}|{tmp_path / 'c.wav'}|12\n",
                     encoding="utf-8")
    plain = cli.cli(["--evaluate_pairs", str(pairs)])
    rep = cli.cli(["--evaluate_pairs", str(pairs), "--voice_quality"])
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    figs = set(audio.VOICE_QUALITY_FIGURES)
    assert all("voice" not in p for p in plain["pairs"]) and "voice" not in plain["overall"] and all("voice" not in s for s in plain["speakers"].values())
    assert [set(p) - {"voice"} for p in saved["pairs"]] == [set(p) for p in plain["pairs"]], "without the flag the key sets are the old ones"
    assert set(saved["overall"]) - {"voice"} == set(plain["overall"]) and set(saved) == set(plain)
    p0, p1, p2 = saved["pairs"]
    for p in saved["pairs"]:
        assert set(p["voice"]) == {"recorded", "synthesised", "delta"} and all(set(p["voice"][k]) == figs for k in p["voice"])
    for k in figs:
        assert abs(p0["voice"]["delta"][k] - (p0["voice"]["synthesised"][k] - p0["voice"]["recorded"][k])) < 1e-12
        assert abs(p0["voice"]["delta"][k] + p1["voice"]["delta"][k]) < 1e-12, "the swapped pair has the opposite deltas"
        assert p2["voice"]["synthesised"][k] is None and p2["voice"]["delta"][k] is None and isinstance(p2["voice"]["recorded"][k], float)
        s7 = saved["speakers"]["7"]["voice"][k]
        assert set(s7) == {"mean_delta", "mean_abs_delta"} and abs(s7["mean_delta"]) < 1e-12 and abs(s7["mean_abs_delta"] - abs(p0["voice"]["delta"][k])) < 1e-12
        assert saved["speakers"]["12"]["voice"][k] == {"mean_delta": None, "mean_abs_delta": None}
        assert abs(saved["overall"]["voice"][k]["mean_abs_delta"] - s7["mean_abs_delta"]) < 1e-12
