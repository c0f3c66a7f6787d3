"""ev_harmonics on the MI355X, through the C ABI, and what stands on it (audio.harmonics, audio.harmonic_statistics, --voice_report --harmonics,
--evaluate_pairs --harmonics).

Yardstick: tests/harmonics_ref.py, the numpy restatement of the definition in include/emojivoice.h, in float64 and in longdouble.  The tests hand
over d_period and d_formant of their own, so only the spectrum differs between device and restatement.  The rule of every comparison (``check``):
  * first, conditions on the INPUT, computed from the restatements alone: float64 and longdouble agree within 1e-11 and on every k*, h_i, A3 range
    and count; the two largest Ldb of every searched range lie at least 1e-6 dB apart; every argument of a floor, a ceil or the resolution
    threshold lies at least 1e-9 from its boundary.  No frame is left out (tests/test_harmonics_host.py checks the same on the CPU);
  * d_count EQUAL and every k* equal (rint(f_h nfft / sr - the restatement's shift) against the restatement's k*);
  * every entry of d_frame and d_harm within 1e-9 max(|ref|, 1), the project's float64 margin, and exactly zero where the restatement is.
Every case prints its worst figures and its smallest margins; DESIGN section 3.22 records them.  Every raw call writes into buffers with 64-element
sentinel margins (tests/analysis_gpu.py); 50.0 lies behind every row's length, and a period behind a row's frames.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import harmonics_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

_CASES, _REF, _LOADED = {}, {}, {}


def case(g):
    """(x, lens, period, formant, fcount) of a geometry, made once and never modified."""
    return A.frozen(_CASES, g, lambda: R.case(g))


def ref_of(g):
    """(float64 result, the conditions' report) of a geometry's case, computed once and never modified."""
    x, lens, period, formant, fcount = case(g)
    return A.frozen(_REF, g, lambda: R.conditions(x, lens, period, g, formant, fcount))


def load(eng, g, **kw):
    """ev_load_harmonics of the geometry (skipped when it is the one loaded); ``kw`` overrides an argument or names a table to pass as NULL."""
    a = g._asdict()
    null = kw.pop("null", ())
    window, tw = kw.pop("window", None), kw.pop("twiddle", None)
    a.update(kw)
    if not kw and not null and window is None and tw is None and _LOADED.get(id(eng)) == g:
        return 0
    t = R.tables(R.Geometry(a["nfft"], a["H"], a["W"], a["sr"], a["n_harm"])) if 16 <= a["nfft"] <= 4096 and 4 <= a["W"] <= a["nfft"] else R.tables(g)
    w = np.ascontiguousarray(t["window"] if window is None else window)
    tw = np.ascontiguousarray(t["twiddle"] if tw is None else tw)
    rc = eng.lib.ev_load_harmonics(eng.h, None if "window" in null else w.ctypes.data, None if "twiddle" in null else tw.ctypes.data, a["W"], a["H"],
                                   a["nfft"], float(a["sr"]), a["n_harm"], float(a["search"]), float(a["min_spacing"]), float(a["a3_range"]))
    if rc == 0:
        _LOADED[id(eng)] = g if not kw else None
    return rc


def raw(eng, g, x, lens, period, formant=None, fcount=None, B=None, L=None, null=(), nform=None, floor=R.POWER_FLOOR):
    """ev_harmonics into guarded buffers: (rc, frame (B, NF, 8), count (B, NF, 2), harm (B, NF, n_harm, 2)) on the host; an argument named in
    ``null`` is passed as NULL (an output then comes back None).  ``B`` / ``L`` / ``nform`` override what is passed to the library."""
    x = torch.tensor(np.array(x, dtype=np.float32)).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    NF = R.frames(Lx, g.H)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    d_per = torch.tensor(np.array(period, dtype=np.float32).reshape(Bx, NF)).to(DEV)
    d_fm = None if formant is None else torch.tensor(np.array(formant, dtype=np.float64)).to(DEV)
    d_fc = None if fcount is None else torch.tensor(np.array(fcount, dtype=np.int32)).to(DEV)
    nform = (0 if formant is None else int(np.asarray(formant).shape[2])) if nform is None else nform
    out = A.Guarded({"frame": ((Bx, NF, 8), torch.float64), "count": ((Bx, NF, 2), torch.int32), "harm": ((Bx, NF, g.n_harm, 2), torch.float64)}, null)
    opt = lambda name, t: None if t is None or name in null else t.data_ptr()
    rc = eng.lib.ev_harmonics(eng.h, opt("x", x), opt("len", d_len), B, L, opt("period", d_per), opt("formant", d_fm), opt("fcount", d_fc), nform,
                              float(floor), out.ptr("frame"), out.ptr("count"), out.ptr("harm"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def check(dev, r64, rep, g, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    fr, ct, hm = dev
    errs = [R.err(fr[..., i], r64["frame"][..., i]) for i in range(8)]
    e_hz, e_db = R.err(hm[..., 0], r64["harm"][..., 0]), R.err(hm[..., 1], r64["harm"][..., 1])
    meas = r64["kstar"] >= 0
    k_dev = np.rint(hm[..., 0] / (float(g.sr) / float(g.nfft)) - r64["shift"]).astype(np.int64)
    k_diff = int((k_dev[meas] != r64["kstar"][meas]).sum())
    print(f"\nharmonics {what}: worst d_frame err {max(errs):.3e} ({', '.join(f'{n} {e:.1e}' for n, e in zip(R.FIGURES, errs))}), d_harm Hz {e_hz:.3e} "
          f"dB {e_db:.3e} (gate {R.TOL:g});  float64 against longdouble {rep['input_err']:.3e};  counts differing {int((ct != r64['count']).sum())}, k* "
          f"differing {k_diff} of {rep['searched']};  smallest margin {rep['min_margin']:.2e} dB, smallest rounding distance {rep['min_rounding']:.2e};  "
          f"frames voiced {rep['voiced']} unvoiced {rep['unvoiced']} unresolved {rep['unresolved']} silent {rep['silent']}, cut by n_harm "
          f"{rep['cut_by_n_harm']} by the Nyquist bin {rep['cut_by_nyquist']}, (frame, lane) pairs with 0 .. 4 harmonics {rep['lanes']}")
    assert rep["input_err"] <= R.INPUT_TOL and rep["decisions_equal"], f"{what}: float64 against longdouble"
    assert rep["min_margin"] >= R.MIN_PEAK_MARGIN and rep["min_rounding"] >= R.MIN_ROUND_MARGIN, f"{what}: a decision too close to call"
    assert np.array_equal(ct, r64["count"]), f"{what}: d_count"
    assert k_diff == 0, f"{what}: k*"
    assert np.isfinite(fr).all() and np.isfinite(hm).all() and max(errs) <= R.TOL and e_hz <= R.TOL and e_db <= R.TOL, f"{what}: d_frame / d_harm"
    assert not fr[r64["frame"] == 0].any() and not hm[r64["harm"] == 0].any(), f"{what}: exact zeros where the definition has them"


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------------------------
def test_a_call_before_a_load_fails_with_a_message():
    e = Engine(0)
    g = R.GEOMETRIES[0]
    rc, *_ = raw(e, g, np.zeros((1, 64), np.float32), None, np.zeros((1, R.frames(64, g.H)), np.float32))
    assert rc != 0 and "ev_harmonics" in err_of(e) and "not loaded" in err_of(e)
    with pytest.raises(Exception, match="not loaded"):
        e.harmonics(torch.zeros(1, 64, device=DEV), None, torch.zeros(1, 7, device=DEV))
    e.close()


@pytest.mark.parametrize("g", R.GEOMETRIES + R.EDGE_GEOMETRIES, ids=R.IDS)
def test_three_ragged_rows_against_the_restatement(eng, g):
    """15, 0 and 1 frames mod 16; voiced, unvoiced, unresolved and silent frames in every row; formants of the test's own with counts -1 .. 4."""
    x, lens, period, formant, fcount = case(g)
    r64, rep = ref_of(g)
    assert load(eng, g) == 0, err_of(eng)
    rc, *dev = raw(eng, g, x, lens, period, formant, fcount)
    assert rc == 0, err_of(eng)
    check(dev, r64, rep, g, f"{tuple(g)[:5]} lens {lens}")
    assert [R.frames(n, g.H) % 16 for n in lens] == [15, 0, 1]
    assert rep["voiced"] and rep["unvoiced"] and rep["unresolved"] and rep["silent"]
    fr, ct, hm = dev
    for b, n in enumerate(lens):
        nf = R.frames(n, g.H)
        assert not fr[b, nf:].any() and not ct[b, nf:].any() and not hm[b, nf:].any(), "zeros past the row's own frames"
    if g.nfft >= 64:
        assert (ct[..., 1] & 16).any() and (ct[..., 1] & 14).any() and (ct[..., 1] & 1).any(), "every flag is seen"


def test_the_cases_cover_what_the_kernel_can_meet():
    lanes = np.sum([ref_of(g)[1]["lanes"] for g in R.GEOMETRIES + R.EDGE_GEOMETRIES], axis=0)
    assert lanes[0] and lanes[1] and lanes[4], "lanes with 0, 1 and 4 harmonics"
    reps = [ref_of(g)[1] for g in R.GEOMETRIES]
    assert any(r["cut_by_n_harm"] for r in reps) and any(r["cut_by_nyquist"] for r in reps)


def test_degenerate_rows(eng):
    g = R.GEOMETRIES[0]
    x, lens, period, formant, fcount = case(g)
    assert load(eng, g) == 0, err_of(eng)
    r64, _ = ref_of(g)
    bad = [0, x.shape[1] + 1, lens[2]]
    rc, fr, ct, hm = raw(eng, g, x, bad, period, formant, fcount)
    assert rc == 0, err_of(eng)
    assert not fr[:2].any() and not ct[:2].any() and not hm[:2].any(), "len 0 and len > L: rows of zeros"
    assert R.err(fr[2], r64["frame"][2]) <= R.TOL and np.array_equal(ct[2], r64["count"][2]), "the good row beside them"
    one = np.full((1, 1), 0.5, np.float32)
    rc, fr, ct, hm = raw(eng, g, one, None, np.full((1, 1), g.nfft / 5.3, np.float32))
    ref = R.batch(one, None, np.full((1, 1), g.nfft / 5.3, np.float32), g)
    assert rc == 0 and fr.shape == (1, 1, 8) and np.array_equal(ct, ref["count"]) and R.err(fr, ref["frame"]) <= R.TOL and R.err(hm, ref["harm"]) <= R.TOL
    odd = np.array([[np.nan, -3.0, np.inf, 1e-30, 0.0, 1e30, 2.0]], np.float32)   # NaN, negative: unvoiced; inf, huge: unresolved; tiny: no harmonic
    n = 7 * g.H
    xs = np.asarray(x[2:3, :n])
    rc, fr, ct, hm = raw(eng, g, xs, None, odd)
    assert rc == 0 and not ct.any() and not hm.any() and not fr[..., :7].any(), "periods that admit no harmonic"
    assert fr[0, 0, 7] == 0 and fr[0, 1, 7] == 0 and fr[0, 4, 7] == 0 and fr[0, 2, 7] == 0 and fr[0, 6, 7] == g.nfft / 2.0 and fr[0, 3, 7] == g.nfft / np.float64(np.float32(1e-30))


def test_ties_go_to_the_lowest_bin(eng):
    """A noise-free band-limited tone: above its partials every bin is the power floor's dB value on the device and in the restatement alike, so
    those ranges are exact ties; every other range keeps its margin and no raw power lies near the floor."""
    g = R.GEOMETRIES[3]
    x, T = R.tie_row(g)
    period = np.full((1, R.frames(len(x), g.H)), T, np.float32)
    r64, rld = R.batch(x[None], None, period, g), R.batch(x[None], None, period, g, dtype=np.longdouble)
    m = r64["margin"][np.isfinite(r64["margin"])]
    power = R.spectrum(x, g)
    assert (m == 0).sum() > 100 and m[m > 0].min() >= R.MIN_PEAK_MARGIN and np.array_equal(r64["kstar"], rld["kstar"])
    assert (np.abs(power - R.POWER_FLOOR) >= 1e-6 * R.POWER_FLOOR).all() and r64["rounding"].min() >= R.MIN_ROUND_MARGIN
    assert load(eng, g) == 0, err_of(eng)
    rc, fr, ct, hm = raw(eng, g, x[None], None, period)
    assert rc == 0, err_of(eng)
    meas = r64["kstar"] >= 0
    k_dev = np.rint(hm[..., 0] / (float(g.sr) / float(g.nfft)) - r64["shift"]).astype(np.int64)
    other = R.batch(x[None], None, period, g, mutant="tie_high")
    print(f"\nharmonics ties: {int((m == 0).sum())} of {m.size} searched ranges are ties; 'the highest k of a tie' moves {int((other['kstar'] != r64['kstar']).sum())} "
          f"peaks; k* differing on the device {int((k_dev[meas] != r64['kstar'][meas]).sum())}; d_harm err {R.err(hm, r64['harm']):.3e}")
    assert (other["kstar"] != r64["kstar"]).sum() > 100
    assert np.array_equal(ct, r64["count"]) and np.array_equal(k_dev[meas], r64["kstar"][meas])
    assert R.err(fr, r64["frame"]) <= R.TOL and R.err(hm, r64["harm"]) <= R.TOL


# ---- 2. the identities ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", (R.GEOMETRIES[0], R.GEOMETRIES[2], R.EDGE_GEOMETRIES[0]), ids=(R.IDS[0], R.IDS[2], R.IDS[5]))
def test_row_alone_in_a_batch_as_a_prefix_without_outputs_twice_and_under_every_arithmetic_give_the_same_bits(eng, g):
    x, lens, period, formant, fcount = case(g)
    assert load(eng, g) == 0, err_of(eng)
    i0 = int(np.argmax((ref_of(g)[0]["count"][..., 1] > 1).sum(axis=1)))   # the row with the most frames that carry a formant figure
    i1, i2 = [i for i in range(3) if i != i0]
    n = lens[i0]
    nf = R.frames(n, g.H)
    c = np.asarray(x[i0, :n]).copy()
    n0 = eng.alloc_count()
    args1 = (period[i0:i0 + 1, :nf], formant[i0:i0 + 1, :nf], fcount[i0:i0 + 1, :nf])
    rc, *alone = raw(eng, g, c[None], None, *args1)
    assert rc == 0, err_of(eng)
    rc, *again = raw(eng, g, c[None], None, *args1)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    rc, f2, c2, none = raw(eng, g, c[None], None, *args1, null=("harm",))
    assert rc == 0 and none is None and np.array_equal(f2, alone[0]) and np.array_equal(c2, alone[1]), "d_harm = NULL"
    rc, f3, c3, h3 = raw(eng, g, c[None], None, args1[0])
    assert rc == 0 and np.array_equal(h3, alone[2]), "d_formant = NULL: the harmonics"
    assert all(np.array_equal(f3[..., i], alone[0][..., i]) for i in (0, 5, 6, 7)) and not f3[..., 1:5].any(), "d_formant = NULL: entries 0, 5, 6, 7"
    assert np.array_equal(c3[..., 0], alone[1][..., 0]) and np.array_equal(c3[..., 1], alone[1][..., 1] & 1), "d_formant = NULL: n_h and bit 0"
    order = [i2, i0, i1]
    rc, *batch = raw(eng, g, np.asarray(x)[order], [lens[i] for i in order], period[order], formant[order], fcount[order])
    assert rc == 0
    Lp = n + 1235
    NFp = R.frames(Lp, g.H)
    xp = np.full((2, Lp), -7.5e3, np.float32)                              # other garbage than in the batch of three
    m1 = min(lens[i1], Lp)
    xp[0, :m1], xp[1, :n] = x[i1, :m1], c
    pp = np.full((2, NFp), g.nfft / 5.3, np.float32)                       # (a voiced period behind the row's own frames must not matter)
    fp, cp = np.full((2, NFp, formant.shape[2], 2), 333.0), np.full((2, NFp), 4, np.int32)
    nf1 = R.frames(m1, g.H)
    pp[0, :nf1], fp[0, :nf1], cp[0, :nf1] = period[i1, :nf1], formant[i1, :nf1], fcount[i1, :nf1]
    pp[1, :nf], fp[1, :nf], cp[1, :nf] = period[i0, :nf], formant[i0, :nf], fcount[i0, :nf]
    rc, *prefix = raw(eng, g, xp, [m1, n], pp, fp, cp)
    assert rc == 0
    assert (alone[1][0, :, 0] > 0).any() and (alone[1][0, :, 1] > 1).any()
    for what, other in (("inside a batch", batch), ("the prefix of a padded row", prefix)):
        for i, out in enumerate(("d_frame", "d_count", "d_harm")):
            assert np.array_equal(alone[i][0, :nf], other[i][1, :nf]), f"{out}: alone against {what}"
            assert not other[i][1, nf:].any(), f"{out}: past the row's frames, {what}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (16, 6, 0):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, g, np.asarray(x)[order], [lens[i] for i in order], period[order], formant[order], fcount[order])
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0, "ev_alloc_count does not move over calls"


def test_no_allocation_and_capturable():
    e = Engine(0)
    g = R.GEOMETRIES[0]
    x, lens, period, formant, fcount = case(g)
    t = R.tables(g)
    n_before = e.alloc_count()
    e.load_harmonics(t["window"], t["twiddle"], g.H, g.nfft, g.sr, g.n_harm, g.search, g.min_spacing, g.a3_range)
    assert e.alloc_count() == n_before + 1, "one device block, counted once"
    xd, ld = torch.tensor(np.array(x)).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    pd, fd, cd = torch.tensor(np.array(period)).to(DEV), torch.tensor(np.array(formant)).to(DEV), torch.tensor(np.array(fcount)).to(DEV)
    n0 = e.alloc_count()
    ref = e.harmonics(xd, ld, pd, fd, cd, R.POWER_FLOOR)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        e.harmonics(xd, ld, pd, fd, cd, R.POWER_FLOOR)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = e.harmonics(xd, ld, pd, fd, cd, R.POWER_FLOOR)
        for o in out:
            o.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b), "the replay equals the eager call"
    assert np.array_equal(out[1].cpu().numpy(), ref_of(g)[0]["count"])
    assert e.alloc_count() == n0
    e.close()


# ---- 3. limits ---------------------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
BAD_CALL = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)),
    ("power_floor=", dict(floor=0.0)), ("power_floor=", dict(floor=-1e-7)), ("power_floor=", dict(floor=INF)), ("power_floor=", dict(floor=NAN)),
    ("d_x", dict(null=("x",))), ("d_period", dict(null=("period",))), ("d_frame", dict(null=("frame",))), ("d_count", dict(null=("count",))),
    ("d_formant and d_fcount", dict(null=("formant",))), ("d_formant and d_fcount", dict(null=("fcount",))),
    ("n_formants=", dict(nform=0)), ("n_formants=", dict(nform=17)),
]


@pytest.mark.parametrize("word,kw", BAD_CALL, ids=[f"{w.strip('=').split()[0]}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_of_a_call_fails_with_a_message_naming_it_and_writes_nothing(eng, word, kw):
    g = R.GEOMETRIES[0]
    assert load(eng, g) == 0, err_of(eng)
    z = np.zeros((2, 256), np.float32)
    NF = R.frames(256, g.H)
    rc, *_ = raw(eng, g, z, None, np.full((2, NF), 12.3, np.float32), np.full((2, NF, 4, 2), 300.0), np.full((2, NF), 4, np.int32), **kw)
    msg = err_of(eng)                                                    # (a failed call writes nothing: raw checks that)
    assert rc != 0 and "ev_harmonics" in msg and word in msg, msg


def test_more_frames_than_a_tile_index_holds_fails_by_name():
    e = Engine(0)
    g = R.Geometry(16, 1, 8, 2000, 4)
    assert load(e, g) == 0, err_of(e)
    rc, *_ = raw(e, g, np.zeros((1, 32), np.float32), None, np.zeros((1, 32), np.float32), L=0x7fffffff)
    assert rc != 0 and "ev_harmonics" in err_of(e) and "more frames" in err_of(e), err_of(e)
    e.close()


BAD_LOAD = [
    ("nfft=", dict(nfft=14, W=12)), ("nfft=", dict(nfft=2050, W=64)), ("nfft=", dict(nfft=63, W=24)), ("W=", dict(W=22)), ("W=", dict(W=68)), ("W=", dict(W=0)),
    ("H=", dict(H=0)), ("H=", dict(H=513)), ("sr=", dict(sr=0.0)), ("sr=", dict(sr=INF)), ("sr=", dict(sr=NAN)),
    ("n_harm=", dict(n_harm=0)), ("n_harm=", dict(n_harm=65)), ("search=", dict(search=0.0)), ("search=", dict(search=0.51)), ("search=", dict(search=NAN)),
    ("min_spacing=", dict(min_spacing=1.9)), ("min_spacing=", dict(min_spacing=INF)), ("min_spacing=", dict(min_spacing=NAN)),
    ("a3_range=", dict(a3_range=-0.1)), ("a3_range=", dict(a3_range=0.6)), ("a3_range=", dict(a3_range=NAN)),
    ("non-null", dict(null=("window",))), ("non-null", dict(null=("twiddle",))), ("window[", dict(window="nan")), ("twiddle[", dict(twiddle="inf")),
    ("LDS", dict(nfft=2048, W=2048, H=512, n_harm=1)), ("LDS", dict(nfft=2048, W=2048, H=256, n_harm=48)),
]


def test_each_limit_of_a_load_fails_by_name_and_leaves_the_tables_in_use(eng):
    g = R.GEOMETRIES[0]
    x, lens, period, formant, fcount = case(g)
    assert load(eng, g) == 0, err_of(eng)
    rc, *before = raw(eng, g, x, lens, period, formant, fcount)
    assert rc == 0
    n0 = eng.alloc_count()
    for word, kw in BAD_LOAD:
        kw = dict(kw)
        for name in ("window", "twiddle"):
            if isinstance(kw.get(name), str):
                t = R.tables(g)[name].copy()
                t.reshape(-1)[3] = float(kw[name])
                kw[name] = t
        rc = load(eng, g, **kw)
        msg = err_of(eng)
        assert rc != 0 and "ev_load_harmonics" in msg and word in msg, (word, kw.keys(), msg)
    assert eng.alloc_count() == n0, "a failed load leaves the count unchanged"
    rc, *after = raw(eng, g, x, lens, period, formant, fcount)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(before, after)), "a failed load leaves the previous tables in use"
    _LOADED.pop(id(eng), None)
    assert load(eng, R.GEOMETRIES[1]) == 0 and eng.alloc_count() == n0 + 1, "loading again: one block more in the count"
    assert load(eng, g) == 0 and eng.alloc_count() == n0 + 2
    rc, *third = raw(eng, g, x, lens, period, formant, fcount)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(before, third)), "loading again gives the same tables"
    assert load(eng, g, nfft=2048, W=2048, H=256, n_harm=32, sr=R.FS) == 0, "nfft = 2048 with H = 256 fits"
    _LOADED.pop(id(eng), None)


# ---- 4. audio.harmonics ----------------------------------------------------------------------------------------------------------------------------------
def vowel(n, f0=147.0, seed=0, tilt_db=0.0, noise=1e-4):
    """(x float32, a): a harmonic complex with formant-shaped amplitudes: a_h = 0.05 10^(-tilt_db (h - 1) / 20) / h times the gain of three
    resonances (650 / 1100 / 2550 Hz, 90 / 110 / 170 Hz wide) at h f0, partials below 5 kHz."""
    rng = np.random.default_rng(800 + seed)
    t = np.arange(n, dtype=np.float64) / R.FS
    hs = np.arange(1, int(5000.0 // f0) + 1)
    f = hs * f0
    gain = np.ones_like(f)
    for F, bw in ((650.0, 90.0), (1100.0, 110.0), (2550.0, 170.0)):
        gain *= (F * F + 0.25 * bw * bw) / np.sqrt((f * f - F * F) ** 2 + (bw * f) ** 2 + 1e-9)
    a = 0.05 * 10.0 ** (-tilt_db * (hs - 1) / 20.0) / hs * gain
    x = sum(a[h - 1] * np.sin(2 * np.pi * h * f0 * t + 0.37 * h * h) for h in hs) + noise * rng.standard_normal(n)
    return x.astype(np.float32), a


def test_audio_harmonics_on_three_ragged_rows_against_the_restatement():
    """1024 / 256 at 22050 Hz on 6000 / 4100 / 2600 samples; the restatement is fed the device's own periods (ev_pitch_yin) and formants (ev_formants)."""
    lens = [6000, 4100, 2600]
    x = np.full((3, 6000 + 29), R.GARBAGE, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = vowel(n, (147.0, 203.0, 118.0)[b], seed=b, tilt_db=0.3 * b)[0]
    g = R.Geometry(1024, 256, 1024, R.FS, 48)
    xd = torch.from_numpy(x).to(DEV)
    out = audio.harmonics(xd, lengths=lens)
    eng = audio._harmonics_engine(xd.device, 22050, 1024, 256, 48, 0.25, 4.0, 0.1)
    n0 = eng.alloc_count()
    out2 = audio.harmonics(xd, lengths=lens)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0, "no allocation"
    F = R.frames(x.shape[1], 256)
    assert set(out) == {"h1_h2_db", "h1_a3_db", "f1_rel_db", "f2_rel_db", "f3_rel_db", "h1_db", "h1_hz", "spacing_bins", "n_harmonics", "flags",
                        "harmonic_hz", "harmonic_db"}
    assert out["h1_h2_db"].shape == (3, F) and out["h1_h2_db"].dtype == torch.float64 and out["harmonic_db"].shape == (3, F, 48)
    assert out["n_harmonics"].dtype == out["flags"].dtype == torch.int32 and out["flags"].shape == (3, F)
    assert all(torch.equal(out[k], out2[k]) for k in out)
    tau_min, tau_max = audio.pitch_lag_range(22050, 65.0, 600.0)
    _, period, _ = audio._trim_engine(xd.device).pitch_yin(xd, torch.tensor(lens), 1024, 256, tau_min, tau_max, want_lag=False, want_cmnd=False)
    fm = audio.formants(xd, lengths=lens)
    fmt = torch.stack((fm["frequency"], fm["bandwidth"]), dim=-1).cpu().numpy()
    r64, rep = R.conditions(x, lens, period.cpu().numpy(), g, fmt, fm["count"].cpu().numpy())
    fr = np.stack([out[k].cpu().numpy() for k in audio._HARMONIC_FRAME], axis=-1)
    ct = np.stack([out["n_harmonics"].cpu().numpy(), out["flags"].cpu().numpy()], axis=-1)
    hm = np.stack([out["harmonic_hz"].cpu().numpy(), out["harmonic_db"].cpu().numpy()], axis=-1)
    check((fr, ct, hm), r64, rep, g, "audio.harmonics 6000 / 4100 / 2600 samples at 22050 Hz")
    given = audio.harmonics(xd, lengths=lens, period=period, formants=fm)
    assert all(torch.equal(out[k], given[k]) for k in out), "the periods and formants given are the ones found"
    nofm = audio.harmonics(xd, lengths=lens, formants=False)
    assert torch.equal(nofm["h1_h2_db"], out["h1_h2_db"]) and torch.equal(nofm["flags"], out["flags"] & 1) and not nofm["h1_a3_db"].any()
    fl = [R.frames(n, 256) for n in lens]
    voiced = period > 0
    st = audio.harmonic_statistics(out, voiced, lengths=fl, fm=fm)
    v = voiced.cpu().numpy() & (np.arange(F)[None, :] < np.array(fl)[:, None])
    assert st["frames"].cpu().tolist() == v.sum(axis=1).tolist() and v[0].sum() > 3
    bw = fm["bandwidth"].cpu().numpy()
    for name, i, bit, col in (("h1_h2_db", 0, 1, None), ("h1_a3_db", 1, 16, 2), ("f1_rel_db", 2, 2, 0), ("f2_rel_db", 3, 4, 1), ("f3_rel_db", 4, 8, 2)):
        for b in range(3):
            sel = v[b] & ((ct[b, :, 1] & bit) != 0) & (True if col is None else bw[b, :, col] <= 700.0)
            got = float(st[name][b])
            assert int(st["used"][name][b]) == sel.sum()
            assert (np.isnan(got) and not sel.any()) or abs(got - fr[b, :, i][sel].mean()) <= 1e-12 * max(1.0, abs(fr[b, :, i][sel].mean())), (name, b)
    one = audio.harmonics(xd[0, :lens[0]])
    assert one["h1_h2_db"].shape == (1, fl[0]) and torch.equal(one["flags"][0], out["flags"][0, :fl[0]]) and torch.equal(one["h1_db"][0], out["h1_db"][0, :fl[0]]), \
        "a 1-D input is the same row"
    print(f"harmonics, vowel rows: {[{k: round(float(st[k][b]), 3) for k in audio.HARMONIC_FIGURES} for b in range(3)]}")


def test_a_synthetic_vowel_of_known_h1_h2():
    """A 147 Hz harmonic complex with formant-shaped amplitudes: H1-H2 = 20 log10(a_1 / a_2) within the host test's gate (twice the restatement's
    measured closed-form error, tests/test_harmonics_host.py), at the device's own YIN periods."""
    CLOSED_GATE_H1H2 = R.CLOSED_GATE_H1H2
    for tilt in (0.0, 1.0):
        x, a = vowel(8000, 147.0, seed=5, tilt_db=tilt)
        out = audio.harmonics(torch.from_numpy(x).to(DEV), formants=False)
        nf = out["h1_h2_db"].shape[1]
        inner = slice(2, nf - 3)
        got = out["h1_h2_db"][0, inner].cpu().numpy()
        want = 20 * np.log10(a[0] / a[1])
        print(f"harmonics vowel, tilt {tilt}: H1-H2 {want:.3f} dB, measured {got.min():.3f} .. {got.max():.3f} dB (gate {CLOSED_GATE_H1H2} dB)")
        assert (out["flags"][0, inner].cpu().numpy() & 1).all() and np.abs(got - want).max() <= CLOSED_GATE_H1H2
        assert np.abs(out["h1_hz"][0, inner].cpu().numpy() - 147.0).max() < 1.0


# ---- 5. the CLI ---------------------------------------------------------------------------------------------------------------------------------------------
def _wavs(tmp_path):
    from emojivoice_amd import cli

    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    sig = [vowel(16000, 147.0, seed=20)[0], vowel(19000, 180.0, seed=21, tilt_db=1.0)[0],
           (0.01 * np.random.default_rng(22).standard_normal(3000)).astype(np.float32)]      # (noise alone: no voiced frame)
    for name, y in zip(names, sig):
        cli.write_wav_pcm16(tmp_path / name, y, R.FS)
    return cli, names


HARM_KEYS = set(audio.HARMONIC_FIGURES) | {"harmonic_frames"}


def test_voice_report_with_harmonics(tmp_path):
    cli, names = _wavs(tmp_path)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{tmp_path / name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    plain = cli.cli(["--voice_report", str(flist), "--batch_size", "2"])
    rep = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--harmonics"])
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert HARM_KEYS == {"h1_h2_db", "h1_a3_db", "f1_rel_db", "f2_rel_db", "f3_rel_db", "harmonic_frames"}
    assert [set(f_) - HARM_KEYS for f_ in saved["files"]] == [set(f_) for f_ in plain["files"]] and not HARM_KEYS & set(plain["files"][0])
    assert set(saved["overall"]) - HARM_KEYS == set(plain["overall"]) and not HARM_KEYS & set(plain["overall"])
    assert all(HARM_KEYS <= set(f_) for f_ in saved["files"]) and HARM_KEYS <= set(saved["overall"]) and HARM_KEYS <= set(saved["speakers"]["7"])
    a, b, c = saved["files"]
    print(f"\nharmonics --voice_report --harmonics: {[[f_[k] for k in ('harmonic_frames',) + audio.HARMONIC_FIGURES] for f_ in saved['files']]}")
    assert a["harmonic_frames"] > 5 and b["harmonic_frames"] > 5 and c["harmonic_frames"] == 0 and all(c[k] is None for k in audio.HARMONIC_FIGURES)
    assert all(isinstance(f_["h1_h2_db"], float) and np.isfinite(f_["h1_h2_db"]) for f_ in (a, b))
    assert b["h1_h2_db"] > a["h1_h2_db"] - 3.0 and -30.0 < a["h1_h2_db"] < 30.0
    s7 = saved["speakers"]["7"]
    assert s7["harmonic_frames"] == a["harmonic_frames"] + b["harmonic_frames"] == saved["overall"]["harmonic_frames"]
    lo, hi = min(a["h1_h2_db"], b["h1_h2_db"]), max(a["h1_h2_db"], b["h1_h2_db"])
    assert lo - 1e-9 <= s7["h1_h2_db"] <= hi + 1e-9 and saved["overall"]["h1_h2_db"] == s7["h1_h2_db"] and saved["speakers"]["12"]["h1_h2_db"] is None
    both = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--harmonics", "--formants"])
    assert all(both["files"][i][k] == saved["files"][i][k] for i in range(3) for k in HARM_KEYS), "with --formants the same figures"


def test_evaluate_pairs_with_harmonics(tmp_path):
    cli, names = _wavs(tmp_path)
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(f"{tmp_path / 'a.wav'}|{tmp_path / 'b.wav'}|7\n{tmp_path / 'b.wav'}|{tmp_path / 'a.wav'}|7\n{tmp_path / 'a.wav'}|{tmp_path / 'c.wav'}|12\n",
                     encoding="utf-8")
    plain = cli.cli(["--evaluate_pairs", str(pairs)])
    rep = cli.cli(["--evaluate_pairs", str(pairs), "--harmonics"])
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
    k = "h1_h2_db"
    assert abs(p0["harmonics"]["delta"][k] - (p0["harmonics"]["synthesised"][k] - p0["harmonics"]["recorded"][k])) < 1e-9
    assert abs(p0["harmonics"]["delta"][k] + p1["harmonics"]["delta"][k]) < 1e-9, "the swapped pair has the opposite deltas"
    assert p2["harmonics"]["synthesised"][k] is None and p2["harmonics"]["delta"][k] is None and isinstance(p2["harmonics"]["recorded"][k], float)
    s7 = saved["speakers"]["7"]["harmonics"][k]
    assert set(s7) == {"mean_delta", "mean_abs_delta"} and abs(s7["mean_delta"]) < 1e-9 and abs(s7["mean_abs_delta"] - abs(p0["harmonics"]["delta"][k])) < 1e-9
    assert saved["speakers"]["12"]["harmonics"][k] == {"mean_delta": None, "mean_abs_delta": None}
    assert abs(saved["overall"]["harmonics"][k]["mean_abs_delta"] - s7["mean_abs_delta"]) < 1e-9
