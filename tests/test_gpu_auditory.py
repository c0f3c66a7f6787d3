"""ev_load_auditory / ev_auditory on the MI355X, through the C ABI, and what stands on them (audio.auditory, audio.auditory_statistics,
audio.voice_functionals(au=...), --voice_report --auditory, --evaluate_pairs --auditory).

Yardstick: tests/auditory_ref.py, the numpy float64 restatement of the definition in include/emojivoice.h (two matrix products with the same
tables).  The device sums in the matrix instruction's own order, so it differs from the restatement by float64 rounding.  The rule of every
comparison (``check``):
  * first, a condition on the INPUT, not on the device: the float64 and the longdouble restatements agree within 1e-11 max(|ref|, 1) on every
    entry (at worst 3.9e-13, the MFCCs of 26 bands and 16 cepstra at 64 / 10 / 24; 2.2e-13 at 64 / 64 / 64 among the six geometries), so no frame is
    left out of the comparison;
  * d_flags EQUAL;
  * every entry of d_frame, d_mfcc and d_bands within 1e-9 max(|ref|, 1): the project's float64 margin (tests/test_gpu_stoi.py,
    tests/test_gpu_voice_quality.py);
  * exact zeros where the definition says zeros.
Observed on the MI355X: d_mfcc 6.2e-14 (64 bands at 64 / 10 / 24), d_frame 2.3e-15 (the power at 1024 / 256 / 1024) and d_bands 4.1e-15 at worst over
all cases, every flag equal.  Every case prints its worst figures, DESIGN section 3.24 records them; the gate stays at 1e-9.  Every raw call writes into buffers with sentinel
margins (tests/analysis_gpu.py); 50.0 sits behind every row's length.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import auditory_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

SMALL = R.GEOMETRIES[0]                  # 64 / 10 / 24: NB = 33, 6 bands, 4 cepstra
BIG = R.GEOMETRIES[3]
NAMES = ("frame", "mfcc", "flags", "bands")
_REF = {}


def ref_of(key, x, lens, g, t):
    """The restatements' results (float64, longdouble), computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: (R.batch(x, lens, g, t), R.batch(x, lens, g, t, dtype=np.longdouble)))


def load(eng, g, t=None, null=(), **kw):
    """ev_load_auditory with the geometry's tables ``t``; ``kw`` overrides an argument, ``null`` names tables passed as NULL."""
    t = R.tables(g) if t is None else t
    a = dict(W=g.W, H=g.H, nfft=g.nfft, n_mel=g.n_mel, n_ceps=g.n_ceps, k_lo=t["k_lo"], k_hi=t["k_hi"], compress=t["compress"])
    a.update({k: v for k, v in kw.items() if k in a})
    arr = {}
    for name in ("window", "twiddle", "mel_w", "eq", "dct"):
        default = R.hann(a["W"]) if name == "window" else R.twiddle(a["nfft"]) if name == "twiddle" else t[name]
        arr[name] = np.ascontiguousarray(kw.get(name, default), dtype=np.float64)
    p = lambda name: None if name in null else arr[name].ctypes.data
    return eng.lib.ev_load_auditory(eng.h, p("window"), p("twiddle"), a["W"], a["H"], a["nfft"], p("mel_w"), a["n_mel"], p("eq"), p("dct"), a["n_ceps"],
                                    a["k_lo"], a["k_hi"], float(a["compress"]))


def raw(eng, g, x, lens, floor=R.POWER_FLOOR, B=None, L=None, null=()):
    """ev_auditory into guarded buffers: (rc, {"frame" (B, NF, 4), "mfcc" (B, NF, n_ceps), "flags" (B, NF), "bands" (B, NF, n_mel)}) on the host; an
    output named in ``null`` is passed as NULL and comes back None.  ``B`` / ``L`` override the shape passed to the library."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    NF = R.frames(Lx, g.H)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"frame": ((Bx, NF, 4), torch.float64), "mfcc": ((Bx, NF, g.n_ceps), torch.float64), "flags": ((Bx, NF), torch.int32),
                     "bands": ((Bx, NF, g.n_mel), torch.float64)}, null)
    rc = eng.lib.ev_auditory(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, float(floor),
                             out.ptr("frame"), out.ptr("mfcc"), out.ptr("flags"), out.ptr("bands"), _stream_ptr())
    return rc, out.collect(rc)


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    r64, r80 = ref
    e_in = {k: R.err(r64[k], r80[k]) for k in ("frame", "mfcc", "bands")}
    assert max(e_in.values()) <= R.INPUT_TOL and np.array_equal(r64["flags"], r80["flags"]), \
        f"{what}: the float64 and longdouble restatements differ by {e_in}, over {R.INPUT_TOL:g}: the input is ill-conditioned"
    per = [R.err(dev["frame"][..., i], r64["frame"][..., i]) for i in range(4)]
    e_m = R.err(dev["mfcc"], r64["mfcc"])
    e_b = R.err(dev["bands"], r64["bands"]) if dev["bands"] is not None else 0.0
    live = (r64["flags"] & 1) != 0
    print(f"\nauditory {what}: d_frame err per figure (loudness, flux, power, log-energy) {[f'{e:.1e}' for e in per]}  d_mfcc err {e_m:.3e}  d_bands err "
          f"{e_b:.3e} (gate {R.TOL:g})  restatement float64 against longdouble {max(e_in.values()):.3e}  flags differing "
          f"{int((dev['flags'] != r64['flags']).sum())}  live frames {int(live.sum())} of {live.size}")
    assert np.array_equal(dev["flags"], r64["flags"]), f"{what}: d_flags"
    assert max(per) <= R.TOL, f"{what}: d_frame"
    assert e_m <= R.TOL, f"{what}: d_mfcc"
    assert e_b <= R.TOL, f"{what}: d_bands"
    for k in ("frame", "mfcc", "bands"):
        assert dev[k] is None or not dev[k][r64[k] == 0].any(), f"{what}: exact zeros of d_{k} where the definition says zeros"
    assert not dev["frame"][~live][:, [0, 3]].any() and not dev["mfcc"][~live].any(), f"{what}: a frame that is not live has no loudness, log-energy or MFCC"


def engine_with(g, t=None):
    return A.engine_with(load, g, t)


@pytest.fixture(scope="module")
def engines():
    yield from A.engines_on_demand(engine_with)


@pytest.fixture(scope="module")
def small(engines):
    return engines(SMALL)


def run(eng, g, x, lens, key, what, t=None, **kw):
    rc, dev = raw(eng, g, x, lens, **kw)
    assert rc == 0, err_of(eng)
    ref = ref_of(key, x, lens, g, R.tables(g) if t is None else t)
    check(dev, ref, what)
    return dev, ref


# ---- 1. the geometries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GEOMETRIES, ids=R.IDS)
def test_geometry_against_the_restatement(engines, g):
    x, lens = R.rows_for(g)
    nfs = [R.frames(n, g.H) for n in lens]
    assert [n % R.TILE for n in nfs] == [14, 0, 1] and max(nfs) >= 31, "one short of, on and one over a tile seam; a flux across two seams"
    dev, _ = run(engines(g), g, x, lens, ("rows", g), f"{tuple(g)} lens {lens}")
    for b in range(3):
        assert all(not dev[k][b, nfs[b]:].any() for k in NAMES), "zeros past the row's own frames"
        assert (dev["flags"][b, :nfs[b]] & 1).sum() > nfs[b] // 2, "most frames are live"
        assert dev["flags"][b, 0] & 2 == 0 and (dev["flags"][b, 1:nfs[b]] & 2).all() and dev["frame"][b, 0, 1] == 0, "frame 0 has no predecessor"
        for f in range(R.TILE, nfs[b], R.TILE):                         # the first frame of every later tile takes its flux from the carried row
            assert dev["frame"][b, f, 1] > 0 or not (dev["flags"][b, f - 1:f + 1] & 1).any()


@pytest.mark.parametrize("g", R.EDGE_GEOMETRIES, ids=R.EDGE_IDS)
def test_edge_geometry_against_the_restatement(engines, g):
    """The same check where the skew walk and the K loops take their rare paths: H < 4, a skew of 3, W / 4 = 3 and W / 4 = 4 (one whole round), one
    bin tile (waves 1-3 hand over their identities), three phase-2 steps, 3 bands of one partial band tile, 2 cepstra."""
    test_geometry_against_the_restatement(engines, g)


@pytest.mark.parametrize("n_mel,n_ceps", [(1, 1), (6, 16), (16, 4), (17, 1), (26, 16), (64, 4)])
def test_band_tiles_and_cepstra(n_mel, n_ceps):
    """One partial band tile, exactly one, one and a bit, two, four (one per wave); 1, 4 and 16 cepstra.  With 64 bands over 33 bins most filters
    hold no bin: E = 0 meets the floor there."""
    g = SMALL._replace(n_mel=n_mel, n_ceps=n_ceps)
    x, lens = R.rows_for(g)
    e = engine_with(g)
    try:
        run(e, g, x, lens, ("rows", g), f"n_mel {n_mel} n_ceps {n_ceps}")
    finally:
        e.close()


@pytest.mark.parametrize("flux,zero", [((5, 6), None), ((0, 33), 2), ((3, 20), None)], ids=["one-bin", "every-bin-zero-column", "17-bins"])
def test_flux_ranges_and_a_zero_column(flux, zero):
    g = SMALL
    t = R.tables(g, flux=flux, zero_column=zero)
    x, lens = R.rows_for(g)
    e = engine_with(g, t)
    try:
        dev, (r64, _) = run(e, g, x, lens, ("flux", flux, zero), f"flux bins {flux} zeroed band {zero}", t=t)
        if zero is not None:
            assert not dev["bands"][..., zero].any() and (r64["bands"][..., zero] == 0).all()
            live = (dev["flags"] & 1) != 0
            assert (dev["bands"][live][:, [0, 1, 3]] > 0).all(), "the other bands are not empty"
        plain = ref_of(("rows", g), x, lens, g, R.tables(g))[0]
        if flux != (0, 33):
            assert R.err(plain["frame"][..., 1], r64["frame"][..., 1]) > 1e-3, "the range shows in the flux"
    finally:
        e.close()


# ---- 2. invariance ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", (SMALL, BIG), ids=(R.IDS[0], R.IDS[3]))
def test_row_alone_in_a_batch_as_a_prefix_and_without_bands_give_the_same_bits(engines, g):
    eng = engines(g)
    x, lens = R.rows_for(g, seed=40)
    n = lens[0]
    c = x[0, :n].copy()
    rc, alone = raw(eng, g, c[None], None)
    assert rc == 0, err_of(eng)
    rc, again = raw(eng, g, c[None], None)
    assert rc == 0 and all(np.array_equal(alone[k], again[k]) for k in NAMES), "two calls"
    rc, nb = raw(eng, g, c[None], None, null=("bands",))
    assert rc == 0 and nb["bands"] is None and all(np.array_equal(alone[k], nb[k]) for k in NAMES[:3]), "d_bands = NULL"
    xb, _, lb = R.padded([(x[2, :lens[2]],) * 2, (c, c), (x[1, :lens[1]],) * 2])
    rc, batch = raw(eng, g, xb, lb)
    assert rc == 0
    xp, _, lp = R.padded([(x[1, :lens[1]],) * 2, (c, c)], L=n + 1235)
    xp[1, n:] = -7.5e3                                                   # other garbage than in the batch of three
    rc, prefix = raw(eng, g, xp, lp)
    assert rc == 0
    nf = R.frames(n, g.H)
    assert (alone["flags"][0] & 1).any()
    for name, other in (("inside a batch", batch), ("the prefix of a padded row", prefix)):
        for k in NAMES:
            assert np.array_equal(alone[k][0, :nf], other[k][1, :nf]) and not other[k][1, nf:].any(), f"d_{k}: alone against {name}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 6):
            eng.set_arithmetic(setting)
            rc, got = raw(eng, g, xb, lb)
            assert rc == 0 and all(np.array_equal(got[k], batch[k]) for k in NAMES), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


def test_graph_replay_and_the_engine_method_allocate_nothing():
    g = SMALL
    x, lens = R.rows_for(g)
    t = R.tables(g)
    e = Engine(0)
    try:
        n_before = e.alloc_count()
        e.load_auditory(t["window"], t["twiddle"], g.H, g.nfft, t["mel_w"], t["eq"], t["dct"], t["k_lo"], t["k_hi"], t["compress"])
        assert e.alloc_count() == n_before + 1, "one device block, counted once"
        xd, ld = torch.tensor(np.array(x)).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
        n0 = e.alloc_count()
        ref = e.auditory(xd, ld, R.POWER_FLOOR, want_bands=True)
        torch.cuda.synchronize()
        assert e.alloc_count() == n0 and e.auditory(xd, ld, R.POWER_FLOOR)["bands"] is None
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            e.auditory(xd, ld, R.POWER_FLOOR, want_bands=True)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = e.auditory(xd, ld, R.POWER_FLOOR, want_bands=True)
            for o in out.values():
                o.fill_(-5)
            graph.replay()
            torch.cuda.synchronize()
        for k in NAMES:
            assert torch.equal(out[k], ref[k]), f"{k}: the replay equals the eager call"
        dev = {k: v.cpu().numpy() for k, v in out.items()}
        check(dev, ref_of(("rows", g), x, lens, g, t), "a replay from a captured graph")
        assert e.alloc_count() == n0
    finally:
        e.close()


# ---- 3. degenerate inputs -----------------------------------------------------------------------------------------------------------------------
def test_silent_frames_and_bad_rows(small):
    g = SMALL
    x, lens = R.rows_for(g)
    L = x.shape[1]
    hole = x[0].copy()
    hole[700:1500] = 0.0                                                 # digital silence in the middle of a row
    x = np.concatenate([x, np.zeros((1, L), np.float32), hole[None], x[:1], x[:1], x[:1]])
    lens = lens + [2000, lens[0], 0, -1, L + 1]
    dev, _ = run(small, g, x, lens, "degenerate", "a zero row, a row with a silent middle and bad rows beside good ones")
    nfz = R.frames(2000, g.H)
    assert all(not dev[k][3].any() for k in ("frame", "mfcc", "bands")), "a zero row: every frame is silent, power and flux 0"
    assert dev["flags"][3, :nfz].tolist() == [0] + [2] * (nfz - 1) and not dev["flags"][3, nfz:].any()
    first = (700 + g.W // 2 - g.H // 2) // g.H + 1                      # the first frame whose window lies inside the hole
    flags, frame = dev["flags"][4], dev["frame"][4]
    assert flags[first - 1] == 3 and flags[first] == 2 and frame[first, 1] > 0 and frame[first, 2] == 0, "the first silent frame: a flux, no live bit"
    assert frame[first + 1, 1] == 0 and flags[first + 1] == 2 and not dev["mfcc"][4, first].any() and not dev["bands"][4, first].any()
    last = (1500 - g.W // 2 - g.H // 2) // g.H
    assert (flags[first:last] == 2).all() and flags[last + 3] == 3 and (flags[:first] == np.array([1] + [3] * (first - 1))).all()
    for b in (5, 6, 7):
        assert all(not dev[k][b].any() for k in NAMES), "len 0, len < 0, len > L: rows of zeros"


def test_a_row_of_one_sample_has_one_frame(small):
    g = SMALL
    x, lens = R.rows_for(g)
    for i, (xs, ls) in enumerate(((x[:2], [1, lens[1]]), (x[:2, :1], None))):   # a row of 1 sample beside a good row; L = 1: NF = 1
        dev, _ = run(small, g, xs, ls, ("one", i), f"a row of one sample ({'L = 1' if ls is None else 'beside a good row'})")
        assert dev["flags"][0, 0] == 1 and not dev["flags"][0, 1:].any() and dev["frame"][0, 0, 1] == 0 and dev["frame"][0, 0, 2] > 0
        assert not dev["frame"][0, 1:].any() and not dev["mfcc"][0, 1:].any()
    assert dev["frame"].shape == (2, 1, 4)


def test_null_d_len_is_every_row_whole(small):
    g = SMALL
    x, _ = R.rows_for(g)
    xs = np.ascontiguousarray(x[:2, :1503])
    dev, _ = run(small, g, xs, None, "null-len", "d_len NULL: L = 1503")
    rc, same = raw(small, g, xs, [1503, 1503])
    assert rc == 0 and all(np.array_equal(dev[k], same[k]) for k in NAMES)


# ---- 4. limits and loading ----------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
BAD_CALL = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)), ("power_floor", dict(floor=0.0)), ("power_floor", dict(floor=-1e-7)),
    ("power_floor", dict(floor=INF)), ("power_floor", dict(floor=NAN)),
    ("d_frame", dict(null=("frame",))), ("d_mfcc", dict(null=("mfcc",))), ("d_flags", dict(null=("flags",))), ("d_x", dict(null=("x",))),
]


@pytest.mark.parametrize("word,kw", BAD_CALL, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_of_ev_auditory_fails_with_a_message_naming_it(small, word, kw):
    z = np.zeros((2, 256), np.float32)
    rc, _ = raw(small, SMALL, z, None, **kw)                             # (a failed call writes nothing: raw checks that)
    msg = err_of(small)
    assert rc != 0 and "ev_auditory" in msg and word in msg, msg


def test_more_frames_than_a_tile_index_holds_fails(small):
    z = np.zeros((1, 256), np.float32)
    e = engine_with(SMALL._replace(H=1, W=24))
    try:
        rc, _ = raw(e, SMALL._replace(H=1), z, None, L=0x7ffffff0)
        msg = err_of(e)
        assert rc != 0 and "ev_auditory" in msg and "L=" in msg and "int32" in msg, msg
    finally:
        e.close()


def _with(a, i, v):
    a = np.array(a, copy=True)
    a.reshape(-1)[i] = v
    return a


_T = R.tables(SMALL)
BAD_LOAD = [
    ("nfft=", dict(nfft=14, W=12)), ("nfft=", dict(nfft=1026, W=1024)), ("nfft=", dict(nfft=65, W=25)), ("W=", dict(W=2)), ("W=", dict(W=68)), ("W=", dict(W=26)),
    ("nfft - W", dict(nfft=66, W=25)), ("H=", dict(H=0)), ("H=", dict(H=513)),
    ("n_mel=", dict(n_mel=0)), ("n_mel=", dict(n_mel=65)), ("n_ceps=", dict(n_ceps=0)), ("n_ceps=", dict(n_ceps=17)),
    ("k_lo=", dict(k_lo=-1)), ("k_lo=", dict(k_lo=7, k_hi=7)), ("k_hi=", dict(k_hi=34)),
    ("compress=", dict(compress=0.0)), ("compress=", dict(compress=1.5)), ("compress=", dict(compress=NAN)),
    ("window[5]", dict(window=_with(R.hann(24), 5, NAN))), ("twiddle[15]", dict(twiddle=_with(R.twiddle(64), 15, INF))),
    ("mel_w[40]", dict(mel_w=_with(_T["mel_w"], 40, NAN))), ("mel_w[41]", dict(mel_w=_with(_T["mel_w"], 41, -0.25))),
    ("eq[3]", dict(eq=_with(_T["eq"], 3, INF))), ("eq[2]", dict(eq=_with(_T["eq"], 2, 0.0))), ("eq[1]", dict(eq=_with(_T["eq"], 1, -1.0))),
    ("dct[7]", dict(dct=_with(_T["dct"], 7, -INF))),
    ("non-null", dict(null=("window",))), ("non-null", dict(null=("twiddle",))), ("non-null", dict(null=("mel_w",))), ("non-null", dict(null=("eq",))),
    ("non-null", dict(null=("dct",))),
]


@pytest.mark.parametrize("word,kw", BAD_LOAD, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_LOAD)])
def test_each_limit_of_ev_load_auditory_fails_with_a_message_naming_it(small, word, kw):
    kw = dict(kw)
    null = kw.pop("null", ())
    if "n_mel" in kw or "n_ceps" in kw:                                   # (tables as large as the counts ask for)
        nm, nc = max(kw.get("n_mel", SMALL.n_mel), 1), max(kw.get("n_ceps", SMALL.n_ceps), 1)
        kw.update(mel_w=np.ones((33, nm)), eq=np.ones(nm), dct=np.ones((nm, nc)))
    n0 = small.alloc_count()
    rc = load(small, SMALL, null=null, **kw)
    msg = err_of(small)
    assert rc != 0 and "ev_load_auditory" in msg and word in msg, msg
    assert small.alloc_count() == n0
    x, lens = R.rows_for(SMALL)                                           # the tables loaded before are still the ones in use
    r64 = ref_of(("rows", SMALL), x, lens, SMALL, R.tables(SMALL))[0]
    rc, dev = raw(small, SMALL, x[:1], lens[:1])
    nf = R.frames(lens[0], SMALL.H)
    assert rc == 0 and np.array_equal(dev["flags"][0, :nf], r64["flags"][0, :nf]) and R.err(dev["frame"][0, :nf], r64["frame"][0, :nf]) <= R.TOL


def test_the_largest_geometry_the_limits_admit_fits_the_lds_budget():
    """ev_load_auditory computes its LDS need and refuses more than 160 KiB by name; under today's limits (nfft <= 1024, H <= 512, 64 bands) the
    largest need is 117 376 bytes, so the load succeeds."""
    e = Engine(0)
    try:
        g = R.Geometry(1024, 512, 1024, R.FS, 64, 4, 20.0, 8000.0)
        t = {"mel_w": np.ones((513, 64)), "eq": np.ones(64), "dct": np.ones((64, 4)), "k_lo": 0, "k_hi": 513, "compress": 0.33}
        need = 16 * 514 * 8 + 32 * 65 * 8 + (15 * 512 + 1024 + 2 * ((15 * 512 + 1023) // 512)) * 4
        assert need == 117376 and need <= 160 * 1024
        n0 = e.alloc_count()
        assert load(e, g, t) == 0 and e.alloc_count() == n0 + 1, err_of(e)
        rc, dev = raw(e, g, np.full((1, 2000), 0.25, np.float32), None)
        assert rc == 0 and (dev["flags"][0] & 1).all() and (dev["frame"][0, :, 0] > 0).all(), err_of(e)
    finally:
        e.close()


def test_a_call_before_a_load_fails_loading_again_replaces_the_tables_and_calls_allocate_nothing():
    e = Engine(0)
    try:
        z = np.zeros((1, 256), np.float32)
        rc, _ = raw(e, SMALL, z, None)
        assert rc != 0 and "ev_load_auditory" in err_of(e)
        n0 = e.alloc_count()
        assert load(e, R.GEOMETRIES[2]) == 0, err_of(e)
        assert e.alloc_count() == n0 + 1, "the tables are one device block that counts in ev_alloc_count"
        assert load(e, SMALL) == 0 and e.alloc_count() == n0 + 2
        x, lens = R.rows_for(SMALL)
        rc, dev = raw(e, SMALL, x, lens)
        assert rc == 0, err_of(e)
        check(dev, ref_of(("rows", SMALL), x, lens, SMALL, R.tables(SMALL)), "after loading twice")
        n1 = e.alloc_count()
        assert n1 == n0 + 2, "a call allocates nothing"
        rc, dev2 = raw(e, SMALL, x, lens)
        torch.cuda.synchronize()
        assert rc == 0 and e.alloc_count() == n1 and all(np.array_equal(dev[k], dev2[k]) for k in NAMES), "a second call at the same shape allocates nothing"
    finally:
        e.close()


# ---- 5. audio.auditory ------------------------------------------------------------------------------------------------------------------------------
def test_audio_auditory_on_three_ragged_rows():
    lens = [4000, 2600, 700]
    sig = [R.speech_like(n, seed=30 + i, fs=R.FS) for i, n in enumerate(lens)]
    x, _, _ = R.padded([(s, s) for s in sig])
    xd = torch.from_numpy(x).to(DEV)
    out = audio.auditory(xd, lengths=lens)
    eng = audio._auditory_engine(xd.device, 22050, 1024, 256, 26, 20.0, 8000.0, 4, 22.0, (0.0, None))
    n0 = eng.alloc_count()
    out2 = audio.auditory(xd, lengths=lens)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0 and eng is audio._auditory_engine(xd.device, 22050, 1024, 256, 26, 20.0, 8000.0, 4, 22.0, (0.0, None)), "one cached engine"
    t = audio.auditory_tables(22050, 1024)
    tabs = dict(R.tables(BIG), mel_w=t["mel_w"], eq=t["eq"], dct=t["dct"])      # audio's own tables under the restatement
    ref = ref_of("audio", x, lens, BIG, tabs)
    F = R.frames(x.shape[1], 256)
    for k in R.FIGURES:
        assert out[k].dtype == torch.float64 and out[k].shape == (3, F) and torch.equal(out[k], out2[k]), k
    assert out["mfcc"].shape == (3, F, 4) and out["live"].dtype == torch.bool and out["has_previous"].dtype == torch.bool
    flags = out["live"].to(torch.int32) + 2 * out["has_previous"].to(torch.int32)
    dev = {"frame": np.stack([out[k].cpu().numpy() for k in R.FIGURES], axis=-1), "mfcc": out["mfcc"].cpu().numpy(), "flags": flags.cpu().numpy(), "bands": None}
    check(dev, ref, "audio.auditory 4000 / 2600 / 700 samples")
    one = audio.auditory(xd[0, :lens[0]])
    nf = R.frames(lens[0], 256)
    assert one["loudness"].shape == (1, nf) and torch.equal(one["loudness"][0], out["loudness"][0, :nf]), "a 1-D input is the same row"


def test_a_steady_tone_and_the_same_tone_at_twice_the_amplitude():
    """147 Hz at 22050 Hz is a period of exactly 150 samples.  At a hop of one period every frame whose window lies inside the row sees the same
    samples, so a steady tone has no flux and a constant loudness.  (At the default hop of 256 the DEFINITION gives neither: the harmonics, 6.8
    bins apart, leak into each other under the Hann window and the interference moves with the frame's phase; the numpy restatement has a flux of
    1.6e-2 of the mean magnitude and a loudness spread of 4e-5 there.)  The bands stop at 4 kHz, inside the tone's 29 harmonics: a band that
    holds leakage only sits on the floor, which no gain moves, and then a gain moves more than c0."""
    n, H = 12000, 150
    tone = R.harmonic_tone(n)
    x = torch.from_numpy(np.stack([tone, 2.0 * tone])).to(DEV)
    au = audio.auditory(x, hop_length=H, n_mels=20, fmax=4000.0)
    g = R.Geometry(1024, H, 1024, R.FS, 20, 4, 20.0, 4000.0)
    inner = slice(4, (n - 512 - H // 2) // H)                           # the frames whose windows lie inside the row
    mean_mag = torch.from_numpy(np.sqrt(R.spectrum(tone, g, R.tables(g))).mean(axis=1)).to(DEV)[inner]
    flux, loud, mfcc = au["spectral_flux"][:, inner], au["loudness"][:, inner], au["mfcc"][:, inner]
    print(f"\nauditory, 147 Hz tone at a hop of one period: flux / mean magnitude {float((flux[0] / mean_mag).max()):.3e} at worst, loudness "
          f"{float(loud[0].mean()):.6f} (spread {float((loud[0] - loud[0].mean()).abs().max() / loud[0].mean()):.3e}), twice the amplitude: loudness ratio "
          f"{float((loud[1] / loud[0]).mean()):.12f} against 4^0.33 = {4 ** 0.33:.12f}, MFCC 1-4 {[round(float(v), 4) for v in mfcc[0].mean(dim=0)]}, "
          f"moved by {float((mfcc[1] - mfcc[0]).abs().max()):.3e} at most")
    assert inner.stop - inner.start > 60 and bool(au["live"][:, inner].all()) and bool((mean_mag > 0.1).all())
    assert bool((flux[0] < 1e-3 * mean_mag).all()), "a steady tone: the spectrum does not move"
    assert bool(((loud[0] - loud[0].mean()).abs() <= 1e-6 * loud[0].mean()).all()), "a steady tone: constant loudness"
    assert bool(((loud[1] / loud[0] - 4.0 ** 0.33).abs() <= 1e-9 * 4.0 ** 0.33).all()), "twice the amplitude: 4^0.33 times the loudness"
    assert bool(((mfcc[1] - mfcc[0]).abs() <= 1e-9 * mfcc[0].abs().clamp(min=1.0)).all()), "a gain moves c0 only"
    assert bool((au["spectral_flux"][0, 1:3] > 1e-3 * mean_mag[0]).all()), "the onset, while the window fills, is a flux event"


# ---- 6. the statistics and the functionals -------------------------------------------------------------------------------------------------------
def test_statistics_and_the_functionals_of_the_auditory_contours():
    lens = [9000, 6100]
    sig = [R.speech_like(n, seed=50 + i, fs=R.FS) for i, n in enumerate(lens)]
    x, _, _ = R.padded([(s, s) for s in sig])
    xd = torch.from_numpy(x).to(DEV)
    pitch = audio.pitch_yin(xd, lengths=lens)
    vq = audio.voice_quality(xd, lengths=lens)
    au = audio.auditory(xd, lengths=lens)
    fl = [R.frames(v, 256) for v in lens]
    st = audio.auditory_statistics(au, pitch["voiced"], fl)
    inside = np.arange(au["live"].shape[1])[None, :] < np.array(fl)[:, None]
    live, moved, voiced = au["live"].cpu().numpy() & inside, au["has_previous"].cpu().numpy() & inside, pitch["voiced"].cpu().numpy()
    assert st["frames"].cpu().tolist() == live.sum(axis=1).tolist() and live.sum() > 40 and (moved & voiced).sum() > 5
    loud, flux, power = (au[k].cpu().numpy() for k in ("loudness", "spectral_flux", "power"))
    for b in range(2):
        assert abs(float(st["loudness"][b]) - loud[b][live[b]].mean()) <= 1e-12 * loud[b][live[b]].mean()
        assert abs(float(st["spectral_flux_voiced"][b]) - flux[b][moved[b] & voiced[b]].mean()) <= 1e-12 * flux[b][moved[b] & voiced[b]].mean()
        want = 10 * np.log10(power[b][inside[b]].mean())
        assert abs(float(st["equivalent_level_db"][b]) - want) <= 1e-12 * abs(want)
    plain = audio.voice_functionals(pitch, vq, fl)
    again = audio.voice_functionals(pitch, vq, fl, au=None)
    both = audio.voice_functionals(pitch, vq, fl, au=au)
    assert plain["contours"] == again["contours"] and both["contours"] == plain["contours"] + audio.AUDITORY_FIGURES[:-1]
    same = lambda a, b: a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())     # (equal, NaN where NaN)
    for c in plain["contours"] + ("segments",):
        for k, v in plain[c].items():
            assert same(v, again[c][k]), f"{c} {k}: au=None is the call without it"
            assert same(v, both[c][k]), f"{c} {k}: the contours in front do not move"
    for c in audio.AUDITORY_FIGURES[:-1]:
        m, s = both[c]["mean"], st[c]
        ok = ~torch.isnan(s)
        assert bool((torch.isnan(m) == torch.isnan(s)).all()) and bool(((m[ok] - s[ok]).abs() <= 1e-12 * s[ok].abs().clamp(min=1.0)).all()), c
        assert both[c]["valid"].cpu().tolist() == st["used"][c].cpu().tolist(), c
    assert bool((both["loudness"]["peaks_per_s"] > 0).all()), "loudness peaks per second"
    print(f"\nauditory statistics: { {k: [round(float(v), 4) for v in st[k]] for k in audio.AUDITORY_FIGURES} } loudness peaks per second "
          f"{[round(float(v), 3) for v in both['loudness']['peaks_per_s']]}")


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------------------
def _wavs(tmp_path, short):
    from emojivoice_amd import cli

    sr = 22050
    names = {"a.wav": "7", "b.wav": "7", "c.wav": "12"}
    for i, name in enumerate(names):
        cli.write_wav_pcm16(tmp_path / name, R.speech_like((16000, 19000, short)[i], seed=20 + i, fs=sr), sr)
    return cli, names


def test_voice_report_with_auditory_and_functionals(tmp_path):
    cli, names = _wavs(tmp_path, 300)
    flist = tmp_path / "filelist.txt"
    flist.write_text("".join(f"{tmp_path / name}|{spk}|text of {name}\n" for name, spk in names.items()), encoding="utf-8")
    plain = cli.cli(["--voice_report", str(flist), "--batch_size", "2"])
    rep = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--auditory"])
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    new = set(audio.AUDITORY_FIGURES) | {"auditory_frames"}
    assert [set(f_) - new for f_ in saved["files"]] == [set(f_) for f_ in plain["files"]] and all(new <= set(f_) for f_ in saved["files"])
    assert set(saved["overall"]) - new == set(plain["overall"]) and new <= set(saved["overall"]) and set(saved) == set(plain)
    assert not new & set(plain["files"][0]) and not new & set(plain["overall"]), "without the flag the key sets are the old ones"
    a, b, c = saved["files"]
    print(f"\nauditory --voice_report: {[[f_['auditory_frames']] + [f_[k] for k in audio.AUDITORY_FIGURES] for f_ in saved['files']]}")
    assert a["auditory_frames"] > 30 and all(isinstance(a[k], float) and np.isfinite(a[k]) for k in audio.AUDITORY_FIGURES)
    assert c["auditory_frames"] == 2 and c["mfcc_1_voiced"] is None and isinstance(c["loudness"], float), "300 samples: live frames, none voiced"
    s7 = saved["speakers"]["7"]
    n = a["auditory_frames"] + b["auditory_frames"]
    pooled = (a["loudness"] * a["auditory_frames"] + b["loudness"] * b["auditory_frames"]) / n
    assert s7["auditory_frames"] == n and abs(s7["loudness"] - pooled) <= 1e-9 * pooled
    level = 10 * np.log10((10 ** (a["equivalent_level_db"] / 10) * a["frames"] + 10 ** (b["equivalent_level_db"] / 10) * b["frames"]) / (a["frames"] + b["frames"]))
    assert abs(s7["equivalent_level_db"] - level) <= 1e-9 * abs(level), "the level pools over the power"
    func = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--auditory", "--functionals"])
    fa = func["files"][0]["functionals"]
    assert set(audio.AUDITORY_FIGURES[:-1]) <= set(fa) and "f0_semitones" in fa and fa["loudness"]["peaks_per_s"] > 0
    assert abs(fa["loudness"]["mean"] - a["loudness"]) <= 1e-9 * a["loudness"]
    assert set(audio.AUDITORY_FIGURES[:-1]) <= set(func["speakers"]["7"]["functionals"]) and "loudness" in func["overall"]["functionals"]
    only = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--functionals"])
    assert not set(audio.AUDITORY_FIGURES) & set(only["files"][0]["functionals"]), "--functionals without --auditory keeps its contours"


def test_evaluate_pairs_with_auditory(tmp_path):
    cli, names = _wavs(tmp_path, 600)
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(f"{tmp_path / 'a.wav'}|{tmp_path / 'b.wav'}|7\n{tmp_path / 'b.wav'}|{tmp_path / 'a.wav'}|7\n", encoding="utf-8")
    plain = cli.cli(["--evaluate_pairs", str(pairs)])
    rep = cli.cli(["--evaluate_pairs", str(pairs), "--auditory"])
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    figs = set(audio.AUDITORY_FIGURES)
    assert all("auditory" not in p for p in plain["pairs"]) and "auditory" not in plain["overall"]
    assert [set(p) - {"auditory"} for p in saved["pairs"]] == [set(p) for p in plain["pairs"]], "without the flag the key sets are the old ones"
    assert set(saved["overall"]) - {"auditory"} == set(plain["overall"]) and set(saved) == set(plain)
    p0, p1 = saved["pairs"]
    for p in saved["pairs"]:
        assert set(p["auditory"]) == {"recorded", "synthesised", "delta"} and all(set(p["auditory"][k]) == figs for k in p["auditory"])
    for k in figs:
        assert abs(p0["auditory"]["delta"][k] - (p0["auditory"]["synthesised"][k] - p0["auditory"]["recorded"][k])) < 1e-12
        assert abs(p0["auditory"]["delta"][k] + p1["auditory"]["delta"][k]) < 1e-12, "the swapped pair has the opposite deltas"
        assert set(saved["overall"]["auditory"][k]) == {"mean_delta", "mean_abs_delta"}
