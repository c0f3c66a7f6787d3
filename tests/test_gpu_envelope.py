"""ev_load_envelope / ev_envelope on the MI355X, through the C ABI.

Yardstick: tests/envelope_ref.py, the numpy float64 restatement of include/emojivoice.h's steps 1 to 7 (CheapTrick on given periods, freqt).
The rule of every comparison (``check``): d_class {class, half, kd} must be EQUAL to the restatement; d_env (the log power envelope, nepers) and
d_mcep lie within the project's 1e-9 ABSOLUTE of it.  The signals are harmonic sums with seeded noise 60 dB down, so the range of P inside a
frame is bounded and the restatement's own rounding (an FFT against the device's GEMM, pairwise against ordered sums) stays far under the gate.
Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py); inputs carry NaN behind each row's length, periods NaN past a
row's frames.

Geometries: sr 4000, nfft 128 (NB = 65: a masked last bin tile), H 32, default period 8; and one case at 22050 / 1024 / 256 with 2 rows x 40
frames.  T_max = (nfft - 3) / 3 is no float32 at either: "at T_max" is the largest float32 not above it, "just outside" the next one up.

Observed on the MI355X (printed by every case; the gate stays as it is): d_class equal throughout; the largest error of Le 1.9e-13 (the case at
22050 / 1024; 7.5e-14 at nfft 128), of the mel-cepstrum 4.9e-15.  The mutants lie 1.2 (no mean removal), 0.60 (the DC interpolation on the
corrected P), 2.3 (a cell offset by 1/2), 1.5 (the lifter without the compensation term) and 2.6 (c[0] not halved) from the device (DESIGN
section 3.29).

Times: not gated here (tools/envelope_bench.py).
"""
import numpy as np
import pytest
import torch

import analysis_gpu as A
import envelope_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import _stream_ptr

pytestmark = pytest.mark.gpu

_REF = {}
NAMES = ("env", "mcep", "class")
SMALL = (4000.0, 128, 32)                # sr, nfft, H
BIG = (22050.0, 1024, 256)
GATE = 1e-9


def tmax32(nfft):
    """The largest float32 not above T_max."""
    t = np.float32(R.t_max(nfft))
    return t if float(t) <= R.t_max(nfft) else np.nextafter(t, np.float32(0))


def load(eng, geom, n_mcep, alpha, warp=None, null=(), **over):
    sr, nfft, H = geom
    a = dict(H=H, nfft=nfft, sr=sr, default_period=0.0, q1=R.Q1, n_mcep=n_mcep)
    a.update(over)
    tw = np.ascontiguousarray(audio.stoi_twiddle(nfft) if "tw" not in over else over["tw"])
    wp = np.ascontiguousarray(audio.freq_warp_matrix(nfft // 2 + 1, n_mcep - 1, alpha) if warp is None else warp, dtype=np.float64)
    return eng.lib.ev_load_envelope(eng.h, None if "twiddle" in null else tw.ctypes.data, a["H"], a["nfft"], a["sr"], a["default_period"], a["q1"],
                                    None if "warp" in null else wp.ctypes.data, a["n_mcep"])


def raw(eng, x, lens, period, geom, n_mcep, B=None, L=None, null=(), floor=R.FLOOR):
    """ev_envelope into guarded buffers -> (rc, {"env", "mcep", "class"} on the host; None where passed as NULL)."""
    _, nfft, H = geom
    x = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    NF = -(-Lx // H)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    d_p = torch.as_tensor(np.asarray(period), dtype=torch.float32).to(DEV).contiguous()
    out = A.Guarded({"env": ((Bx, NF, nfft // 2 + 1), torch.float64), "mcep": ((Bx, NF, n_mcep), torch.float64), "class": ((Bx, NF, 3), torch.int32)},
                    tuple(n for n in null if n in NAMES))
    rc = eng.lib.ev_envelope(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(),
                             None if "period" in null else d_p.data_ptr(), Bx if B is None else B, Lx if L is None else L, floor,
                             out.ptr("env"), out.ptr("mcep"), out.ptr("class"), _stream_ptr())
    return rc, out.collect(rc)


def same_bits(a, b, names=NAMES):
    return all(np.array_equal(a[k], b[k]) for k in names)


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    e_env = float(np.abs(dev["env"] - ref["env"]).max()) if dev["env"] is not None else 0.0
    e_mc = float(np.abs(dev["mcep"] - ref["mcep"]).max())
    print(f"\nenvelope {what}: abs err Le {e_env:.3e} mcep {e_mc:.3e} (gate {GATE:g})  classes {np.bincount(dev['class'][..., 0].ravel(), minlength=4).tolist()}")
    assert np.array_equal(dev["class"], ref["class"]), f"{what}: d_class differs at {np.argwhere(dev['class'] != ref['class'])[:8].tolist()}"
    assert e_env <= GATE, f"{what}: d_env"
    assert e_mc <= GATE, f"{what}: d_mcep"


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
def row_a():
    """17 frames at H = 32 (a second tile holding one frame) and the periods that take every path: the longest window beside the shortest in
    one tile, both limits and the values just outside them, unvoiced, NaN and negative periods."""
    x = R.harmonic_row(17 * 32, 20.0, seed=1)
    p = np.full(17, 20.0, np.float32)
    p[1], p[2] = tmax32(128), 2.0
    p[3], p[4] = np.nextafter(tmax32(128), np.float32(np.inf)), np.nextafter(np.float32(2.0), np.float32(0))
    p[5], p[6], p[7], p[9] = 0.0, np.nan, -3.0, 13.37
    return x, p


def silent_inside():
    x = R.harmonic_row(12 * 32, 8.0, seed=2)
    x[140:260] = 0.0                                                     # frames 5, 6 and 7 at T = 8 (half = 12) see zeros only
    return x, np.full(12, 8.0, np.float32)


def case(name):
    """-> (geometry, x (B, L) with NaN behind the rows, lens, period (B, NF) with NaN past the rows' frames)."""
    def pack(geom, rows, lens_over=None):
        x, lens = R.padded([r for r, _ in rows])
        NF = -(-x.shape[1] // geom[2])
        p = np.full((len(rows), NF), np.nan, np.float32)
        for b, (_, pr) in enumerate(rows):
            p[b, :len(pr)] = pr
        return geom, x, (lens if lens_over is None else lens_over), p

    if name == "small3":                                                 # B = 3 with an empty row and a length that is no multiple of H
        return pack(SMALL, [row_a(), (np.zeros(0, np.float32), np.zeros(0, np.float32)), (R.harmonic_row(153, 11.5, seed=3), np.full(5, 11.5, np.float32))])
    if name == "misc":                                                   # a silent stretch, len < H, an all-unvoiced row, len > L (an empty row)
        rows = [silent_inside(), (R.harmonic_row(20, 6.0, seed=4), np.full(1, 6.0, np.float32)),
                (R.harmonic_row(300, 9.0, seed=5), np.zeros(10, np.float32)), (R.harmonic_row(100, 9.0, seed=6), np.full(4, 9.0, np.float32))]
        return pack(SMALL, rows, [12 * 32, 20, 300, 12 * 32 + 1])
    if name == "big":                                                    # 22050 / 1024 / 256, 2 rows x 40 frames
        p0 = np.full(40, 147.0, np.float32)
        p0[3], p0[4], p0[5], p0[6] = tmax32(1024), 2.0, 0.0, np.nextafter(tmax32(1024), np.float32(np.inf))
        p1 = np.full(40, 60.5, np.float32)
        p1[10], p1[39] = 2.0, tmax32(1024)
        return pack(BIG, [(R.harmonic_row(40 * 256, 147.0, seed=7), p0), (R.harmonic_row(40 * 256 - 100, 60.5, seed=8), p1)])
    raise KeyError(name)


def default_period(geom):
    return geom[0] / 500.0


def case_ref(name, n_mcep, alpha, mutant=None):
    geom, x, lens, p = case(name)
    Aw = audio.freq_warp_matrix(geom[1] // 2 + 1, n_mcep - 1, alpha)
    return R.envelope(x, lens, p, geom[2], geom[1], Aw, default_period(geom), mutant=mutant)


@pytest.fixture(scope="module")
def engines():
    yield from A.engines_on_demand(lambda key: A.engine_with(load, *key))


def run_case(engines, name, n_mcep, alpha, null=()):
    geom, x, lens, p = case(name)
    ref = A.frozen(_REF, (name, n_mcep, alpha), lambda: case_ref(name, n_mcep, alpha))
    eng = engines((geom, n_mcep, alpha))
    rc, dev = raw(eng, x, lens, p, geom, n_mcep, null=null)
    assert rc == 0, err_of(eng)
    check(dev, ref, f"{name} x {x.shape} n_mcep {n_mcep} alpha {alpha}")
    return geom, x, lens, p, ref, dev, eng


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_mcep,alpha", [("small3", 5, 0.455), ("small3", 1, 0.0), ("small3", 25, 0.455), ("small3", 25, 0.0),
                                               ("misc", 5, 0.455), ("big", 25, 0.455)])
def test_case_against_the_restatement(engines, name, n_mcep, alpha):
    geom, x, lens, p, ref, dev, eng = run_case(engines, name, n_mcep, alpha)
    for b, n in enumerate(lens):
        nf = R.frames_of(n, x.shape[1], geom[2])
        assert (dev["class"][b, nf:] == [3, 0, 0]).all() and not dev["env"][b, nf:].any() and not dev["mcep"][b, nf:].any(), "zeros past the row"
        assert (dev["class"][b, :nf, 0] < 3).all()
    silent = dev["class"][..., 0] == 2
    assert not dev["env"][silent].any() and not dev["mcep"][silent].any(), "a silent frame is zeros"
    rc, lean = raw(eng, x, lens, p, geom, n_mcep, null=("env",))
    assert rc == 0 and lean["env"] is None and same_bits(dev, lean, ("mcep", "class")), "without d_env: the same bits"


def test_the_named_cases_hold_what_their_names_say(engines):
    c = A.frozen(_REF, ("small3", 5, 0.455), lambda: case_ref("small3", 5, 0.455))["class"]
    assert c[0, :8, 0].tolist() == [0, 0, 0, 1, 1, 1, 1, 1] and c[0, 16, 0] == 0, "both limits are inside, the neighbours and the unvoiced take the default"
    assert c[0, 1, 1] == 62 and 2 * c[0, 1, 1] + 1 == 128 - 3, "the longest window: K = nfft - 3"
    assert c[0, 2, 1:].tolist() == [3, 64], "the shortest window; kd = nfft / 2: the widest correction and smoothing"
    assert c[0, 3, 1:].tolist() == [12, 16], "the default period 8"
    assert (c[1, :, 0] == 3).all() and c[2, :5, 0].tolist() == [0] * 5 and (c[2, 5:, 0] == 3).all()
    m = A.frozen(_REF, ("misc", 5, 0.455), lambda: case_ref("misc", 5, 0.455))["class"]
    assert m[0, :, 0].tolist() == [0, 0, 0, 0, 0, 2, 2, 2, 0, 0, 0, 0], "the silent stretch inside a voiced row"
    assert m[1, :, 0].tolist() == [0] + [3] * 11 and m[2, :10, 0].tolist() == [1] * 10 and (m[3, :, 0] == 3).all()


# ---- 2. the identities: bit-equal outputs ---------------------------------------------------------------------------------------------------
def test_row_alone_in_a_batch_at_a_larger_L_twice_and_under_every_arithmetic(engines):
    geom, n_mcep = SMALL, 5
    eng = engines((geom, n_mcep, 0.455))
    x, p = row_a()
    x, p = x[:-9], p.copy()                                              # (17 frames still, the last one short)
    rc, alone = raw(eng, x[None], None, p[None], geom, n_mcep)
    assert rc == 0, err_of(eng)
    n0 = eng.alloc_count()
    rc, again = raw(eng, x[None], None, p[None], geom, n_mcep)
    assert rc == 0 and same_bits(alone, again) and eng.alloc_count() == n0, "a second call: the same bits, no allocation"
    other = R.harmonic_row(700, 15.0, seed=9)
    xb, lb = R.padded([other, x, other[:100]], L=900)
    NF = -(-900 // 32)
    pb = np.full((3, NF), 15.0, np.float32)
    pb[1, :17] = p
    pb[1, 17:] = np.nan
    rc, batch = raw(eng, xb, lb, pb, geom, n_mcep)
    assert rc == 0 and np.isnan(xb[1, len(x):]).all(), "NaN behind the row"
    for k in NAMES:
        assert np.array_equal(alone[k][0], batch[k][1, :17]), f"d_{k}: alone against inside a batch at a larger L"
    assert (batch["class"][1, 17:] == [3, 0, 0]).all() and not batch["mcep"][1, 17:].any() and not batch["env"][1, 17:].any()
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 6, 16):
            eng.set_arithmetic(setting)
            rc, got = raw(eng, xb, lb, pb, geom, n_mcep)
            assert rc == 0 and same_bits(got, batch), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


def test_a_captured_graph_replays_the_eager_bits(engines):
    geom, x, lens, p = case("small3")
    n_mcep, alpha = 5, 0.455
    rc, raw_out = raw(engines((geom, n_mcep, alpha)), x, lens, p, geom, n_mcep)
    assert rc == 0
    eng = A.engine_with()                                                # (through Engine.load_envelope / Engine.envelope, the bindings)
    try:
        eng.load_envelope(audio.stoi_twiddle(geom[1]), geom[2], geom[1], geom[0], audio.freq_warp_matrix(geom[1] // 2 + 1, n_mcep - 1, alpha))
        xd, ld, pd = torch.from_numpy(x).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), torch.from_numpy(p).to(DEV)
        full = eng.envelope(xd, ld, pd, R.FLOOR, want_envelope=True)     # (the call that sizes the arena)
        torch.cuda.synchronize()
        n0 = eng.alloc_count()
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            eng.envelope(xd, ld, pd, R.FLOOR, want_envelope=True)
            torch.cuda.synchronize()
            assert eng.alloc_count() == n0, "the arena has its size"
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = eng.envelope(xd, ld, pd, R.FLOOR, want_envelope=True)
            for t in out:
                t.fill_(5)
            graph.replay()
            torch.cuda.synchronize()
        for a, b, k in zip(out, full, NAMES):
            assert torch.equal(a, b), "the replay equals the eager call"
            assert np.array_equal(a.cpu().numpy(), raw_out[k]), "and the raw call on another handle"
    finally:
        eng.close()


# ---- 3. mutants of the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_device_disagrees_with_each_mutant(engines, mutant):
    geom, x, lens, p, ref, dev, eng = run_case(engines, "small3", 5, 0.455)
    mut = case_ref("small3", 5, 0.455, mutant=mutant)
    far = max(float(np.abs(dev["env"] - mut["env"]).max()), float(np.abs(dev["mcep"] - mut["mcep"]).max()))
    print(f"\nenvelope mutant {mutant}: the device is {far:.3e} from it (gate {GATE:g})")
    assert far > GATE, f"the device agrees with the mutant {mutant}"


# ---- 4. limits --------------------------------------------------------------------------------------------------------------------------------
NAN_TW = audio.stoi_twiddle(128).copy()
NAN_TW[5, 0] = np.nan
NAN_WARP = audio.freq_warp_matrix(65, 4, 0.455)
NAN_WARP[2, 3] = np.inf
BAD_LOADS = [
    ("nfft=", dict(nfft=130 + 1)), ("nfft=", dict(nfft=14)), ("nfft=", dict(nfft=1026)), ("H=", dict(H=0)), ("H=", dict(H=513)),
    ("n_mcep=", dict(n_mcep=0)), ("n_mcep=", dict(n_mcep=65)), ("sr=", dict(sr=0.0)), ("sr=", dict(sr=float("nan"))), ("q1=", dict(q1=float("inf"))),
    ("default_period", dict(default_period=float("nan"))), ("default_period", dict(default_period=1.5)), ("default_period", dict(default_period=41.7)),
    ("default_period", dict(sr=500.0)), ("non-null", dict(null=("twiddle",))), ("non-null", dict(null=("warp",))), ("twiddle[10]", dict(tw=NAN_TW)),
    ("warp[133]", dict(warp=NAN_WARP)),
]
BAD_CALLS = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)), ("power_floor", dict(floor=0.0)), ("power_floor", dict(floor=float("inf"))),
    ("power_floor", dict(floor=float("nan"))), ("d_x", dict(null=("x",))), ("d_period", dict(null=("period",))), ("d_mcep", dict(null=("mcep",))),
    ("d_class", dict(null=("class",))),
]


@pytest.mark.parametrize("word,kw", BAD_LOADS, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_LOADS)])
def test_each_limit_of_the_load_fails_with_a_message_naming_it(word, kw):
    kw = dict(kw)
    eng = A.engine_with()
    try:
        n0 = eng.alloc_count()
        big = np.ones((1040, 2))                                         # (large enough for every nfft tried: nothing past a table is read)
        rc = load(eng, SMALL, kw.pop("n_mcep", 5), 0.455, **{"tw": big, "warp": np.ones((65, 600)), **kw})
        msg = err_of(eng)
        assert rc != 0 and "ev_load_envelope" in msg and word in msg, msg
        assert eng.alloc_count() == n0
        rc, _ = raw(eng, np.zeros((1, 256), np.float32), None, np.zeros((1, 8), np.float32), SMALL, 5)
        assert rc != 0 and "not loaded" in err_of(eng), "a failed load loads nothing"
    finally:
        eng.close()


@pytest.mark.parametrize("word,kw", BAD_CALLS, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALLS)])
def test_each_limit_of_the_call_fails_with_a_message_naming_it(engines, word, kw):
    eng = engines((SMALL, 5, 0.455))
    n0 = eng.alloc_count()
    rc, _ = raw(eng, np.zeros((2, 256), np.float32), None, np.zeros((2, 8), np.float32), SMALL, 5, **kw)   # (a failed call writes nothing: raw checks)
    msg = err_of(eng)
    assert rc != 0 and "ev_envelope" in msg and word in msg, msg
    assert eng.alloc_count() == n0, "a failed call leaves ev_alloc_count unmoved"


def test_a_call_before_any_load_fails_and_a_failed_reload_keeps_the_tables():
    geom, x, lens, p = case("small3")
    eng = A.engine_with()
    try:
        rc, _ = raw(eng, x, lens, p, geom, 5)
        assert rc != 0 and "ev_load_envelope" in err_of(eng)
        n0 = eng.alloc_count()
        assert load(eng, geom, 5, 0.455) == 0 and eng.alloc_count() == n0 + 1, "the load owns one block"
        rc, first = raw(eng, x, lens, p, geom, 5)
        assert rc == 0, err_of(eng)
        assert load(eng, geom, 5, 0.455, tw=NAN_TW) != 0 and "twiddle[10]" in err_of(eng)
        rc, kept = raw(eng, x, lens, p, geom, 5)
        assert rc == 0 and same_bits(first, kept), "a failed load leaves the previous tables in use"
        assert load(eng, geom, 5, 0.0) == 0, err_of(eng)
        rc, other = raw(eng, x, lens, p, geom, 5)
        assert rc == 0
        check(other, A.frozen(_REF, ("small3", 5, 0.0), lambda: case_ref("small3", 5, 0.0)), "a second load replaces the first")
    finally:
        eng.close()
