"""ev_load_speech_rate / ev_speech_rate on the MI355X, through the C ABI.

Yardstick: tests/speech_rate_ref.py, the numpy float64 restatement with the header's orders (64 slots, the xor tree, selection on bit patterns).
The rule of every comparison (``check``): each case first asserts ``margin >= 1e-6`` (the least relative distance between the two sides of any
comparison a decision rests on: raw, peak rule, dips, rank neighbours); then d_mark and d_count must be EQUAL to the restatement, and d_power and
d_stat are compared by test_gpu_loudness.py's rule, relative to max(|ref|, 1e-9 x the row's largest |ref|), within the project's 1e-9 gate.
H = 64 throughout; every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py); inputs carry NaN behind each row's length.

Two cases that the definition itself rules out, and what stands in their place: with nf = 3 frame 1 MAY be a candidate
(1 <= f <= nf - 2), so "no candidate" is asserted for nf in {1, 2} and nf = 3 is held to the restatement; the dip interval is never EMPTY (the
frame behind a candidate is never a candidate, by the peak rule), so the case is the interval of exactly one frame, a candidate at nf - 2.

Observed on the MI355X (printed by every case; the gate stays as it is): d_power and d_stat came out BIT-EQUAL to the restatement on every
case (relative error 0 against the gate 1e-9), NF = 16384 and W = 4096 included; the least margin of any case is 3.6e-5 (b5-w256).  The mutants
lie 2.1 (no fill), 1.0 ((b) before (a)), 0.19 (rank k + 1: ref alone, marks and counts equal) and 1.1e11 (no mean subtraction) from the device;
the dip before the peak (15 nuclei for 14), >= on the left (16 candidates for 2) and the last candidate never counted (0 nuclei for 1) leave the
floats alone and differ in marks and counts.

Times: not gated here (tools/speech_rate_bench.py).
"""
import numpy as np
import pytest
import torch

import analysis_gpu as A
import speech_rate_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd._lib import _stream_ptr

pytestmark = pytest.mark.gpu

_REF = {}
H = R.H0
NAMES = ("power", "mark", "stat", "count")
WIN = lambda W: np.kaiser(W, 20.24).astype(np.float64)


def load(eng, W, H_=H, window=None, null=False):
    w = np.ascontiguousarray(WIN(W) if window is None else window, dtype=np.float64)
    return eng.lib.ev_load_speech_rate(eng.h, None if null else w.ctypes.data, W, H_)


def raw(eng, x, lens, par, voiced=None, B=None, L=None, null=(), H_=H, **over):
    """ev_speech_rate into guarded buffers -> (rc, {"power", "mark", "stat", "count"} on the host; None where passed as NULL).  ``B`` / ``L``
    override the shape passed to the library, ``over`` the scalar arguments, ``null`` names pointers passed as NULL."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    NF = -(-Lx // H_)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    d_v = None if voiced is None else torch.as_tensor(np.asarray(voiced), dtype=torch.uint8).to(DEV).contiguous()
    sil, dip = R.ratios(par)
    a = dict(power_floor=par["power_floor"], rank_fraction=par["rank_fraction"], silence_ratio=sil, dip_ratio=dip, min_pause=par["min_pause"],
             min_sound=par["min_sound"])
    a.update(over)
    out = A.Guarded({"power": ((Bx, NF), torch.float64), "mark": ((Bx, NF), torch.uint8), "stat": ((Bx, 4), torch.float64),
                     "count": ((Bx, 8), torch.int32)}, tuple(n for n in null if n in NAMES))
    rc = eng.lib.ev_speech_rate(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(),
                                None if d_v is None else d_v.data_ptr(), Bx if B is None else B, Lx if L is None else L, a["power_floor"],
                                a["rank_fraction"], a["silence_ratio"], a["dip_ratio"], a["min_pause"], a["min_sound"], out.ptr("power"),
                                out.ptr("mark"), out.ptr("stat"), out.ptr("count"), _stream_ptr())
    return rc, out.collect(rc)


def same_bits(a, b, names=NAMES):
    return all(np.array_equal(a[k], b[k]) for k in names)


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    margin = float(ref["margin"].min())
    err = {k: R.rel_err(dev[k], ref[k]) for k in R.FLOAT_OUTPUTS}
    print(f"\nspeech rate {what}: rel err power {err['power']:.3e} stat {err['stat']:.3e} (gate 1e-9)  P bit-equal "
          f"{np.array_equal(dev['power'], ref['power'])}  least margin {margin:.3e}  count {dev['count'].tolist()}")
    assert margin >= 1e-6, f"{what}: a comparison of the reference has its sides {margin:.3e} apart"
    assert np.array_equal(dev["count"], ref["count"]), f"{what}: d_count {dev['count'].tolist()} against {ref['count'].tolist()}"
    assert np.array_equal(dev["mark"], ref["mark"]), f"{what}: d_mark differs at {np.argwhere(dev['mark'] != ref['mark'])[:8].tolist()}"
    for k in R.FLOAT_OUTPUTS:
        assert err[k] <= 1e-9, f"{what}: d_{k}"


@pytest.fixture(scope="module")
def engines():
    yield from A.engines_on_demand(lambda W: A.engine_with(load, W))


def run_case(engines, name):
    x, lens, W, par = R.case(name)
    ref = A.frozen(_REF, name, lambda: R.case_ref(name))
    rc, dev = raw(engines(W), x, lens, par)
    assert rc == 0, err_of(engines(W))
    check(dev, ref, f"{name} x {x.shape} W {W}")
    return x, lens, W, par, ref, dev


# ---- 1. the cases ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_case_against_the_restatement(engines, name):
    x, lens, W, par, ref, dev = run_case(engines, name)
    for b, n in enumerate(lens):
        nf = R.frames_of(n, x.shape[1], H)
        assert dev["count"][b, 0] == nf and not dev["power"][b, nf:].any() and not dev["mark"][b, nf:].any(), "zeros past the row's own frames"
        assert dev["count"][b, [1, 3, 6, 7]].sum() == nf, "sounding + pause + leading + trailing frames = nf"
        if nf == 0:
            assert not any(dev[k][b].any() for k in dev), "len 0 and len > L are rows of zeros"
        if nf in (1, 2):
            assert dev["count"][b, 4] == 0, "no candidate is possible"


def test_the_named_cases_hold_what_their_names_say(engines):
    c = lambda name: A.frozen(_REF, name, lambda: R.case_ref(name))
    assert c("lengths")["count"][:, 0].tolist() == [0, 1, 1, 1, 2, 2, 4, 3, 21, 0]
    for name in ("b1-w128", "b3-w192", "b5-w256"):                       # the ground truth of the generator: 14 bursts, 3 interior gaps
        assert (c(name)["count"][:, 5] == 14).all() and (c(name)["count"][:, 2] == 3).all()
    assert c("last-only")["count"][0, 4:6].tolist() == [1, 1], "the only candidate is the last one, and it counts"
    one = c("one-frame-dip")
    assert np.flatnonzero(one["mark"][0] & R.CAND).tolist() == [one["count"][0, 0] - 2], "the dip interval holds exactly one frame"
    raw_runs = lambda name, b: [(e - s + 1, v) for s, e, v in R.runs_of(c(name)["mark"][b, :c(name)["count"][b, 0]] & R.RAW)]
    assert (7, False) in raw_runs("pause-edges", 0) and c("pause-edges")["count"][0, 2] == 0, "a silent run of min_pause - 1 is filled"
    assert (8, False) in raw_runs("pause-edges", 1) and c("pause-edges")["count"][1, 2:4].tolist() == [1, 8], "one of min_pause is a pause"
    assert (3, True) in raw_runs("sound-edges", 0) and c("sound-edges")["count"][0, 1] == 0, "a sounding run of min_sound - 1 is dropped"
    assert (4, True) in raw_runs("sound-edges", 1) and c("sound-edges")["count"][1, 1] == 4, "one of min_sound stays"
    s = c("silent-and-sounding")["count"]
    assert s[0, [1, 6, 7]].tolist() == [0, 30, 0] and s[1, 1] == 30


def test_exact_ties_on_a_plateau(engines):
    x, lens, W, par, ref, dev = run_case(engines, "plateau")
    P, mark = dev["power"][0], dev["mark"][0]
    assert np.array_equal(dev["power"], ref["power"]) and len(set(P[9:15].tolist())) == 1, "frames of identical samples: bit-equal power"
    assert not (mark[10:15] & R.CAND).any(), "the plateau gives no candidate: > on the left"
    assert mark[9] & R.CAND and P[9] == P[10] and mark[9] & R.NUC, "its first frame is one, >= on the right, and the step down is its dip"


def test_the_lds_ceiling_and_the_longest_window(engines):
    row = np.tile(R.bursts(H, seed=11)[0][: 128 * H], 128)               # NF = 16384 exactly
    assert len(row) == 16384 * H
    ref = A.frozen(_REF, "ceiling", lambda: R.speech_rate(row[None], None, WIN(128), H))
    rc, dev = raw(engines(128), row[None], None, R.PAR)
    assert rc == 0, err_of(engines(128))
    check(dev, ref, "NF = 16384, W = 128")
    rc, lean = raw(engines(128), row[None], None, R.PAR, null=("power", "mark"))
    assert rc == 0 and same_bits(dev, lean, ("stat", "count")), "without d_power and d_mark: the same bits"
    rc, _ = raw(engines(128), np.zeros((1, 16384 * H + 1), np.float32), None, R.PAR)
    assert rc != 0 and "NF=16385" in err_of(engines(128)), "NF = 16385 is refused"
    x, lens = R.padded([R.bursts(H, groups=(3, 2), seed=12)[0][: 80 * H - 9]])
    ref = A.frozen(_REF, "w4096", lambda: R.speech_rate(x, lens, WIN(4096), H))
    rc, dev = raw(engines(4096), x, lens, R.PAR)
    assert rc == 0, err_of(engines(4096))
    check(dev, ref, "nf = 80, W = 4096")


# ---- 2. the identities: bit-equal outputs ----------------------------------------------------------------------------------------------------
def test_row_alone_in_a_batch_as_a_prefix_twice_without_outputs_and_under_every_arithmetic(engines):
    eng, par = engines(192), R.PAR
    row = R.bursts(H, seed=21)[0][:-23]
    nf = -(-len(row) // H)
    rc, alone = raw(eng, row[None], None, par)
    assert rc == 0 and alone["count"][0, 0] == nf, err_of(eng)
    for null in (("power",), ("mark",), ("power", "mark")):
        rc, lean = raw(eng, row[None], None, par, null=null)
        assert rc == 0 and same_bits(alone, lean, [k for k in NAMES if k not in null]) and all(lean[k] is None for k in null)
    n0 = eng.alloc_count()
    rc, again = raw(eng, row[None], None, par, null=("power",))
    assert rc == 0 and same_bits(alone, again, NAMES[1:]) and eng.alloc_count() == n0, "a second call: the same bits, no allocation"
    xb, lb = R.padded([R.bursts(H, seed=22)[0], row, R.bursts(H, groups=(2,), seed=23)[0]])
    rc, batch = raw(eng, xb, lb, par)
    assert rc == 0
    xp, lp = R.padded([R.bursts(H, groups=(1,), seed=24)[0], row], L=len(row) + 1234)
    rc, prefix = raw(eng, xp, lp, par)
    assert rc == 0 and np.isnan(xp[1, len(row):]).all(), "NaN behind the row"
    for got, what in ((batch, "inside a batch"), (prefix, "the prefix of a longer row with NaN behind it")):
        for k in ("power", "mark"):
            assert np.array_equal(alone[k][0], got[k][1, :alone[k].shape[1]]) and not got[k][1, nf:].any(), f"d_{k}: alone against {what}"
        assert all(np.array_equal(alone[k][0], got[k][1]) for k in ("stat", "count")), f"alone against {what}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 6, 16):
            eng.set_arithmetic(setting)
            rc, got = raw(eng, xb, lb, par)
            assert rc == 0 and same_bits(got, batch), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


def test_a_captured_graph_replays_the_eager_bits(engines):
    x, lens, W, par = R.case("b3-w192")
    rc, raw_out = raw(engines(W), x, lens, par)
    assert rc == 0
    sil, dip = R.ratios(par)
    args = (par["power_floor"], par["rank_fraction"], sil, dip, par["min_pause"], par["min_sound"])
    eng = A.engine_with()                                                # (through Engine.load_speech_rate / Engine.speech_rate, the bindings)
    try:
        eng.load_speech_rate(WIN(W), H)
        xd, ld = torch.from_numpy(x).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
        full = eng.speech_rate(xd, ld, None, *args)
        eng.speech_rate(xd, ld, None, *args, want_power=False)           # (the warm-up call that sizes the arena)
        torch.cuda.synchronize()
        n0 = eng.alloc_count()
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            eng.speech_rate(xd, ld, None, *args, want_power=False)
            torch.cuda.synchronize()
            assert eng.alloc_count() == n0, "the arena has its size"
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = eng.speech_rate(xd, ld, None, *args, want_power=False)
            for t in out[1:]:
                t.fill_(5)
            graph.replay()
            torch.cuda.synchronize()
        assert out[0] is None
        for a, b, k in zip(out[1:], full[1:], NAMES[1:]):
            assert torch.equal(a, b), "the replay equals the eager call"
            assert np.array_equal(a.cpu().numpy(), raw_out[k]), "and the raw call on another handle"
    finally:
        eng.close()


# ---- 3. voicing ------------------------------------------------------------------------------------------------------------------------------
def test_voicing_removes_exactly_the_nuclei_it_covers(engines):
    x, lens, W, par, ref, dev = run_case(engines, "b3-w192")
    eng, (B, NF) = engines(W), dev["mark"].shape
    rc, ones = raw(eng, x, lens, par, voiced=np.ones((B, NF), np.uint8))
    assert rc == 0 and same_bits(ones, dev), "d_voiced all ones: the outputs of NULL"
    nuclei = np.argwhere(dev["mark"] & R.NUC)
    b0, f0 = nuclei[len(nuclei) // 2]
    v = np.ones((B, NF), np.uint8)
    v[b0, f0] = 0
    rc, cut = raw(eng, x, lens, par, voiced=v)
    want = dev["mark"].copy()
    want[b0, f0] &= ~np.uint8(R.NUC)
    assert rc == 0 and np.array_equal(cut["mark"], want) and cut["count"][b0, 5] == dev["count"][b0, 5] - 1, "a zero at a nucleus removes that nucleus"
    assert np.array_equal(np.delete(cut["count"], 5, axis=1), np.delete(dev["count"], 5, axis=1)) and same_bits(cut, dev, ("power", "stat"))
    wv = R.speech_rate(x, lens, WIN(W), H, par, voiced=v)
    assert np.array_equal(cut["mark"], wv["mark"]) and np.array_equal(cut["count"], wv["count"]), "as the restatement has it"
    v = ((dev["mark"] & R.CAND) > 0).astype(np.uint8) * 200              # (any non-zero byte is voiced; zeros at every non-candidate)
    rc, only = raw(eng, x, lens, par, voiced=v)
    assert rc == 0 and same_bits(only, dev), "bytes at non-candidates change nothing"


# ---- 4. mutants of the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_device_disagrees_with_each_mutant(engines, mutant):
    name = R.MUTANT_CASE[mutant]
    x, lens, W, par, ref, dev = run_case(engines, name)
    far, counts_differ = R.mutant_distance(dev, R.case_ref(name, mutant=mutant))
    print(f"\nspeech rate mutant {mutant} on {name}: the device is {far:.3e} from it; marks or counts differ: {counts_differ}")
    assert far > 1e-9 or counts_differ, f"the device agrees with the mutant {mutant}"


# ---- 5. limits -------------------------------------------------------------------------------------------------------------------------------
NAN_WIN = WIN(128)
NAN_WIN[5] = np.nan
BAD_LOADS = [
    ("W=", dict(W=6)), ("W=", dict(W=4098)), ("W=", dict(W=129)), ("H=", dict(H_=32)), ("H=", dict(H_=96)), ("H=", dict(H_=1088)),
    ("non-null", dict(W=128, null=True)), ("window[5]", dict(W=128, window=NAN_WIN)), ("sw=", dict(W=128, window=np.zeros(128))),
    ("sw=", dict(W=128, window=-WIN(128))),
]
BAD_CALLS = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)), ("NF=", dict(L=16384 * H + 1)), ("power_floor", dict(power_floor=0.0)),
    ("power_floor", dict(power_floor=float("inf"))), ("power_floor", dict(power_floor=float("nan"))), ("rank_fraction", dict(rank_fraction=-0.1)),
    ("rank_fraction", dict(rank_fraction=1.0)), ("silence_ratio", dict(silence_ratio=0.0)), ("silence_ratio", dict(silence_ratio=1.0)),
    ("dip_ratio", dict(dip_ratio=0.99)), ("dip_ratio", dict(dip_ratio=float("inf"))), ("min_pause", dict(min_pause=0)),
    ("min_pause", dict(min_pause=4097)), ("min_sound", dict(min_sound=0)), ("min_sound", dict(min_sound=4097)), ("d_x", dict(null=("x",))),
    ("d_stat", dict(null=("stat",))), ("d_count", dict(null=("count",))),
]


@pytest.mark.parametrize("word,kw", BAD_LOADS, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_LOADS)])
def test_each_limit_of_the_load_fails_with_a_message_naming_it(word, kw):
    kw = dict(kw)
    eng = A.engine_with()
    try:
        n0 = eng.alloc_count()
        rc = load(eng, kw.pop("W", 4096), **{"window": np.ones(8192), **kw})
        msg = err_of(eng)
        assert rc != 0 and "ev_load_speech_rate" in msg and word in msg, msg
        assert eng.alloc_count() == n0
        rc, _ = raw(eng, np.zeros((1, 512), np.float32), None, R.PAR)
        assert rc != 0 and "not loaded" in err_of(eng), "a failed load loads nothing"
    finally:
        eng.close()


@pytest.mark.parametrize("word,kw", BAD_CALLS, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALLS)])
def test_each_limit_of_the_call_fails_with_a_message_naming_it(engines, word, kw):
    eng = engines(128)
    n0 = eng.alloc_count()
    rc, _ = raw(eng, np.zeros((2, 1024), np.float32), None, R.PAR, **kw)  # (a failed call writes nothing, margins intact: raw checks that)
    msg = err_of(eng)
    assert rc != 0 and "ev_speech_rate" in msg and word in msg, msg
    assert eng.alloc_count() == n0, "a failed call leaves ev_alloc_count unmoved"


def test_a_call_before_any_load_fails_and_a_failed_reload_keeps_the_tables():
    x, lens, W, par = R.case("b1-w128")
    eng = A.engine_with()
    try:
        rc, _ = raw(eng, x, lens, par)
        assert rc != 0 and "ev_load_speech_rate" in err_of(eng)
        n0 = eng.alloc_count()
        assert load(eng, W) == 0 and eng.alloc_count() == n0 + 1, "the load owns one block"
        rc, first = raw(eng, x, lens, par)
        assert rc == 0, err_of(eng)
        assert load(eng, 130, window=NAN_WIN.tolist() + [1.0, 1.0]) != 0 and "window[5]" in err_of(eng)
        rc, kept = raw(eng, x, lens, par)
        assert rc == 0 and same_bits(first, kept), "a failed load leaves the previous tables in use"
        assert load(eng, 256) == 0, err_of(eng)
        rc, other = raw(eng, x, lens, par)
        ref = R.speech_rate(x, lens, WIN(256), H, par)
        assert rc == 0 and np.array_equal(other["mark"], ref["mark"]) and R.rel_err(other["power"], ref["power"]) <= 1e-9, "a second load replaces the first"
    finally:
        eng.close()
