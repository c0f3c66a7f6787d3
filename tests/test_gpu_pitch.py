"""ev_pitch_yin on the MI355X, through the C ABI.

Yardstick: tests/pitch_ref.py, the numpy float64 restatement of the header's semantics (librosa is not a dependency).  The device sums the
same exact float64 squares in another order (four quarters of the window, one fma per term), so d(tau) differs from the restatement's by a
few 2^-53 relative and d' likewise.  The rule of every comparison (``check``):
  * d_lag is EQUAL on every frame whose decision margin (pitch_ref: the least distance of a comparison of the decision from flipping) is
    at least 1e-9, seven orders above that rounding; frames below it are left out, and at most 2 % of a case's frames may be;
    tests/test_pitch_host.py asserts on the CPU that the parity rows leave out none;
  * |period - ref| <= 1e-5 ref on the voiced frames: the output is ONE float32 rounding (2^-24 = 6e-8 relative) of a float64 value;
  * d_cmnd within 1e-5 relative, by the same argument.
Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py).  Inputs carry loud garbage behind each row's d_len samples.

Times: not gated here (tools/pitch_bench.py).
"""
import numpy as np
import pytest
import torch

import analysis_gpu as A
import pitch_ref as P
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, EvLibraryError, _stream_ptr

pytestmark = pytest.mark.gpu

GARBAGE = P.GARBAGE
STD = P.STD
_REF = {}


def ref_of(key, x, lens, **kw):
    """The restatement's result, computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: P.pitch_yin(x, lens, **kw))


def raw(eng, x, lens, frame_length=1024, hop_length=256, tau_min=36, tau_max=340, threshold=0.1, want=(True, True, True)):
    """ev_pitch_yin into guarded buffers: (rc, lag, period, cmnd), each (B, F) on the host or None."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    B, L = x.shape
    F = -(-L // hop_length)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"lag": ((B, F), torch.int32), "period": ((B, F), torch.float32), "cmnd": ((B, F), torch.float32)},
                    tuple(k for k, w in zip(("lag", "period", "cmnd"), want) if not w))
    rc = eng.lib.ev_pitch_yin(eng.h, x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, frame_length, hop_length, tau_min, tau_max,
                              threshold, out.ptr("lag"), out.ptr("period"), out.ptr("cmnd"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def check(dev, ref, what, may_leave_out=None):
    """The comparison rule of the module docstring; prints the figures before it asserts.  ``may_leave_out``: the number of frames the case is
    KNOWN to leave out (its caller says why and checks them itself) instead of the 2 % allowance."""
    lag, period, cmnd = dev
    keep = ref["margin"] >= 1e-9
    left_out = int((~keep).sum())
    voiced = keep & (ref["lag"] > 0)
    e_p = float(np.max(np.abs(period[voiced] - ref["period"][voiced]) / ref["period"][voiced])) if voiced.any() else 0.0
    nz = keep & (ref["cmnd"] != 0)
    e_c = float(np.max(np.abs(cmnd[nz] - ref["cmnd"][nz]) / np.abs(ref["cmnd"][nz]))) if nz.any() else 0.0
    print(f"\nPITCH {what}: frames {keep.size} left out {left_out} voiced {int(voiced.sum())} lag mismatches {int((lag != ref['lag'])[keep].sum())} "
          f"period rel err {e_p:.3e} cmnd rel err {e_c:.3e} least margin {float(ref['margin'].min()):.3e}")
    if may_leave_out is None:
        assert left_out <= 0.02 * keep.size, f"{what}: {left_out} of {keep.size} frames have a decision margin under 1e-9"
    else:
        assert left_out == may_leave_out, f"{what}: {left_out} frames have a decision margin under 1e-9, {may_leave_out} expected"
    assert np.array_equal(lag[keep], ref["lag"][keep]), f"{what}: d_lag"
    assert e_p <= 1e-5, f"{what}: d_period"
    assert np.all(period[keep & (ref["lag"] == 0)] == 0.0), f"{what}: d_period of unvoiced frames"
    assert e_c <= 1e-5, f"{what}: d_cmnd"
    assert np.all(cmnd[keep & (ref["cmnd"] == 0)] == 0.0), f"{what}: d_cmnd of frames past the row"


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
def test_parity_with_the_restatement(eng):
    x, lens = P.parity_rows()
    ref = ref_of("parity", x, lens, **STD)                                # (the restatement reads x[b, :len] only)
    assert int((ref["margin"] < 1e-9).sum()) == 0, "the parity rows must leave out no frame (change the seed)"
    assert (ref["lag"][0] > 0).sum() >= 26 and (ref["lag"][1] > 0).sum() >= 26 and (ref["lag"][2] > 0).sum() >= 4 and not ref["lag"][3].any()
    rc, *dev = raw(eng, x, lens, **STD)
    assert rc == 0, err_of(eng)
    check(dev, ref, "parity B4 L8192")
    assert np.all(dev[2][3] == 1.0), "a silent frame has d' = 1 at every lag"
    assert np.all(dev[0][2, 20:] == 0) and np.all(dev[2][2, 20:] == 0.0), "frames past ceil(5001 / 256) = 20"


# ---- 2. other geometries -----------------------------------------------------------------------------------------------------------------
GEOMETRIES = P.GEOMETRIES


@pytest.mark.parametrize("W,H,t0,t1,L,f0", GEOMETRIES, ids=[f"W{g[0]}-H{g[1]}-tau{g[2]}-{g[3]}" for g in GEOMETRIES])
def test_other_geometries(eng, W, H, t0, t1, L, f0):
    x = np.stack([P.harmonic_tone(f0, L), P.chirp(100.0, 300.0, L)])
    kw = dict(frame_length=W, hop_length=H, tau_min=t0, tau_max=t1, threshold=0.1)
    ref = ref_of(("geo", W, H, t0, t1), x, None, **kw)
    rc, *dev = raw(eng, x, None, **kw)
    assert rc == 0, err_of(eng)
    check(dev, ref, f"W{W} H{H} tau {t0}..{t1} L{L}")
    if t0 == t1 == 100:
        assert (ref["lag"][0] == 100).all()
    if t1 == 1:
        assert not ref["lag"].any() and np.all(dev[2] == 1.0)              # d'(1) is 1: nothing is ever voiced


# ---- 3. independence of batch and padding ------------------------------------------------------------------------------------------------
def test_row_alone_in_a_batch_and_as_a_prefix_give_the_same_bits(eng):
    x, lens = P.parity_rows()
    n = 5001
    row = x[2, :n]
    nf = -(-n // 256)
    rc, *alone = raw(eng, row[None], None, **STD)
    assert rc == 0
    rc, *again = raw(eng, row[None], None, **STD)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    rc, *batch = raw(eng, x, lens, **STD)
    assert rc == 0
    longer = np.full((2, n + 777), GARBAGE, np.float32)
    longer[1, :n] = row
    longer[0] = P.chirp(100.0, 300.0, n + 777)
    rc, *prefix = raw(eng, longer, [n + 777, n], **STD)
    assert rc == 0
    for name, a, b, c in zip(("lag", "period", "cmnd"), alone, batch, prefix):
        assert a.shape[1] == nf
        assert np.array_equal(a[0], b[2, :nf]), f"{name}: alone against inside a batch"
        assert np.array_equal(a[0], c[1, :nf]) and not c[1, nf:].any(), f"{name}: alone against the prefix of a padded row"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 6, 16):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, x, lens, **STD)
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


# ---- 4. bad rows -------------------------------------------------------------------------------------------------------------------------
def test_bad_rows_are_zeros_and_short_rows_match(eng):
    L = 3000
    good = P.harmonic_tone(200.0, L)
    x = np.stack([np.full(L, GARBAGE, np.float32), good, np.full(L, GARBAGE, np.float32), np.full(L, GARBAGE, np.float32)])
    rc, *alone = raw(eng, good[None], None, **STD)
    assert rc == 0
    rc, *got = raw(eng, x, [0, L, -3, L + 1], **STD)
    assert rc == 0
    for a, g in zip(alone, got):
        assert not g[0].any() and not g[2].any() and not g[3].any(), "bad rows are zeros"
        assert np.array_equal(a[0], g[1]), "the good row next to them is unchanged"
    short = np.full((2, L), GARBAGE, np.float32)
    short[0, :1] = 0.25
    short[1, :100] = P.harmonic_tone(441.0, 100)
    ref = ref_of("short", short, [1, 100], **STD)
    rc, *dev = raw(eng, short, [1, 100], **STD)
    assert rc == 0
    # The one-sample row's only frame has d(tau) = 2 x^2 at EVERY lag (the sample meets a zero once as s[j] and once as s[j + tau]), so d' is 1 at
    # every lag up to rounding and the two smallest tie: the margin rule leaves that frame out, and it is held to its known answer instead.
    assert ref["margin"][0, 0] < 1e-9 and ref["lag"][0, 0] == 0 and abs(ref["cmnd"][0, 0] - 1.0) < 1e-12
    check(dev, ref, "len 1 and len 100", may_leave_out=1)
    assert dev[0][0, 0] == 0 and dev[1][0, 0] == 0.0 and abs(dev[2][0, 0] - 1.0) <= 1e-5, "the one-sample row: unvoiced, d' = 1"
    assert not dev[0][:, 1:].any() and not dev[2][:, 1:].any(), "one frame each"


# ---- 5. arguments ------------------------------------------------------------------------------------------------------------------------
BAD_ARGS = [
    ("B=", dict(), (0, 512)),
    ("B=", dict(), (65536, 64)),
    ("hop_length", dict(hop_length=0), None), ("hop_length", dict(hop_length=100), None), ("hop_length", dict(hop_length=4160), None),
    ("frame_length", dict(frame_length=0), None), ("frame_length", dict(frame_length=1000), None), ("frame_length", dict(frame_length=4160), None),
    ("tau_min", dict(tau_min=0), None), ("tau_min", dict(tau_min=341), None), ("tau_max", dict(tau_max=2049), None),
    ("threshold", dict(threshold=0.0), None), ("threshold", dict(threshold=1.5), None), ("threshold", dict(threshold=float("nan")), None),
    ("output", dict(want_lag=False, want_period=False, want_cmnd=False), None),
]


@pytest.mark.parametrize("word,kw,shape", BAD_ARGS, ids=[f"{w}-{i}" for i, (w, _, _) in enumerate(BAD_ARGS)])
def test_each_limit_fails_with_a_message_naming_it(eng, word, kw, shape):
    x = torch.zeros(shape or (2, 2048), device=DEV)
    with pytest.raises(EvLibraryError, match=word):
        eng.pitch_yin(x, **kw)


def test_any_output_may_be_null(eng):
    x, lens = P.parity_rows()
    rc, *full = raw(eng, x, lens, **STD)
    assert rc == 0
    for want in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)]:
        rc, *got = raw(eng, x, lens, want=want, **STD)
        assert rc == 0, err_of(eng)
        for w, g, f in zip(want, got, full):
            assert (g is None) if not w else np.array_equal(g, f), f"outputs {want}"


# ---- 6. allocation and capture -----------------------------------------------------------------------------------------------------------
def test_no_allocation_and_capturable():
    e = Engine(0)
    x, lens = P.parity_rows()
    xd = torch.from_numpy(x).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    n0 = e.alloc_count()
    ref = e.pitch_yin(xd, ld, **STD)
    e.pitch_yin(xd[:1, :1000].contiguous(), None, 64, 64, 1, 1, 0.5)
    e.pitch_yin(xd[:2, :4096].contiguous(), None, 4096, 4096, 1, 2048, 0.1)   # (more LDS than the default grant: the attribute, no allocation)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        e.pitch_yin(xd, ld, **STD)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = e.pitch_yin(xd, ld, **STD)
        for t in out:
            t.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b), "the replay equals the eager call"
    assert e.alloc_count() == n0
    e.close()


# ---- 7. audio.pitch_yin end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f0", [110.0, 220.0])
def test_audio_pitch_yin_recovers_the_tones(f0):
    y = torch.from_numpy(P.harmonic_tone(f0, 8192)).to(DEV)
    out = audio.pitch_yin(y)
    f, v, ap = out["f0"].cpu().numpy(), out["voiced"].cpu().numpy(), out["aperiodicity"].cpu().numpy()
    assert f.shape == v.shape == ap.shape == (1, 32) and out["f0"].dtype == torch.float32 and out["voiced"].dtype == torch.bool
    it = P.interior_frames(32, 8192)
    assert v[0][it].all() and np.all(f[~v] == 0)
    e_all, e_in = np.max(np.abs(f[v] / f0 - 1)), np.max(np.abs(f[0][it] / f0 - 1))
    print(f"\nPITCH audio.pitch_yin {f0} Hz: voiced {int(v.sum())}/32, rel err interior {e_in:.3e} all voiced {e_all:.3e}")
    assert e_in <= P.F0_TOL_INTERIOR and e_all <= P.F0_TOL_ALL                 # (established on the restatement: tests/test_pitch_host.py)
    assert np.all(ap[v] < 0.1)


def test_audio_pitch_yin_on_silence():
    out = audio.pitch_yin(torch.zeros(2, 4096, device=DEV), lengths=[4096, 1000])
    assert out["voiced"].shape == (2, 16) and not out["voiced"].any() and not out["f0"].any()
    ap = out["aperiodicity"].cpu().numpy()
    assert np.all(ap[0] == 1.0) and np.all(ap[1, :4] == 1.0) and np.all(ap[1, 4:] == 0.0)
