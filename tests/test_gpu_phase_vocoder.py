"""ev_load_phase_vocoder / ev_phase_vocoder on the MI355X, through the C ABI, and audio.time_stretch / audio.pitch_shift on top of it.

Yardstick: tests/phase_vocoder_ref.py, the numpy restatement of include/emojivoice.h's definition, in float64 and in longdouble.  The rule of every
comparison (``check``) has five parts:
  1. the input condition: the float64 and the longdouble restatement agree within INPUT_TOL (1e-11) of the row's largest |Y| (for d_stretch) and of
     the row's peak (for d_y) — a bin at rounding-noise level has an arbitrary angle which the accumulated phase carries on, so an input that
     fails this is ill-conditioned and proves nothing about the device;
  2. d_counts {nf, n_out} and d_out_len are EQUAL to the restatement;
  3. d_stretch lies within TOL (1e-9) x the row's largest |Y| of the longdouble restatement, compared as complex numbers, never as phases;
  4. |d_y - ref| <= 2^-24 |ref| + TOL x peak: the first term is the one float32 rounding;
  5. exact zeros behind n_out (d_stretch) and behind out_len (d_y).
Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py); inputs carry 50.0 behind each row's length.

Shapes, the smallest at which each path can go wrong: nfft 16 (H 4, NB 9: under one bin tile, the K tail 9 -> 12), 64 (NB 33: a one-column bin
tail, K tail 33 -> 36, one column tile per wave in the synthesis), 256, 1024 at L = 3000 and 2048 at L = 5000 (the largest footprint); three rows
a case with nf mod 16 in {15, 0, 1} where L allows; one case with n_out mod 13 in {12, 0, 1}, 13 being the hop segments a workgroup of
pv_synthesis_kernel owns.  Rates at nfft 64: 1.0, 0.8, 1.25, 0.5 (a_t exactly 0 or 0.5), 1.7 (products that do not floor as the real number
does), 3.7 (frames skipped), 0.125 and 8.0 (the limits).

Observed on the MI355X (printed by every case; the gates stay as they are): counts and out_len equal throughout; d_stretch at most 3.3e-12 of the
largest |Y| from the longdouble restatement (nfft 256, rate 0.8; 1.3e-12 at nfft 64 / rate 0.125, 1.9e-13 at nfft 2048), the float64 restatement's own
distance from it; d_y beyond its float32 rounding 0 in every case; the worst input condition 3.3e-12.

Times: not gated here (tools/phase_vocoder_bench.py).
"""
import numpy as np
import pytest
import torch

import analysis_gpu as A
import phase_vocoder_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import _stream_ptr

pytestmark = pytest.mark.gpu

_REF = {}
NAMES = ("y", "out_len", "counts", "stretch")
BEHIND = 50.0


def load(eng, nfft, null=(), window=None, tw=None):
    w = np.ascontiguousarray(R.window(nfft) if window is None else window, dtype=np.float64)
    t = np.ascontiguousarray(R.twiddle(nfft) if tw is None else tw, dtype=np.float64)
    return eng.lib.ev_load_phase_vocoder(eng.h, None if "window" in null else w.ctypes.data, None if "twiddle" in null else t.ctypes.data, nfft)


@pytest.fixture(scope="module")
def engines():
    yield from A.engines_on_demand(lambda nfft: A.engine_with(load, nfft))


def raw(eng, x, lens, rate, nfft, B=None, L=None, L_out=None, null=()):
    """ev_phase_vocoder into guarded buffers -> (rc, {"y", "out_len", "counts", "stretch"} on the host; None where passed as NULL)."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    Lo, _, NO = R.out_shape(Lx, rate, nfft) if np.isfinite(rate) and rate > 0 else (Lx, 0, 1)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"y": ((Bx, Lo), torch.float32), "out_len": ((Bx,), torch.int32), "counts": ((Bx, 2), torch.int32),
                     "stretch": ((Bx, NO, nfft // 2 + 1, 2), torch.float64)}, tuple(n for n in null if n in NAMES))
    rc = eng.lib.ev_phase_vocoder(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(), Bx if B is None else B,
                                  Lx if L is None else L, float(rate), out.ptr("y"), Lo if L_out is None else L_out, out.ptr("out_len"),
                                  out.ptr("counts"), out.ptr("stretch"), _stream_ptr())
    return rc, out.collect(rc)


def reference(key, x, lens, rate, nfft):
    """(float64, longdouble) restatements of a case, computed once."""
    return A.frozen(_REF, key, lambda: (R.stretch(x, lens, rate, nfft), R.stretch(x, lens, rate, nfft, np.longdouble)))


def cabs(a):
    return np.hypot(a[..., 0], a[..., 1])


def check(dev, refs, what):
    """The five-part rule of the module docstring, per row; prints the worst figures before it asserts."""
    r64, rld = refs
    B = rld["y"].shape[0]
    worst = {"in_Y": 0.0, "in_y": 0.0, "Y": 0.0, "y": 0.0}
    fails = []
    if dev["counts"] is not None and not np.array_equal(dev["counts"], rld["counts"]):
        fails.append(f"d_counts {dev['counts'].tolist()} != {rld['counts'].tolist()}")
    if not np.array_equal(dev["out_len"], rld["out_len"]):
        fails.append(f"d_out_len {dev['out_len'].tolist()} != {rld['out_len'].tolist()}")
    for b in range(B):
        n_out, out_len = int(rld["counts"][b, 1]), int(rld["out_len"][b])
        ymax = float(cabs(rld["stretch"][b]).max()) if n_out else 0.0
        peak = float(np.abs(rld["y"][b]).max())
        if ymax > 0:
            worst["in_Y"] = max(worst["in_Y"], float(cabs(r64["stretch"][b] - rld["stretch"][b]).max()) / ymax)
        if peak > 0:
            worst["in_y"] = max(worst["in_y"], float(np.abs(r64["y"][b] - rld["y"][b]).max()) / peak)
        if dev["stretch"] is not None:
            if ymax > 0:
                worst["Y"] = max(worst["Y"], float(cabs(dev["stretch"][b].astype(np.longdouble) - rld["stretch"][b]).max()) / ymax)
            if np.any(dev["stretch"][b, n_out:] != 0):
                fails.append(f"row {b}: d_stretch is not zero behind n_out = {n_out}")
        d = np.abs(dev["y"][b].astype(np.longdouble) - rld["y"][b])
        over = d - 2.0 ** -24 * np.abs(rld["y"][b])
        if peak > 0:
            worst["y"] = max(worst["y"], float(over.max()) / peak)
        elif np.any(dev["y"][b] != 0):
            fails.append(f"row {b}: d_y of a silent or empty row is not zero")
        if np.any(dev["y"][b, out_len:] != 0):
            fails.append(f"row {b}: d_y is not zero behind out_len = {out_len}")
    print(f"\nphase vocoder {what}: input condition Y {worst['in_Y']:.3e} y {worst['in_y']:.3e} (gate {R.INPUT_TOL:g});  device Y {worst['Y']:.3e}  "
          f"y beyond the fp32 rounding {worst['y']:.3e} (gate {R.TOL:g});  counts {rld['counts'].tolist()} out_len {rld['out_len'].tolist()}")
    assert worst["in_Y"] <= R.INPUT_TOL and worst["in_y"] <= R.INPUT_TOL, f"{what}: the input is ill-conditioned"
    assert not fails, f"{what}: " + "; ".join(fails)
    assert worst["Y"] <= R.TOL, f"{what}: d_stretch"
    assert worst["y"] <= R.TOL, f"{what}: d_y"


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
def case(name):
    """-> (nfft, rate, x (B, L) with 50.0 behind the rows, lens)."""
    kind, nfft, rate = name
    if kind == "frames":                                                 # nf mod 16 in {15, 0, 1}
        lens = R.lens_for(nfft, 17)
        L = max(lens) + 3
    elif kind == "long":                                                 # the issue's L at the two large geometries: a full row, a shorter one, one frame
        L = {1024: 3000, 2048: 5000}[nfft]
        lens = [L, L - nfft // 4 + 61, nfft // 4 - 56]
    elif kind == "synth":                                                # n_out mod 13 in {12, 0, 1} at rate 1 (n_out = nf)
        lens = R.lens_for(nfft, 20, (12, 0, 1), R.SYNTH_OWNED)
        L = max(lens) + 3
    else:
        raise KeyError(name)
    return nfft, rate, R.batch(lens, L, "speech" if nfft != 256 else "noise", seed=nfft, behind=BEHIND), lens


CASES = [("frames", 16, 0.8), ("frames", 16, 1.25)] + [("frames", 64, r) for r in R.RATES_64] + [("frames", 256, 0.8), ("frames", 256, 1.25)] \
    + [("long", 1024, 0.8), ("long", 1024, 1.25), ("long", 2048, 0.8), ("long", 2048, 1.25), ("synth", 64, 1.0)]


@pytest.mark.parametrize("name", CASES, ids=lambda n: f"{n[0]}-{n[1]}-{n[2]}")
def test_against_the_restatement(engines, name):
    nfft, rate, x, lens = case(name)
    rc, dev = raw(engines(nfft), x, lens, rate, nfft)
    assert rc == 0, err_of(engines(nfft))
    check(dev, reference(name, x, lens, rate, nfft), f"{name}")


def test_rate_one_returns_the_input(engines):
    nfft, rate, x, lens = case(("frames", 64, 1.0))
    rc, dev = raw(engines(nfft), x, lens, rate, nfft)
    assert rc == 0
    for b, n in enumerate(lens):
        e = float(np.abs(dev["y"][b, :n].astype(np.float64) - x[b, :n]).max()) / float(np.abs(x[b, :n]).max())
        print(f"\nrate 1.0 row {b}: |y - x| / peak {e:.3e}")
        assert e <= 2.0 ** -23 and dev["out_len"][b] == n


# ---- rows: alone, in a batch, as a prefix, twice ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,rate", [(64, 0.8), (64, 1.7), (256, 1.25)])
def test_a_row_gives_the_same_bits_however_it_is_run(engines, nfft, rate):
    eng = engines(nfft)
    lens = R.lens_for(nfft, 17)
    L = max(lens) + 3
    x = R.batch(lens, L, "speech", seed=7, behind=BEHIND)
    rc, whole = raw(eng, x, lens, rate, nfft)
    rc2, again = raw(eng, x, lens, rate, nfft)
    assert rc == 0 and rc2 == 0
    assert all(np.array_equal(whole[k], again[k]) for k in NAMES), "a second call"
    for b, n in enumerate(lens):
        rc, alone = raw(eng, x[b:b + 1, :n], None, rate, nfft)                                  # the row alone at L = its length
        assert rc == 0
        longer = np.full((1, L + 2 * nfft + 5), -BEHIND, np.float32)                            # the prefix of a longer row, other things behind it
        longer[0, :n] = x[b, :n]
        rc, pre = raw(eng, longer, [n], rate, nfft)
        assert rc == 0
        for got, how in ((alone, "alone"), (pre, "as a prefix")):
            n_out, out_len = int(whole["counts"][b, 1]), int(whole["out_len"][b])
            assert np.array_equal(got["counts"][0], whole["counts"][b]) and got["out_len"][0] == out_len, how
            assert np.array_equal(got["stretch"][0, :n_out], whole["stretch"][b, :n_out]), f"row {b} {how}: d_stretch"
            assert not np.any(got["stretch"][0, n_out:]), how
            m = min(got["y"].shape[1], whole["y"].shape[1])
            assert m >= out_len and np.array_equal(got["y"][0, :m], whole["y"][b, :m]) and not np.any(got["y"][0, m:]), f"row {b} {how}: d_y"


def test_short_empty_and_oversized_rows(engines):
    nfft, rate = 64, 0.8
    L = 100
    x = R.batch([1, 0, L + 1, 37], L, "noise", seed=3, behind=BEHIND)
    x[2] = R.noise(L, 5)
    lens = [1, 0, L + 1, 37]
    rc, dev = raw(engines(nfft), x, lens, rate, nfft)
    assert rc == 0
    check(dev, reference("short", x, lens, rate, nfft), "one sample, len 0, len > L, 37 samples")
    assert dev["counts"].tolist()[0] == [1, 2] and dev["out_len"][0] == 1 and dev["y"][0, 0] != 0
    for b in (1, 2):
        assert not dev["y"][b].any() and not dev["stretch"][b].any() and dev["out_len"][b] == 0 and dev["counts"][b].tolist() == [0, 0]


def test_optional_outputs_as_null(engines):
    nfft, rate, x, lens = case(("frames", 64, 1.25))
    eng = engines(nfft)
    rc, full = raw(eng, x, lens, rate, nfft)
    assert rc == 0
    for null in (("counts",), ("stretch",), ("counts", "stretch")):
        rc, part = raw(eng, x, lens, rate, nfft, null=null)
        assert rc == 0, err_of(eng)
        for k in NAMES:
            assert (part[k] is None) if k in null else np.array_equal(part[k], full[k]), (null, k)
    rc, no_len = raw(eng, x[:, :lens[2]], None, rate, nfft)
    assert rc == 0 and no_len["out_len"].tolist() == [R.out_len_of(lens[2], rate)] * 3


# ---- limits -------------------------------------------------------------------------------------------------------------------------------------
BAD_CALLS = [
    (dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(L=0), "L=0"), (dict(rate=0.1249), "rate="), (dict(rate=8.001), "rate="),
    (dict(rate=float("nan")), "rate="), (dict(rate=float("inf")), "rate="), (dict(L_out=1), "L_out=1"), (dict(null=("x",)), "d_x"),
    (dict(null=("y",)), "d_y"), (dict(null=("out_len",)), "d_out_len"),
]


@pytest.mark.parametrize("over,word", BAD_CALLS, ids=[w + str(i) for i, (_, w) in enumerate(BAD_CALLS)])
def test_every_limit_of_the_call_names_itself_and_writes_nothing(engines, over, word):
    eng = engines(64)
    over = dict(over)
    x = R.batch([200, 150], 200, "noise", seed=1)
    rc, res = raw(eng, x, [200, 150], over.pop("rate", 0.8), 64, **over)
    msg = err_of(eng)
    assert rc != 0 and "ev_phase_vocoder" in msg and word in msg, msg
    assert all(v is None for v in res.values())


def test_scratch_over_four_gib_names_the_figure(engines):
    eng = engines(2048)
    x = torch.zeros((2, 8), dtype=torch.float32, device=DEV)                                    # (never read: the call fails on its arguments)
    B, L, rate = 60000, 40000, 0.125
    rc = eng.lib.ev_phase_vocoder(eng.h, x.data_ptr(), None, B, L, rate, x.data_ptr(), 320000, x.data_ptr(), None, None, _stream_ptr())
    msg = err_of(eng)
    need = 8 * B * 1025 * (2 * (1 + L // 512) + 2 * int(np.ceil((1 + L // 512) / rate)))
    assert rc != 0 and "4 GiB" in msg and str(need) in msg, msg
    assert audio.phase_vocoder_scratch_bytes(B, L, rate, 2048) == need


def test_a_call_before_a_load_fails():
    eng = A.engine_with()
    try:
        rc, res = raw(eng, R.batch([100], 100, "noise"), None, 0.8, 64)
        assert rc != 0 and "not loaded" in err_of(eng) and all(v is None for v in res.values())
    finally:
        eng.close()


BAD_LOADS = [(dict(nfft=8), "nfft=8"), (dict(nfft=2064), "nfft=2064"), (dict(nfft=72), "nfft=72"), (dict(null=("window",)), "non-null"),
             (dict(null=("twiddle",)), "non-null"), (dict(bad="window"), "window[3]"), (dict(bad="twiddle"), "twiddle[3]")]


@pytest.mark.parametrize("over,word", BAD_LOADS, ids=[w + str(i) for i, (_, w) in enumerate(BAD_LOADS)])
def test_every_limit_of_the_load_names_itself_and_keeps_the_tables(over, word):
    eng = A.engine_with(load, 64)
    try:
        x = R.batch([200], 200, "noise", seed=2)
        _, before = raw(eng, x, None, 0.8, 64)
        nfft = over.get("nfft", 64)
        w, tw = R.window(max(nfft, 16)), R.twiddle(max(nfft, 16))
        if over.get("bad") == "window":
            w[3] = np.nan
        if over.get("bad") == "twiddle":
            tw.reshape(-1)[3] = np.inf
        rc = load(eng, nfft, over.get("null", ()), w, tw)
        msg = err_of(eng)
        assert rc != 0 and "ev_load_phase_vocoder" in msg and word in msg, msg
        rc, after = raw(eng, x, None, 0.8, 64)
        assert rc == 0 and all(np.array_equal(before[k], after[k]) for k in NAMES)
    finally:
        eng.close()


def test_a_second_call_allocates_nothing_and_a_reload_replaces_the_tables():
    eng = A.engine_with(load, 64)
    try:
        x = R.batch([300, 200], 300, "noise", seed=4)
        n0 = eng.alloc_count()
        rc, a = raw(eng, x, [300, 200], 0.8, 64)
        n1 = eng.alloc_count()
        rc2, b = raw(eng, x, [300, 200], 0.8, 64)
        assert rc == 0 and rc2 == 0 and n1 > n0 and eng.alloc_count() == n1, "a second call at the same shape allocates nothing"
        assert load(eng, 16) == 0 and eng.alloc_count() == n1 + 1
        rc, c = raw(eng, x, [300, 200], 0.8, 16)
        assert rc == 0 and c["counts"].tolist() == [[76, 95], [51, 64]]
    finally:
        eng.close()


def test_the_call_is_capturable_once_the_arena_has_its_size():
    nfft, rate, x, lens = case(("frames", 64, 0.8))
    eng = A.engine_with()
    eng.load_phase_vocoder(R.window(nfft), R.twiddle(nfft), nfft)
    xd, ld = torch.as_tensor(x).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)   # (lengths on the device: no copy under capture)
    ref = eng.phase_vocoder(xd, ld, rate, True, True)
    torch.cuda.synchronize()
    n0 = eng.alloc_count()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        eng.phase_vocoder(xd, ld, rate, True, True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = eng.phase_vocoder(xd, ld, rate, True, True)
        for o in out:
            o.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b), "the replay equals the eager call"
    assert eng.alloc_count() == n0
    eng.close()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------
def test_time_stretch_matches_the_raw_call(engines):
    nfft, rate, x, lens = case(("frames", 64, 0.8))
    rc, dev = raw(engines(nfft), x, lens, rate, nfft)
    assert rc == 0
    y, out = audio.time_stretch(torch.as_tensor(x).to(DEV), rate, lens, n_fft=nfft)
    assert np.array_equal(y.cpu().numpy(), dev["y"]) and out.tolist() == dev["out_len"].tolist() and out.dtype == torch.int64
    y1, out1 = audio.time_stretch(torch.as_tensor(x[0, :lens[0]]).to(DEV), rate, n_fft=nfft)     # 1-D: B = 1
    assert y1.shape == (1, out1[0]) and np.array_equal(y1[0].cpu().numpy(), dev["y"][0, :out1[0]])


def test_time_stretch_splits_a_batch_over_the_scratch_limit(engines, monkeypatch):
    nfft, rate, x, lens = case(("frames", 64, 0.8))
    xd = torch.as_tensor(x).to(DEV)
    whole = audio.time_stretch(xd, rate, lens, n_fft=nfft)
    monkeypatch.setattr(audio, "PHASE_VOCODER_SCRATCH_BYTES", 2 * audio.phase_vocoder_scratch_bytes(1, x.shape[1], rate, nfft))   # groups of two rows
    split = audio.time_stretch(xd, rate, lens, n_fft=nfft)
    assert torch.equal(whole[0], split[0]) and torch.equal(whole[1], split[1])


def test_pitch_shift_moves_the_median_f0_by_the_realised_cents():
    sr, f0, n = 22050, 150.0, 22050
    t = np.arange(n) / sr
    rng = np.random.default_rng(0)
    x = sum(np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 11)) + 0.01 * rng.standard_normal(n)
    x = torch.as_tensor((0.5 * x / np.abs(x).max()).astype(np.float32)).to(DEV)[None, :]
    y, cents = audio.pitch_shift(x, 2, sr)
    assert y.shape == x.shape and abs(cents - 200.0) < 0.1

    def median_f0(sig):
        p = audio.pitch_yin(sig, sr)
        f, v = p["f0"][0], p["voiced"][0].bool()
        return float(f[v].median())
    a, b = median_f0(x), median_f0(y)
    moved = 1200.0 * np.log2(b / a)
    print(f"\npitch_shift(+2): median f0 {a:.2f} -> {b:.2f} Hz: {moved:.2f} cents against {cents:.2f} realised")
    assert abs(moved - cents) <= 20.0
    same, zero = audio.pitch_shift(x, 0, sr)
    assert zero == 0.0 and torch.equal(same, x) and same.data_ptr() != x.data_ptr()
