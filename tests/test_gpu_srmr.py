"""ev_srmr on the MI355X, through the C ABI.

Yardstick: tests/srmr_ref.py, the numpy float64 restatement with the header's chunks, carries and orders.  The device writes fmas where the
header does and numpy rounds those products first, so the two differ by float64 rounding carried through band filters whose poles sit within
4e-4 of the unit circle (4 Hz at 16 kHz).  The rule of every comparison (``check``):
  * d_frame, d_mean and d_srmr by test_gpu_loudness.py's rule: relative to max(|ref|, 1e-9 x the output's largest |ref| in the row), within
    ``R.gpu_gate(case)`` = max(1e-9, 16 x the restatement's own distance from its longdouble plain form on that case);
  * each case first asserts that every cumulative share of the restatement is at least 1e-6 away from 0.9; then d_counts must be EQUAL.
Geometry H = 64, W = 256 (tables designed for 1 kHz) except the case "big": the default tables, H = 1024, 23 x 8, B = 2, 1.6 s at 16 kHz.
Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py).  Inputs carry NaN behind each row's length.

Observed on the MI355X (printed by every case; the gates stay as they are): at H = 64 the worst relative error of any case is 1.2e-12 (d_frame
of (1, 32, 5)) against the gate 1e-9; on "big" d_frame is 2.2e-10 from the restatement, which itself stands 1.8e-10 from longdouble there: gate
2.9e-9.  The least share margin of any case is 2.7e-3.  The mutants lie 34 (no carry), 4.5 (quarter), 1.0 (no gain), 0.33 (share on >=, the
exact tie) and 6.8e8 (K* unclamped: a ratio of 0 against 29.3) from the device.

Times: not gated here (tools/srmr_bench.py).
"""
import numpy as np
import pytest
import torch

import analysis_gpu as A
import srmr_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd._lib import _stream_ptr

pytestmark = pytest.mark.gpu

_REF = {}
F64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)


def load(eng, tab, N=None, K=None, H=None, null=(), **over):
    """ev_load_srmr with the tables of ``tab``; ``over`` replaces tables, N / K / H the sizes passed, ``null`` names pointers passed as NULL."""
    t = {k: F64(over.get(k, tab[k])) for k in ("chan", "mod", "window", "erb", "cutoff")}
    p = lambda k: None if k in null else t[k].ctypes.data
    return eng.lib.ev_load_srmr(eng.h, p("chan"), p("mod"), p("window"), p("erb"), p("cutoff"), tab["chan"].shape[0] if N is None else N,
                                tab["mod"].shape[0] if K is None else K, tab["hop"] if H is None else H)


def raw(eng, x, lens, tab, want_frame=True, B=None, L=None, null=()):
    """ev_srmr into guarded buffers -> (rc, {"frame", "mean", "srmr", "counts"} on the host; frame None when not asked for).  ``B`` / ``L``
    override the shape passed to the library, ``null`` names pointers passed as NULL (the argument tests)."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    N, K, H = tab["chan"].shape[0], tab["mod"].shape[0], tab["hop"]
    NF = (Lx - 4 * H) // H + 1 if Lx >= 4 * H else 0
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"frame": ((Bx, NF, N, K), torch.float64), "mean": ((Bx, N, K), torch.float64), "srmr": ((Bx, 2), torch.float64),
                     "counts": ((Bx, 3), torch.int32)}, tuple(null) + (() if want_frame else ("frame",)))
    rc = eng.lib.ev_srmr(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, out.ptr("frame"),
                         out.ptr("mean"), out.ptr("srmr"), out.ptr("counts"), _stream_ptr())
    return rc, out.collect(rc)


def same_bits(a, b, names=("frame", "mean", "srmr", "counts")):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in names)


def check(dev, ref, gate, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    margin = float(ref["margin"].min())
    err = {k: R.rel_err(dev[k], ref[k]) for k in R.FLOAT_OUTPUTS}
    print(f"\nSRMR {what}: rel err frame {err['frame']:.3e} mean {err['mean']:.3e} srmr {err['srmr']:.3e} (gate {gate:.3e})  counts "
          f"{dev['counts'].tolist()}  least share margin {margin:.3e}  ratio {dev['srmr'][:, 0].tolist()}")
    assert margin >= 1e-6, f"{what}: a cumulative share of the reference lies {margin:.3e} from 0.9"
    assert np.array_equal(dev["counts"], ref["counts"]), f"{what}: d_counts {dev['counts'].tolist()} against {ref['counts'].tolist()}"
    for k in R.FLOAT_OUTPUTS:
        assert err[k] <= gate, f"{what}: d_{k}"


@pytest.fixture(scope="module")
def engines():
    def make(name):
        tab = {"tie": lambda: R.tie_case()[2], "kstar": lambda: R.kstar_case()[2]}.get(name, lambda: R.case(name)[2])()
        return A.engine_with(load, tab)
    yield from A.engines_on_demand(make)


# ---- 1. the cases: every (B, N, K), every length, the long geometry ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_case_against_the_restatement(engines, name):
    x, lens, tab = R.case(name)
    K = tab["mod"].shape[0]
    ref = A.frozen(_REF, name, lambda: R.srmr(x, lens, tab))
    rc, dev = raw(engines(name), x, lens, tab)
    assert rc == 0, err_of(engines(name))
    check(dev, ref, R.gpu_gate(name), f"{name} x {x.shape} lens {lens}")
    for b, n in enumerate(lens):
        nf = R.frames_of(n, x.shape[1], tab["hop"])
        assert dev["counts"][b, 0] == nf and not dev["frame"][b, nf:].any(), "zeros past the row's own frames"
        if nf == 0:
            assert not any(dev[k][b].any() for k in dev), "len < W, len 0 and len > L are rows of zeros"
    if K <= 4:
        assert not dev["srmr"][:, 0].any(), "K <= 4: no high band, ratio 0"
    else:
        assert all(dev["srmr"][b, 0] > 0 for b, n in enumerate(lens) if R.frames_of(n, x.shape[1], tab["hop"]) > 0)
    rc, lean = raw(engines(name), x, lens, tab, want_frame=False)
    assert rc == 0 and lean["frame"] is None and same_bits(dev, lean, ("mean", "srmr", "counts")), "without d_frame: the same bits"


def test_lengths_case_has_the_frames_the_header_counts(engines):
    x, lens, tab = R.case("lengths")
    assert A.frozen(_REF, "lengths", lambda: R.srmr(x, lens, tab))["counts"][:, 0].tolist() == [0, 1, 1, 1, 2, 2, 37, 0, 0]


# ---- 2. the identities: bit-equal outputs --------------------------------------------------------------------------------------------------------
def test_row_alone_in_a_batch_as_a_prefix_twice_and_under_every_arithmetic(engines):
    name = "shape-2-23-8"
    eng, tab = engines(name), R.case(name)[2]
    H = tab["hop"]
    row = R.voice(21 * H + 5, 1000, seed=77)
    nf = 18
    rc, alone = raw(eng, row[None], None, tab)
    assert rc == 0 and alone["counts"][0, 0] == nf, err_of(eng)
    n0 = eng.alloc_count()
    rc, again = raw(eng, row[None], None, tab)
    assert rc == 0 and same_bits(alone, again) and eng.alloc_count() == n0, "a second call: the same bits, no allocation"
    xb, lb = R.padded([R.voice(30 * H, 1000, seed=78), row, R.voice(7 * H + 1, 1000, seed=79)])
    rc, batch = raw(eng, xb, lb, tab)
    assert rc == 0
    xp, lp = R.padded([R.voice(5 * H, 1000, seed=80), row], L=len(row) + 1234)
    rc, prefix = raw(eng, xp, lp, tab)
    assert rc == 0 and np.isnan(xp[1, len(row):]).all(), "NaN behind the row"
    for got, what in ((batch, "inside a batch"), (prefix, "the prefix of a longer row with NaN behind it")):
        assert np.array_equal(alone["frame"][0], got["frame"][1, :nf]) and not got["frame"][1, nf:].any(), f"d_frame: alone against {what}"
        assert all(np.array_equal(alone[k][0], got[k][1]) for k in ("mean", "srmr", "counts")), f"alone against {what}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 6, 16):
            eng.set_arithmetic(setting)
            rc, got = raw(eng, xb, lb, tab)
            assert rc == 0 and same_bits(got, batch), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


def test_a_captured_graph_replays_the_eager_bits(engines):
    name = "shape-2-23-8"
    x, lens, tab = R.case(name)
    rc, raw_out = raw(engines(name), x, lens, tab)
    assert rc == 0
    eng = A.engine_with()                                                # (loaded and called through Engine.load_srmr / Engine.srmr, the bindings)
    try:
        eng.load_srmr(tab["chan"], tab["mod"], tab["window"], tab["erb"], tab["cutoff"], tab["hop"])
        xd, ld = torch.from_numpy(x).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
        ref = eng.srmr(xd, ld, want_frame=True)
        torch.cuda.synchronize()
        n0 = eng.alloc_count()
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            eng.srmr(xd, ld, want_frame=True)
            torch.cuda.synchronize()
            assert eng.alloc_count() == n0, "the arena has its size"
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = eng.srmr(xd, ld, want_frame=True)
            for t in out:
                t.fill_(-5)
            graph.replay()
            torch.cuda.synchronize()
        for a, b, k in zip(out, ref, ("frame", "mean", "srmr", "counts")):
            assert torch.equal(a, b), "the replay equals the eager call"
            assert np.array_equal(a.cpu().numpy(), raw_out[k]), "and the raw call on another handle"
    finally:
        eng.close()


# ---- 3. a second load replaces the first -----------------------------------------------------------------------------------------------------
def test_a_second_load_replaces_the_first():
    xa, la, ta = R.case("shape-3-3-8")
    xb, lb, tb = R.case("shape-1-32-5")
    eng = A.engine_with(load, ta)
    try:
        assert load(eng, tb) == 0, err_of(eng)
        rc, dev = raw(eng, xb, lb, tb)
        assert rc == 0, err_of(eng)
        check(dev, A.frozen(_REF, "shape-1-32-5", lambda: R.srmr(xb, lb, tb)), R.gpu_gate("shape-1-32-5"), "after a second load")
    finally:
        eng.close()


# ---- 4. mutants of the restatement: the device must disagree with each, past 1e-6 ----------------------------------------------------------------
MUTANT_CASE = {"no_carry": "shape-2-23-8", "quarter": "shape-2-23-8", "no_gain": "shape-2-23-8", "share_ge": "tie", "kstar_unclamped": "kstar"}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_device_disagrees_with_each_mutant(engines, mutant):
    name = MUTANT_CASE[mutant]
    x, lens, tab = {"tie": R.tie_case, "kstar": R.kstar_case}.get(name, lambda: R.case(name))()
    ref = A.frozen(_REF, name, lambda: R.srmr(x, lens, tab))
    wrong = R.srmr(x, lens, tab, mutant)
    rc, dev = raw(engines(name), x, lens, tab)
    assert rc == 0, err_of(engines(name))
    if name == "tie":                                                    # (exact by construction: the share IS 0.9, so no margin is asked)
        assert ref["margin"][0] == 0.0 and all(np.array_equal(dev[k], ref[k]) for k in dev), "the tie case is exact on both sides"
    else:
        check(dev, ref, 1e-9, f"{name} (the case of mutant {mutant})")
    far = max(R.rel_err(dev[k], wrong[k]) for k in R.FLOAT_OUTPUTS)
    print(f"\nSRMR mutant {mutant} on {name}: the device is {far:.3e} from it")
    assert far > 1e-6, f"the device agrees with the mutant {mutant}"


# ---- 5. limits -----------------------------------------------------------------------------------------------------------------------------------
T0 = R.tables(n_channels=3, n_bands=8)
UNSTABLE = T0["mod"].copy()
UNSTABLE[2, 3:] = (-2.1, 1.05)
NAN_WIN = T0["window"].copy()
NAN_WIN[5] = np.nan
POLE = T0["chan"].copy()
POLE[1, :2] = (0.8, 0.6)
BAD_LOADS = [
    ("N=", dict(N=0)), ("N=", dict(N=33)), ("K=", dict(K=0)), ("K=", dict(K=9)), ("H=", dict(H=32)), ("H=", dict(H=96)), ("H=", dict(H=1088)),
    ("non-null", dict(null=("chan",))), ("non-null", dict(null=("cutoff",))), ("mod band 2", dict(mod=UNSTABLE)), ("window[5]", dict(window=NAN_WIN)),
    ("chan[1]", dict(chan=POLE)),
]
BAD_CALLS = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("L=", dict(L=0)), ("d_x", dict(null=("x",))), ("d_mean", dict(null=("mean",))),
    ("d_srmr", dict(null=("srmr",))), ("d_counts", dict(null=("counts",))),
]


@pytest.mark.parametrize("word,kw", BAD_LOADS, ids=[f"{w.strip('=').replace(' ', '')}-{i}" for i, (w, _) in enumerate(BAD_LOADS)])
def test_each_limit_of_the_load_fails_with_a_message_naming_it(word, kw):
    big = dict(T0, window=np.concatenate([T0["window"]] * 5))            # (room for any H the call names)
    eng = A.engine_with()
    try:
        n0 = eng.alloc_count()
        rc = load(eng, big, **kw)
        msg = err_of(eng)
        assert rc != 0 and "ev_load_srmr" in msg and word in msg, msg
        assert eng.alloc_count() == n0
        rc, _ = raw(eng, np.zeros((1, 512), np.float32), None, T0)
        assert rc != 0 and "not loaded" in err_of(eng), "a failed load loads nothing"
    finally:
        eng.close()


@pytest.mark.parametrize("word,kw", BAD_CALLS, ids=[f"{w.strip('=')}-{i}" for i, (w, _) in enumerate(BAD_CALLS)])
def test_each_limit_of_the_call_fails_with_a_message_naming_it(engines, word, kw):
    eng = engines("shape-3-3-8")
    n0 = eng.alloc_count()
    rc, _ = raw(eng, np.zeros((2, 1024), np.float32), None, T0, **kw)    # (a failed call writes nothing, margins intact: raw checks that)
    msg = err_of(eng)
    assert rc != 0 and "ev_srmr" in msg and word in msg, msg
    assert eng.alloc_count() == n0, "a failed call leaves ev_alloc_count unmoved"


def test_a_call_before_any_load_fails():
    eng = A.engine_with()
    try:
        rc, _ = raw(eng, np.zeros((1, 512), np.float32), None, T0)
        assert rc != 0 and "ev_load_srmr" in err_of(eng)
    finally:
        eng.close()


# ---- 6. the host layer on the device -------------------------------------------------------------------------------------------------------------
def test_audio_srmr_resamples_and_matches_the_restatement():
    from emojivoice_amd import audio

    y = torch.from_numpy(np.stack([R.voice(22050, 22050, seed=3, f0=120.0), R.voice(22050, 22050, seed=4, f0=200.0)])).to(DEV)
    lens = [22050, 4000]                                                 # 1 s, and 181 ms: under a frame
    out = audio.srmr(y, 22050, lengths=lens, energies=True)
    x16 = audio.resample(y, 22050, 16000, lengths=torch.tensor(lens)).cpu().numpy()
    ref = R.srmr(x16, [16000, -(-4000 * 320 // 441)], audio.srmr_tables())
    got = {"mean": out["mean"].cpu().numpy(), "frame": out["energies"].cpu().numpy(),
           "srmr": np.stack([np.nan_to_num(out["srmr"].cpu().numpy()), out["bw"].cpu().numpy()], axis=1)}
    err = {k: R.rel_err(got[k], ref[k]) for k in R.FLOAT_OUTPUTS}
    print(f"\nSRMR audio.srmr 1 s at 22.05 kHz: rel err {err}  srmr {out['srmr'].tolist()}  K* {out['k_star'].tolist()}  frames {out['frames'].tolist()}")
    assert out["frames"].tolist() == ref["counts"][:, 0].tolist() == [12, 0] and out["k_star"].tolist() == ref["counts"][:, 2].tolist()
    assert max(err.values()) <= R.gpu_gate("big") and bool(torch.isnan(out["srmr"][1])) and float(out["srmr"][0]) > 0
    one = audio.srmr(y[0])
    assert one["srmr"].shape == (1,) and float(one["srmr"][0]) == float(out["srmr"][0]), "a 1-D input is the same row"


# ---- 7. the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_reverb_report_end_to_end(tmp_path):
    import json

    from emojivoice_amd import audio, cli

    takes = {"a.wav": ("7", R.voice(11025, 22050, seed=21, f0=110.0)), "b.wav": ("7", R.voice(16000, 22050, seed=22, f0=170.0)),
             "c.wav": ("12", R.voice(3000, 22050, seed=23))}             # c: 136 ms, under a frame
    for name, (_, y) in takes.items():
        cli.write_wav_pcm16(tmp_path / name, y, 22050)
    flist = tmp_path / "takes.txt"
    flist.write_text("".join(f"{name}|{spk}|text of {name}\n" for name, (spk, _) in takes.items()), encoding="utf-8")
    rep = cli.cli(["--reverb_report", str(flist), "--batch_size", "2"])
    with open(f"{flist}.srmr.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep)) and set(saved) == {"sample_rate", "srmr_sample_rate", "files", "speakers", "overall"}
    for f_, (name, (spk, _)) in zip(saved["files"], takes.items()):
        y = audio.load_audio(tmp_path / name, 22050, DEV)                # (what the 16-bit file holds)
        x16 = audio.resample(y, 22050, 16000).cpu().numpy()
        want = R.srmr(x16, None, audio.srmr_tables())
        assert f_["speaker"] == spk and f_["frames"] == int(want["counts"][0, 0]) and f_["k_star"] == int(want["counts"][0, 2])
        if want["counts"][0, 0] == 0:
            assert f_["srmr"] is None
        else:
            assert abs(f_["srmr"] - want["srmr"][0, 0]) <= R.gpu_gate("big") * want["srmr"][0, 0]
    assert [f_["frames"] for f_ in saved["files"]] == [4, 8, 0]
    assert saved["speakers"]["7"]["measured"] == 2 and saved["speakers"]["12"]["mean"] is None and saved["overall"]["files"] == 3
