"""ev_dtw on the MI355X, through the C ABI, and the evaluation report built on it.

Yardstick: tests/dtw_ref.py, the numpy float64 restatement of the header's semantics.  The device forms the local cost with one fma per
channel where numpy multiplies and adds, so the cost of a K-cell path may differ by about K 2^-53 ~ 1e-13 relative; the rule is
  * integer-valued inputs under metric 1: everything is exact in float64, cells tie all over the matrix, and cost, steps and path are
    EQUAL to the restatement;
  * Euclidean inputs: the restatement's path margin (dtw_ref: the least gap between the best and the second-best predecessor along the
    path, over the cost) is asserted >= 1e-9 first, four orders above that rounding; then steps and path are EQUAL and
    |cost - ref| <= 1e-9 ref.
Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py).  Inputs carry loud garbage behind each row's lengths.

Times: not gated here (tools/dtw_bench.py).
"""
import json
import math
import wave

import numpy as np
import pytest
import torch

import analysis_gpu as A
import dtw_ref as R
import pitch_ref as P
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, EvLibraryError, _stream_ptr

pytestmark = pytest.mark.gpu

GARBAGE = R.GARBAGE
_REF = {}


def ref_of(key, x, y, xl, yl, metric):
    """The restatement's result, computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: R.dtw(x, y, xl, yl, metric))


def raw(eng, x, y, xl=None, yl=None, metric=0, want_path=True):
    """ev_dtw into guarded buffers: (rc, cost (B,), steps (B,), path (B, Tx + Ty - 1, 2) or None) on the host."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    y = torch.as_tensor(y, dtype=torch.float32).to(DEV).contiguous()
    B, C, Tx = x.shape
    Ty = y.shape[2]
    NP = Tx + Ty - 1
    d_xl = None if xl is None else torch.tensor(xl, dtype=torch.int32, device=DEV)
    d_yl = None if yl is None else torch.tensor(yl, dtype=torch.int32, device=DEV)
    out = A.Guarded({"cost": ((B,), torch.float64), "steps": ((B,), torch.int32), "path": ((B, NP, 2), torch.int32)}, () if want_path else ("path",))
    rc = eng.lib.ev_dtw(eng.h, x.data_ptr(), y.data_ptr(), None if d_xl is None else d_xl.data_ptr(), None if d_yl is None else d_yl.data_ptr(),
                        B, C, Tx, Ty, metric, out.ptr("cost"), out.ptr("steps"), out.ptr("path"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def check_equal(dev, ref, what):
    cost, steps, path = dev
    print(f"\nDTW {what}: cost {cost} ref {ref['cost']} steps {steps} path mismatches {int((path != ref['path']).sum())} margin {ref['margin']}")
    assert np.array_equal(steps, ref["steps"]), f"{what}: d_steps"
    assert np.array_equal(path, ref["path"]), f"{what}: d_path"
    assert np.array_equal(cost, ref["cost"]), f"{what}: d_cost"


def check_close(dev, ref, what):
    cost, steps, path = dev
    rel = np.abs(cost - ref["cost"]) / np.where(ref["cost"] != 0, ref["cost"], 1.0)
    print(f"\nDTW {what}: cost rel err {rel} steps {steps} path mismatches {int((path != ref['path']).sum())} margin {ref['margin']}")
    assert np.all(ref["margin"] >= 1e-9), f"{what}: the reference's path margin is under 1e-9 (change the seed)"
    assert np.array_equal(steps, ref["steps"]), f"{what}: d_steps"
    assert np.array_equal(path, ref["path"]), f"{what}: d_path"
    assert np.all(np.abs(cost - ref["cost"]) <= 1e-9 * ref["cost"]), f"{what}: d_cost"


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


# ---- 1. exact, with ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Tx,Ty", R.EXACT_CASES, ids=[f"C{c}-{a}x{b}" for c, a, b in R.EXACT_CASES])
def test_integer_features_are_exact_ties_included(eng, C, Tx, Ty):
    x, y, xl, yl = R.exact_batch(C, Tx, Ty)
    ref = ref_of(("exact", C, Tx, Ty), x, y, xl, yl, 1)
    rc, *dev = raw(eng, x, y, xl, yl, 1)
    assert rc == 0, err_of(eng)
    check_equal(dev, ref, f"exact C{C} {Tx}x{Ty}")


# ---- 2. Euclidean parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Tx,Ty", R.EUCLID_CASES, ids=[f"C{c}-{a}x{b}" for c, a, b in R.EUCLID_CASES])
def test_euclidean_parity_with_the_restatement(eng, C, Tx, Ty):
    x, y, xl, yl = R.euclid_batch(C, Tx, Ty)
    ref = ref_of(("euclid", C, Tx, Ty), x, y, xl, yl, 0)
    assert np.all(ref["margin"] >= 1e-9), "the reference's path margin is under 1e-9 (change the seed)"
    rc, *dev = raw(eng, x, y, xl, yl, 0)
    assert rc == 0, err_of(eng)
    check_close(dev, ref, f"euclid C{C} {Tx}x{Ty}")
    for b in range(len(xl)):
        K = dev[1][b]
        assert max(xl[b], yl[b]) <= K <= xl[b] + yl[b] - 1 and np.all(dev[2][b, K:] == -1)


# ---- 3. warp recovery, known answer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_a_warp_is_recovered_exactly(eng, metric):
    g = np.random.default_rng(11)
    rows, want = [], []
    for tx, ty in ((40, 67), (9, 9), (130, 131)):
        xr = g.standard_normal((13, tx)).astype(np.float32)
        idx = R.covering_warp(tx, ty, seed=tx)
        rows.append((xr, xr[:, idx]))
        want.append(np.stack([idx, np.arange(ty)], axis=1))
    x, y, xl, yl = R.pad_batch(rows)
    rc, cost, steps, path = raw(eng, x, y, xl, yl, metric)
    assert rc == 0, err_of(eng)
    for b, w in enumerate(want):
        assert cost[b] == 0.0 and steps[b] == yl[b]
        assert np.array_equal(path[b, : yl[b]], w) and np.all(path[b, yl[b]:] == -1)


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tx,Ty", R.EDGE_CASES)
def test_edges(eng, Tx, Ty):
    x, y, xl, yl = R.edge_batch(Tx, Ty)
    ref = ref_of(("edge", Tx, Ty), x, y, xl, yl, 0)
    rc, *dev = raw(eng, x, y, xl, yl, 0)
    assert rc == 0, err_of(eng)
    check_close(dev, ref, f"edge {Tx}x{Ty}")


def test_the_limit_4096_by_4096(eng):
    x, y = R.limit_pair()
    ref = ref_of("limit", x, y, None, None, R.LIMIT_METRIC)
    assert ref["margin"][0] >= 1e-9, "the reference's path margin is under 1e-9 (change the seed)"
    rc, *dev = raw(eng, x, y, None, None, R.LIMIT_METRIC)
    assert rc == 0, err_of(eng)
    check_close(dev, ref, "limit 4096x4096")


# ---- 5. same bits ------------------------------------------------------------------------------------------------------------------------
def test_row_alone_in_a_batch_and_as_a_prefix_give_the_same_bits(eng):
    C, Tx, Ty = 13, 130, 97
    x, y, xl, yl = R.euclid_batch(C, Tx, Ty)
    b, tx, ty = 1, xl[1], yl[1]
    xa, ya = x[b:b + 1, :, :tx], y[b:b + 1, :, :ty]
    rc, *alone = raw(eng, xa, ya)
    assert rc == 0
    rc, *again = raw(eng, xa, ya)
    assert rc == 0 and all(np.array_equal(a, c) for a, c in zip(alone, again)), "two calls"
    rc, *batch = raw(eng, x, y, xl, yl)
    assert rc == 0
    xp = np.full((2, C, 1100), GARBAGE, np.float32)                       # Tx = 1100: two rows per thread, bits in the arena
    yp = np.full((2, C, 600), GARBAGE, np.float32)
    xp[1, :, :tx], yp[1, :, :ty] = xa[0], ya[0]
    xp[0, :, :300], yp[0, :, :200] = R.noisy_warp_pair(C, 300, 200, seed=5)
    rc, *prefix = raw(eng, xp, yp, [300, tx], [200, ty])
    assert rc == 0
    K = alone[1][0]
    assert alone[0][0] == batch[0][b] == prefix[0][1], "cost: alone, inside a batch, as a prefix"
    assert K == batch[1][b] == prefix[1][1]
    assert np.array_equal(alone[2][0, :K], batch[2][b, :K]) and np.array_equal(alone[2][0, :K], prefix[2][1, :K])
    assert np.all(batch[2][b, K:] == -1) and np.all(prefix[2][1, K:] == -1)
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 6, 16):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, x, y, xl, yl)
            assert rc == 0 and all(np.array_equal(a, c) for a, c in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


# ---- 6. bad rows and short rows ----------------------------------------------------------------------------------------------------------
def test_bad_rows_are_empty_and_short_rows_match(eng):
    C, Tx, Ty = 5, 40, 33
    gx, gy = R.noisy_warp_pair(C, Tx, Ty, seed=21)
    rc, *alone = raw(eng, gx[None], gy[None])
    assert rc == 0
    x = np.full((6, C, Tx), GARBAGE, np.float32)
    y = np.full((6, C, Ty), GARBAGE, np.float32)
    x[1], y[1] = gx, gy
    x[4], y[4] = gx, gy
    rc, cost, steps, path = raw(eng, x, y, [0, Tx, Tx + 1, 7, Tx, -2], [Ty, Ty, 5, Ty + 1, Ty, 0])
    assert rc == 0
    for b in (0, 2, 3, 5):
        assert cost[b] == 0.0 and steps[b] == 0 and np.all(path[b] == -1), "a bad row: cost 0, steps 0, a path of -1"
    for b in (1, 4):
        assert cost[b] == alone[0][0] and steps[b] == alone[1][0] and np.array_equal(path[b], alone[2][0]), "the good rows next to them"
    xs = np.full((3, C, Tx), GARBAGE, np.float32)
    ys = np.full((3, C, Ty), GARBAGE, np.float32)
    xs[0, :, :1], ys[0] = gx[:, :1], gy
    xs[1], ys[1, :, :1] = gx, gy[:, :1]
    xs[2, :, :1], ys[2, :, :1] = gx[:, 3:4], gy[:, 2:3]
    xl, yl = [1, Tx, 1], [Ty, 1, 1]
    ref = ref_of("short", xs, ys, xl, yl, 0)
    rc, *dev = raw(eng, xs, ys, xl, yl)
    assert rc == 0
    check_close(dev, ref, "xlen = 1 and ylen = 1")
    assert dev[1].tolist() == [Ty, Tx, 1]


# ---- 7. messages -------------------------------------------------------------------------------------------------------------------------
BAD_ARGS = [("B=", (0, 2, 4, 4), 0), ("B=", (65536, 1, 1, 1), 0), ("C=", (1, 0, 4, 4), 0), ("C=", (1, 129, 4, 4), 0), ("Tx=", (1, 2, 0, 4), 0),
            ("Tx=", (1, 1, 4097, 4), 0), ("Ty=", (1, 2, 4, 0), 0), ("Ty=", (1, 1, 4, 4097), 0), ("metric", (1, 2, 4, 4), 2), ("metric", (1, 2, 4, 4), -1)]


@pytest.mark.parametrize("word,shape,metric", BAD_ARGS, ids=[f"{w}-{i}" for i, (w, _, _) in enumerate(BAD_ARGS)])
def test_each_limit_fails_with_a_message_naming_it(eng, word, shape, metric):
    B, C, Tx, Ty = shape
    with pytest.raises(EvLibraryError, match=word):
        eng.dtw(torch.zeros(B, C, Tx, device=DEV), torch.zeros(B, C, Ty, device=DEV), metric=metric)


def test_null_outputs_fail_with_a_message(eng):
    x = torch.zeros(1, 2, 4, device=DEV)
    cost = torch.zeros(1, dtype=torch.float64, device=DEV)
    steps = torch.zeros(1, dtype=torch.int32, device=DEV)
    for c, s, word in ((None, steps.data_ptr(), "d_cost"), (cost.data_ptr(), None, "d_steps")):
        rc = eng.lib.ev_dtw(eng.h, x.data_ptr(), x.data_ptr(), None, None, 1, 2, 4, 4, 0, c, s, None, _stream_ptr())
        assert rc != 0 and word in err_of(eng)


# ---- 8. NULL path ------------------------------------------------------------------------------------------------------------------------
def test_null_path_gives_the_same_cost_and_steps_without_scratch():
    e = Engine(0)
    n0 = e.alloc_count()
    for C, Tx, Ty in ((13, 130, 97), (3, 1100, 600)):                    # (the second would need the arena for its bits)
        rows = [R.noisy_warp_pair(C, tx, ty, seed=tx) for tx, ty in ((Tx, Ty), (Tx - 30, Ty - 7))]
        x, y, xl, yl = R.pad_batch(rows, Tx, Ty)
        rc, cost0, steps0, none = raw(e, x, y, xl, yl, 0, want_path=False)
        assert rc == 0 and none is None
        assert e.alloc_count() == n0, "no path: no scratch"
        rc, cost, steps, _ = raw(e, x, y, xl, yl, 0)
        assert rc == 0 and np.array_equal(cost, cost0) and np.array_equal(steps, steps0)
    e.close()


# ---- 9. allocation and capture -----------------------------------------------------------------------------------------------------------
def test_second_call_allocates_nothing_and_capturable():
    e = Engine(0)
    C, Tx, Ty = 4, 1100, 700                                             # bits in the arena
    rows = [R.noisy_warp_pair(C, tx, ty, seed=tx) for tx, ty in ((Tx, Ty), (500, 650))]
    x, y, xl, yl = R.pad_batch(rows, Tx, Ty)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    n0 = e.alloc_count()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        ref = e.dtw(xd, yd, xl, yl)
        torch.cuda.synchronize()
        n1 = e.alloc_count()
        assert n1 == n0 + 1, "the arena of the decision bits is one allocation"
        again = e.dtw(xd, yd, xl, yl)
        small = e.dtw(xd[:, :, :64].contiguous(), yd[:, :, :50].contiguous())          # (bits in LDS)
        torch.cuda.synchronize()
        assert e.alloc_count() == n1, "a second call at the same shape allocates nothing"
        assert all(torch.equal(a, b) for a, b in zip(ref, again)) and int(small[1][0]) >= 64
        xl_d, yl_d = torch.tensor(xl, dtype=torch.int32, device=DEV), torch.tensor(yl, dtype=torch.int32, device=DEV)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = e.dtw(xd, yd, xl_d, yl_d)
        for t in out:
            t.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b), "the replay equals the eager call"
    assert e.alloc_count() == n1
    r = R.dtw(x, y, xl, yl, 0)
    assert np.all(r["margin"] >= 1e-9) and np.array_equal(ref[2].cpu().numpy(), r["path"]) and np.array_equal(ref[1].cpu().numpy(), r["steps"])
    e.close()


# ---- 10. host layer ----------------------------------------------------------------------------------------------------------------------
def test_mcd_of_a_mel_against_its_own_warp_is_zero():
    g = torch.Generator().manual_seed(2)
    mel = (torch.randn(2, 80, 50, generator=g) * 2 - 5).to(DEV)
    idx = torch.from_numpy(R.covering_warp(50, 77, seed=9)).to(DEV)
    mcd = audio.mel_cepstral_distortion(mel, mel[:, :, idx])
    assert mcd.dtype == torch.float64 and mcd.shape == (2,) and mcd.tolist() == [0.0, 0.0]
    out = audio.dtw(audio.mel_cepstrum(mel), audio.mel_cepstrum(mel[:, :, idx]))
    assert out["steps"].tolist() == [77, 77] and torch.equal(out["path"][0, :77, 0].long(), idx)
    mcd = audio.mel_cepstral_distortion(mel, mel[:, :, idx], len_a=[50, 20], len_b=[77, 31])
    assert float(mcd[0]) == 0.0 and float(mcd[1]) > 0.0


def test_mcd_of_a_one_frame_pair():
    g = torch.Generator().manual_seed(3)
    a, b = (torch.randn(1, 80, 1, generator=g) - 5).to(DEV), (torch.randn(1, 80, 1, generator=g) - 5).to(DEV)
    ca, cb = audio.mel_cepstrum(a).cpu().numpy().astype(np.float64), audio.mel_cepstrum(b).cpu().numpy().astype(np.float64)
    want = audio.MCD_DB * math.sqrt(float(((ca - cb) ** 2).sum()))
    got = float(audio.mel_cepstral_distortion(a, b)[0])
    print(f"\nDTW one-frame MCD {got} want {want}")
    assert abs(got - want) <= 1e-12 * want


# ---- 11. CLI -----------------------------------------------------------------------------------------------------------------------------
def write_wav16(path, y, sr=22050):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(y, -1, 1) * 32767.0).astype("<i2").tobytes())


def test_cli_evaluate_pairs(tmp_path):
    from emojivoice_amd.cli import cli

    write_wav16(tmp_path / "a.wav", P.harmonic_tone(150.0, 40 * 256 + 100))
    write_wav16(tmp_path / "b.wav", P.harmonic_tone(180.0, 52 * 256))
    write_wav16(tmp_path / "short.wav", P.harmonic_tone(150.0, 300))
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("a.wav|a.wav\na.wav|b.wav|7\nshort.wav|a.wav|7\n")
    cli(["--evaluate_pairs", str(pairs), "--batch_size", "2"])
    rep = json.loads((tmp_path / "pairs.txt.eval.json").read_text())
    same, diff = rep["pairs"]
    keys = {"mcd_db", "f0_rmse_cents", "voicing_error", "voiced_pairs", "frames_recorded", "frames_synthesised", "path_steps"}
    assert keys <= set(same) and keys <= set(diff)
    assert same["speaker"] == "0" and diff["speaker"] == "7"
    assert same["mcd_db"] == 0 and same["f0_rmse_cents"] == 0 and same["voicing_error"] == 0
    assert same["frames_recorded"] == same["frames_synthesised"] == same["path_steps"] == 40 and same["voiced_pairs"] > 0
    assert diff["frames_recorded"] == 40 and diff["frames_synthesised"] == 52 and 52 <= diff["path_steps"] <= 91
    assert math.isfinite(diff["mcd_db"]) and diff["mcd_db"] > 0 and math.isfinite(diff["f0_rmse_cents"]) and diff["f0_rmse_cents"] > 0
    assert abs(diff["f0_rmse_cents"] - 1200 * math.log2(180 / 150)) < 30, "the tones are 316 cents apart"
    assert 0 <= diff["voicing_error"] <= 1
    assert set(rep["speakers"]) == {"0", "7"} and rep["speakers"]["7"]["pairs"] == 1 and rep["overall"]["pairs"] == 2
    assert abs(rep["overall"]["mcd_db"] - diff["mcd_db"] / 2) < 1e-12
    assert len(rep["skipped"]) == 1 and rep["skipped"][0]["recorded"].endswith("short.wav")
