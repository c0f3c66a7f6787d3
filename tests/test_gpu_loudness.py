"""ev_loudness on the MI355X, through the C ABI.

Yardstick: tests/loudness_ref.py, the numpy / scipy float64 restatement (scipy.signal.lfilter per stage over the whole row).  The device
filters the row in chunks of 1024 samples joined by an exact carry of the filter state and sums in another order, so it differs from the
restatement by float64 rounding: two float64 orderings of this recurrence differ by 6e-14 on the signal on the CPU.  The rule of every
comparison (``check``):
  * d_sub within 1e-9, relative to max(ref, 1e-9 x the row's largest sub-block energy); d_block and d_gated by the same rule, each against
    its own row maximum.  1e-9 is four orders above the reordering error and corresponds to 4e-9 dB;
  * each case first asserts that the restatement's gate margin is at least 1e-3 dB; then d_counts must be EQUAL;
  * d_block must be BIT-EQUAL to the header's formula applied on the host to the device's own d_sub.
Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py).  Inputs carry loud garbage (50.0) behind each row's length.

Observed on the MI355X (printed by every case; the gate stays at 1e-9): the worst relative error of any case is 8.6e-12 (d_sub of the
gating row at S = 64, on a sub-block 7e-9 of the row's maximum, where the loud segment's decaying tail is measured against near-silence);
the cases without such a segment stay at or under 4e-13.

Times: not gated here (tools/loudness_bench.py).
"""
import json
import wave

import numpy as np
import pytest
import torch

import analysis_gpu as A
import loudness_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import _stream_ptr

pytestmark = pytest.mark.gpu

TOL = 1e-9
K22 = audio.k_weighting(22050)
_REF = {}


def ref_of(key, x, lens, S, coef=K22):
    """The restatement's result, computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: R.loudness(x, lens, S, coef))


def raw(eng, x, lens, S, coef=K22, abs_gate=R.ABS_GATE, want=(True, True), B=None, L=None, null=()):
    """ev_loudness into guarded buffers: (rc, sub (B, NS), block (B, NB), gated (B, 2), counts (B, 3)) on the host; sub / block None when not
    asked for.  ``B`` / ``L`` override the shape passed to the library, ``null`` names pointers passed as NULL (the argument tests)."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    Bx, Lx = x.shape
    B, L = Bx if B is None else B, Lx if L is None else L
    NS = Lx // S if S > 0 else 0
    NB = max(NS - 3, 0)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"sub": ((Bx, NS), torch.float64), "block": ((Bx, NB), torch.float64), "gated": ((Bx, 2), torch.float64),
                     "counts": ((Bx, 3), torch.int32)}, tuple(null) + tuple(k for k, w in zip(("sub", "block"), want) if not w))
    coef = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
    rc = eng.lib.ev_loudness(eng.h, None if "x" in null else x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, S,
                             None if coef is None else coef.ctypes.data, float(abs_gate), out.ptr("sub"), out.ptr("block"), out.ptr("gated"),
                             out.ptr("counts"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def rel_err(dev, ref):
    """max |dev - ref| / max(|ref|, 1e-9 x the row's largest |ref|); a row whose reference is all zeros must be all zeros."""
    worst = 0.0
    for d, r in zip(np.atleast_2d(dev), np.atleast_2d(ref)):
        top = float(np.max(np.abs(r))) if r.size else 0.0
        if top == 0.0:
            assert not d.any(), "a row of zeros in the reference is a row of zeros on the device"
            continue
        worst = max(worst, float(np.max(np.abs(d - r) / np.maximum(np.abs(r), 1e-9 * top))))
    return worst


def check(dev, ref, S, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    sub, block, gated, counts = dev
    assert float(ref["margin"].min()) >= 1e-3, f"{what}: the reference's gate margin {float(ref['margin'].min()):.3e} dB is under 1e-3 dB"
    e_s, e_b, e_g = rel_err(sub, ref["sub"]), rel_err(block, ref["block"]), rel_err(gated, ref["gated"])
    print(f"\nLOUDNESS {what}: rel err sub {e_s:.3e} block {e_b:.3e} gated {e_g:.3e} (gate {TOL:g})  counts {counts.tolist()}  "
          f"least margin {float(ref['margin'].min()):.3f} dB  integrated {R.lufs(gated[:, 0]).tolist()}")
    assert np.array_equal(counts, ref["counts"]), f"{what}: d_counts {counts.tolist()} against {ref['counts'].tolist()}"
    assert np.array_equal(block, R.block_formula(sub, counts, S)), f"{what}: d_block is not the formula applied to the device's own d_sub"
    assert e_s <= TOL, f"{what}: d_sub"
    assert e_b <= TOL, f"{what}: d_block"
    assert e_g <= TOL, f"{what}: d_gated"


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


# ---- 1. gating ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.GATING_S)
def test_gating(eng, S):
    row = R.gating_row(S)
    x, lens = R.padded([row], tail=65)                                   # garbage behind the row; at S = 64 a 41st, empty sub-block
    ref = ref_of(("gating", S), x, lens, S)
    assert tuple(ref["counts"][0]) == R.GATING_COUNTS[S] and abs(ref["integrated"][0] - R.GATING_LUFS[S]) <= 0.01
    rc, *dev = raw(eng, x, lens, S)
    assert rc == 0, err_of(eng)
    check(dev, ref, S, f"gating S{S} len {len(row)}")
    assert not dev[0][0, len(row) // S:].any() and not dev[1][0, ref["counts"][0, 0]:].any(), "zeros past the row's own sub-blocks and blocks"


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------------
def test_edges_in_one_ragged_batch(eng):
    x, lens = R.edge_rows()
    ref = ref_of("edges", x, lens, R.EDGE_S)
    assert ref["counts"][:, 0].tolist() == [0, 1, 1, 1, 0, 12, 13, 13, 30, 0, 0]
    rc, *dev = raw(eng, x, lens, R.EDGE_S)
    assert rc == 0, err_of(eng)
    check(dev, ref, R.EDGE_S, f"edges S64 lens {lens}")
    for b in (9, 10):
        assert not dev[0][b].any() and not dev[1][b].any() and not dev[2][b].any() and not dev[3][b].any(), "len > L and len = 0 are rows of zeros"
    assert not dev[1][0].any() and not dev[2][0].any() and dev[0][0, :3].all() and not dev[0][0, 3:].any(), "4 S - 1 samples: three sub-blocks, no block"
    assert not dev[0][4].any(), "a single sample is no sub-block"


# ---- 3. independence of batch and padding ------------------------------------------------------------------------------------------------
def test_row_alone_in_a_batch_and_as_a_prefix_give_the_same_bits(eng):
    S = 100
    row = R.gating_row(S)                                                # 4028 samples: four chunks of the device's filter
    n, ns = len(row), len(row) // S
    rc, *alone = raw(eng, row[None], None, S)
    assert rc == 0, err_of(eng)
    rc, *again = raw(eng, row[None], None, S)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    g = np.random.default_rng(3)
    others = [(0.2 * g.standard_normal(n + 777)).astype(np.float32), (0.05 * g.standard_normal(1500)).astype(np.float32)]
    xb, lb = R.padded([others[0], row, others[1]])
    rc, *batch = raw(eng, xb, lb, S)
    assert rc == 0
    xp, lp = R.padded([others[1], row], L=n + 1234)                      # (an even L: other row alignments than in the batch of 3)
    rc, *prefix = raw(eng, xp, lp, S)
    assert rc == 0
    for name, a, b, c, valid in zip(("sub", "block", "gated", "counts"), alone, batch, prefix, (ns, ns - 3, 2, 3)):
        assert a.shape[1] == valid
        assert np.array_equal(a[0], b[1, :valid]) and not b[1, valid:].any(), f"{name}: alone against inside a batch"
        assert np.array_equal(a[0], c[1, :valid]) and not c[1, valid:].any(), f"{name}: alone against the prefix of a padded row"
    rc, _, _, gated, counts = raw(eng, xb, lb, S, want=(False, False))
    assert rc == 0 and np.array_equal(gated, batch[2]) and np.array_equal(counts, batch[3]), "without d_sub and d_block"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 6, 16):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, xb, lb, S)
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)


# ---- 4. silence --------------------------------------------------------------------------------------------------------------------------
def test_silence(eng):
    rc, sub, block, gated, counts = raw(eng, np.zeros((1, 8 * 64), np.float32), None, 64)
    assert rc == 0, err_of(eng)
    assert counts.tolist() == [[5, 0, 0]] and gated.tolist() == [[0.0, 0.0]]
    assert sub.shape == (1, 8) and block.shape == (1, 5) and not sub.any() and not block.any()
    out = audio.loudness(torch.zeros(2, 22050, device=DEV), lengths=[22050, 500])
    assert out["integrated"].tolist() == [float("-inf")] * 2 and out["blocks"].tolist() == [7, 0] and out["gated_blocks"].tolist() == [0, 0]
    assert bool(torch.isinf(out["momentary"]).all())


# ---- 5. audio.loudness on realistic rows -------------------------------------------------------------------------------------------------
def test_audio_loudness_on_realistic_rows():
    x, lens = R.realistic_rows()
    ref = ref_of("realistic", x, lens, 2205)
    assert float(ref["margin"].min()) >= 1e-3
    xd = torch.from_numpy(x).to(DEV)
    out = audio.loudness(xd, 22050, lengths=lens)
    e = audio._trim_engine(xd.device)
    n0 = e.alloc_count()
    out2 = audio.loudness(xd, 22050, lengths=lens)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0, "a second call at the same shape allocates nothing"
    assert all(torch.equal(out[k], out2[k]) for k in out), "two calls"
    assert out["integrated"].dtype == torch.float64 and out["sub_energy"].shape == (3, 30) and out["momentary"].shape == (3, 27)
    power = lambda l: np.where(np.isfinite(l), 10.0 ** ((l - R.OFFSET) / 10.0), 0.0)
    e_s = rel_err(out["sub_energy"].cpu().numpy(), ref["sub"])
    e_b = rel_err(power(out["momentary"].cpu().numpy()), ref["block"])
    e_i = rel_err(power(out["integrated"].cpu().numpy())[:, None], ref["gated"][:, :1])
    print(f"\nLOUDNESS audio.loudness 1.0 / 2.3 / 3.0 s: rel err sub {e_s:.3e} momentary (as power) {e_b:.3e} integrated (as power) {e_i:.3e}  "
          f"integrated {out['integrated'].tolist()} LUFS  blocks {out['blocks'].tolist()} gated {out['gated_blocks'].tolist()}")
    assert out["blocks"].tolist() == ref["counts"][:, 0].tolist() and out["gated_blocks"].tolist() == ref["counts"][:, 2].tolist()
    assert e_s <= TOL and e_b <= TOL and e_i <= TOL
    one = audio.loudness(xd[0, :lens[0]])
    assert one["integrated"].shape == (1,) and float(one["integrated"][0]) == float(out["integrated"][0]), "a 1-D input is the same row"


# ---- 6. arguments ------------------------------------------------------------------------------------------------------------------------
UNSTABLE_1 = np.concatenate([[1.0, 0.0, 0.0, -2.1, 1.05], K22[5:]])       # |a2| >= 1
UNSTABLE_2 = np.concatenate([K22[:5], [1.0, -2.0, 1.0, -1.995, 0.99]])    # |a1| >= 1 + a2
BAD_ARGS = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("sub_len", dict(S=15)), ("sub_len", dict(S=65537)), ("sub_len", dict(S=0)), ("L=", dict(L=0)),
    ("d_gated", dict(null=("gated",))), ("d_counts", dict(null=("counts",))), ("d_x", dict(null=("x",))), ("coef", dict(coef=None)),
    ("stage 1", dict(coef=UNSTABLE_1)), ("stage 2", dict(coef=UNSTABLE_2)), ("stage 2", dict(coef=np.concatenate([K22[:9], [float("nan")]]))),
]


@pytest.mark.parametrize("word,kw", BAD_ARGS, ids=[f"{w.strip('=').replace(' ', '')}-{i}" for i, (w, _) in enumerate(BAD_ARGS)])
def test_each_limit_fails_with_a_message_naming_it(eng, word, kw):
    kw = dict(kw)
    S = kw.pop("S", 64)
    rc, *_ = raw(eng, np.zeros((2, 1024), np.float32), None, S, **kw)   # (a failed call writes nothing: raw checks that)
    msg = err_of(eng)
    assert rc != 0 and "ev_loudness" in msg and word in msg, msg


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------------------------
def _takes():
    """Three short takes of two speakers: a tone under noise at two levels, and a quiet one with a click (a high peak at a low loudness)."""
    g = np.random.default_rng(5)
    n = 33075                                                           # 1.5 s
    tone = lambda a, f: (R.P.harmonic_tone(f, n, scale=a) + (0.05 * a * g.standard_normal(n))).astype(np.float32)
    a, b, c = tone(0.2, 150.0), tone(0.04, 190.0), tone(0.03, 120.0)
    c[n // 2] = 0.9
    return {"a.wav": ("7", a), "b.wav": ("7", b), "c.wav": ("12", c)}


def _read16(path):
    with wave.open(str(path), "rb") as f:
        return f.readframes(f.getnframes()), f.getframerate()


def test_loudness_report_and_prepare_dataset_target_lufs(tmp_path):
    from emojivoice_amd import cli

    raw_dir = tmp_path / "raw"
    raw_dir.mkdir()
    takes = _takes()
    for name, (_, y) in takes.items():
        cli.write_wav_pcm16(raw_dir / name, y, 22050)
    flist = tmp_path / "raw.txt"
    flist.write_text("".join(f"raw/{name}|{spk}|text of {name}\n" for name, (spk, _) in takes.items()), encoding="utf-8")

    rep = cli.cli(["--loudness_report", str(flist), "--batch_size", "2"])
    with open(f"{flist}.loudness.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep)) and set(saved) == {"sample_rate", "outlier_lu", "files", "speakers"}
    k = audio.k_weighting(22050)
    for f_, (name, (spk, y)) in zip(saved["files"], takes.items()):
        q = np.round(np.clip(y.astype(np.float64), -1, 1) * 32767.0) / 32768.0       # what the 16-bit file holds
        want = R.loudness(q.astype(np.float32), None, 2205, k)
        assert f_["speaker"] == spk and f_["seconds"] == 1.5 and f_["path"].endswith(name)
        assert abs(f_["integrated_lufs"] - want["integrated"][0]) < 1e-6 and abs(f_["max_momentary_lufs"] - R.lufs(want["block"][0]).max()) < 1e-6
        assert abs(f_["peak_dbfs"] - 20 * np.log10(np.abs(q).max())) < 1e-5
    s7 = saved["speakers"]["7"]
    la, lb = saved["files"][0]["integrated_lufs"], saved["files"][1]["integrated_lufs"]
    assert s7["files"] == 2 and s7["measured"] == 2 and abs(s7["mean"] - (la + lb) / 2) < 1e-9 and abs(s7["std"] - abs(la - lb) / 2) < 1e-9
    assert (s7["min"], s7["max"]) == (min(la, lb), max(la, lb)) and abs(la - lb) > 13 and len(s7["outliers"]) == 2, "14 dB apart: both 7 LU off the mean"
    assert saved["speakers"]["12"]["files"] == 1 and saved["speakers"]["12"]["outliers"] == []

    # levelled by loudness: the files land on the target where the peak allows it
    target = -20.0
    out = tmp_path / "clean"
    cli.cli(["--prepare_dataset", str(flist), "--out_dir", str(out), "--target_lufs", str(target)])
    with open(f"{flist}.durations.json") as f:
        dur = json.load(f)
    assert dur["target_lufs"] == target and [f_["capped"] for f_ in dur["files"]] == [False, False, True]
    again = cli.cli(["--loudness_report", str(out / "filelist.txt")])
    for f_, d in zip(again["files"], dur["files"]):
        assert set(d) >= {"integrated_lufs", "gain_db", "capped", "seconds_in", "seconds_out"}
        print(f"\nLOUDNESS prepared {f_['path']}: {d['integrated_lufs']:.2f} LUFS {d['gain_db']:+.2f} dB capped {d['capped']} -> {f_['integrated_lufs']:.3f} LUFS "
              f"peak {f_['peak_dbfs']:.2f} dBFS")
        if not d["capped"]:
            assert abs(f_["integrated_lufs"] - target) <= 0.1
            assert abs(d["integrated_lufs"] + d["gain_db"] - target) < 1e-9
        else:
            assert f_["integrated_lufs"] < target - 0.1 and abs(f_["peak_dbfs"] - 20 * np.log10(0.95)) < 0.01, "held at the peak ceiling, under the target"

    # without the flag: today's bytes, i.e. audio.prepare_recording's output through the 16-bit writer, and today's JSON keys
    plain = tmp_path / "plain"
    rep = cli.cli(["--prepare_dataset", str(flist), "--out_dir", str(plain)])
    assert "target_lufs" not in rep and all(set(f_) == {"path", "out", "speaker", "seconds_in", "seconds_out"} for f_ in rep["files"])
    for name in takes:
        y, _ = audio.prepare_recording(raw_dir / name, 22050, 60.0, 0.95, DEV)
        cli.write_wav_pcm16(tmp_path / "want.wav", y.cpu().numpy(), 22050)
        assert (plain / name).read_bytes() == (tmp_path / "want.wav").read_bytes(), f"{name}: --prepare_dataset without --target_lufs changed"
