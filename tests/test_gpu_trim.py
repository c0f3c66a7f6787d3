"""ev_trim_bounds and ev_trim_apply on the MI355X, through the C ABI.

Yardstick: tests/trim_ref.py, the numpy float64 restatement of librosa.effects.trim's frames and bounds (librosa is not a dependency).
The bounds are integers, so the comparison is EXACT.  That is sound because the rows keep their distance from the threshold: they are
``trim_ref.three_level_row`` (Gaussian noise at -80 dB, -50 dB, a burst at 0 dB, and the mirror image) and with top_db = 60 every
frame's mean square lies at least 1 dB (a factor 1.26) from the threshold, asserted on the reference below; the device sums the exact
float64 squares of the same fp32 samples in another order, which moves a frame's sum by a few 2^-53 relative.  Lengths: 1, 63, 1023,
1024, 1025, 5000, 5120 and 3 * 2048 + 511, under (F, H) = (2048, 512), (1024, 256) and (512, 512): rows shorter than half a frame, at a
multiple of the hop and one off it, several workgroups per row (8 hop blocks each), and a hop-block grid offset by H / 2 (F / H odd).
Every batch is laid out with an odd row stride, so that rows start at all four alignments and both the 16-byte and the 4-byte load
paths run.  Two mutants of the EXPECTATION (the uncentred frame [f H, f H + F); the end not clipped to len) must each disagree with the
device on at least one of these cases.

The peak is compared bit for bit with ``x.abs().max()``, the output of ev_trim_apply bit for bit with ``x[start:end] * (target / peak)``
computed by torch in fp32 (one division, one multiply per sample).  Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py).

Times: not gated here (tools/trim_bench.py).  This module has not run on an MI355X yet: the margins and the restatement's bounds above are
CPU figures (tests/test_trim_host.py asserts them without a GPU); the TRIM lines of a -s run carry the device's.
"""
import json
import wave

import numpy as np
import pytest
import torch

import analysis_gpu as A
import trim_ref as T
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, EvLibraryError, _stream_ptr

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 1023, 1024, 1025, 5000, 5120, 3 * 2048 + 511]
CONFIGS = [(2048, 512), (1024, 256), (512, 512)]
L_PAD = max(LENGTHS) + 4                 # 6659: odd, so the rows of a batch start at every alignment
GARBAGE = 50.0                           # what lies behind a row's d_len samples: loud, so that reading it would show
_ROWS, _REF = {}, {}


def row(n):
    if n not in _ROWS:
        _ROWS[n] = T.three_level_row(n, seed=n)
    return _ROWS[n]


def ref_bounds(n, F, H):
    """(start, end) of the restatement for row(n), its margin asserted; computed once."""
    if (n, F, H) not in _REF:
        x, _ = row(n)
        margin = T.margin_db(T.frame_ms(x, F, H), 60.0)
        assert margin >= 1.0, f"row {n} under F={F} H={H}: a frame lies {margin:.2f} dB from the threshold"
        _REF[(n, F, H)] = T.bounds(x, 60.0, F, H)
    return _REF[(n, F, H)]


def padded_batch(lengths=LENGTHS, L=L_PAD):
    x = torch.full((len(lengths), L), GARBAGE)
    for b, n in enumerate(lengths):
        x[b, :n] = torch.from_numpy(row(n)[0])
    return x.to(DEV)


def on_device(out):
    """The collected host copies back on the device, where the tests compare them with torch (None stays None)."""
    return tuple(None if a is None else torch.from_numpy(a).to(DEV) for a in out.values())


def raw_bounds(eng, x, lens, F=2048, H=512, top_db=60.0, want_peak=True):
    """ev_trim_bounds into guarded buffers: (rc, bounds (B, 2) int32, peak (B,) or None)."""
    B, L = x.shape
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"bounds": ((B, 2), torch.int32), "peak": ((B,), torch.float32)}, () if want_peak else ("peak",))
    rc = eng.lib.ev_trim_bounds(eng.h, x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, F, H, top_db, out.ptr("bounds"),
                                out.ptr("peak"), _stream_ptr())
    return (rc, *on_device(out.collect(rc)))


def raw_apply(eng, x, bounds, peak, target, L_out):
    """ev_trim_apply into guarded buffers: (rc, y (B, L_out), out_len (B,))."""
    B, L = x.shape
    out = A.Guarded({"y": ((B, L_out), torch.float32), "out_len": ((B,), torch.int32)})
    rc = eng.lib.ev_trim_apply(eng.h, x.data_ptr(), bounds.data_ptr(), None if peak is None else peak.data_ptr(), target, B, L, out.ptr("y"), L_out,
                               out.ptr("out_len"), _stream_ptr())
    return (rc, *on_device(out.collect(rc)))


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


@pytest.mark.parametrize("F,H", CONFIGS, ids=[f"F{F}-H{H}" for F, H in CONFIGS])
def test_bounds_and_peak_equal_the_restatement_exactly(eng, F, H):
    want = [list(ref_bounds(n, F, H)) for n in LENGTHS]
    x = padded_batch()
    rc, bounds, peak = raw_bounds(eng, x, LENGTHS, F, H)
    assert rc == 0, err_of(eng)
    print(f"\nTRIM F{F} H{H}: device {bounds.tolist()}  restatement {want}")
    assert bounds.tolist() == want
    for b, n in enumerate(LENGTHS):
        assert peak[b].item() == x[b, :n].abs().max().item(), f"peak of row {n}"
        lens = row(n)[1]
        if n >= 4096:                                                    # (shorter rows: start = f_first H is coarser than their segments)
            assert bounds[b, 0] <= lens[0] and bounds[b, 1] >= n - lens[4], "the -50 dB parts are kept"
            assert bounds[b, 0] > 0, "-80 dB samples are dropped"
        alone = torch.from_numpy(row(n)[0]).to(DEV).unsqueeze(0)
        rc, b1, p1 = raw_bounds(eng, alone, None, F, H)                  # the row alone: L = len, no d_len
        assert rc == 0 and b1.tolist() == [want[b]] and torch.equal(p1, peak[b:b + 1])


def test_each_mutant_expectation_disagrees_with_the_device(eng):
    wrong = {"uncentred": 0, "unclipped": 0}
    for F, H in CONFIGS:
        rc, bounds, _ = raw_bounds(eng, padded_batch(), LENGTHS, F, H)
        assert rc == 0
        for b, n in enumerate(LENGTHS):
            ref_bounds(n, F, H)                                          # (asserts the margin)
            wrong["uncentred"] += tuple(bounds[b].tolist()) != T.bounds(row(n)[0], 60.0, F, H, centred=False)
            wrong["unclipped"] += tuple(bounds[b].tolist()) != T.bounds(row(n)[0], 60.0, F, H, clip_end=False)
    print(f"\nTRIM mutants: cases that disagree with the device {wrong}")
    assert wrong["uncentred"] > 0 and wrong["unclipped"] > 0


def test_alone_in_a_batch_and_as_a_prefix_give_the_same_bits(eng):
    n = 5000
    x = torch.from_numpy(row(n)[0]).to(DEV)
    rc, b0, p0 = raw_bounds(eng, x.unsqueeze(0).contiguous(), None)
    assert rc == 0 and b0.tolist() == [list(ref_bounds(n, 2048, 512))]
    g = torch.Generator().manual_seed(3)
    batch = (torch.randn(5, n + 1, generator=g) * 3.0).to(DEV)           # odd stride: row 3 starts 4 bytes off a 16-byte boundary
    batch[3, :n] = x
    batch[3, n:] = GARBAGE
    rc, b5, p5 = raw_bounds(eng, batch, [n + 1, 17, n + 1, n, 4000])
    assert rc == 0 and torch.equal(b5[3:4], b0) and torch.equal(p5[3:4], p0)
    long_row = torch.full((1, 2 * n + 77), GARBAGE, device=DEV)
    long_row[0, :n] = x
    rc, bp, pp = raw_bounds(eng, long_row, [n])
    assert rc == 0 and torch.equal(bp, b0) and torch.equal(pp, p0)
    rc, b5b, p5b = raw_bounds(eng, batch, [n + 1, 17, n + 1, n, 4000])
    assert rc == 0 and torch.equal(b5b, b5) and torch.equal(p5b, p5), "two calls, the same bits"
    rc, bn, pn = raw_bounds(eng, batch, [n + 1, 17, n + 1, n, 4000], want_peak=False)
    assert rc == 0 and pn is None and torch.equal(bn, b5)


@pytest.mark.parametrize("L_out", [L_PAD, 1000, 1001, 1], ids=lambda v: f"Lout{v}")
def test_apply_is_the_torch_product_bit_for_bit(eng, L_out):
    x = padded_batch()
    B = len(LENGTHS)
    rc, bounds, peak = raw_bounds(eng, x, LENGTHS)
    assert rc == 0
    gain = (torch.tensor(0.95, dtype=torch.float32) / peak.cpu()).to(DEV)    # one fp32 division per row, IEEE (on the host)
    rc, y, out_len = raw_apply(eng, x, bounds, peak, 0.95, L_out)
    assert rc == 0, err_of(eng)
    rc, c, c_len = raw_apply(eng, x, bounds, peak, 0.0, L_out)           # target <= 0: a copy
    rc2, c2, _ = raw_apply(eng, x, bounds, None, 0.95, L_out)            # no peak: a copy as well
    assert rc == 0 and rc2 == 0 and torch.equal(c, c2) and torch.equal(c_len, out_len)
    truncated = 0
    for b in range(B):
        s, e = bounds[b].tolist()
        k = min(e - s, L_out)
        truncated += e - s > L_out
        assert out_len[b].item() == k
        assert torch.equal(y[b, :k], x[b, s:s + k] * gain[b]), f"row {b}"
        assert torch.equal(c[b, :k], x[b, s:s + k])
        assert not y[b, k:].any() and not c[b, k:].any(), "zeros right of out_len"
        want, kk = T.apply(x[b].cpu().numpy(), s, e, peak[b].item(), 0.95, L_out)
        assert kk == k and np.array_equal(y[b].cpu().numpy(), want)
    if L_out < 2000:
        assert truncated > 0, "L_out below the trimmed length truncates"


def test_bad_rows_are_zeros(eng):
    n, L = 5000, 5003
    lens = [n, 0, L + 1, -3, 5]
    x = padded_batch([n] * 5, L)
    rc, bounds, peak = raw_bounds(eng, x, lens)
    assert rc == 0
    assert bounds[0].tolist() == list(ref_bounds(n, 2048, 512)) and peak[0].item() == x[0, :n].abs().max().item()
    for r in (1, 2, 3):
        assert bounds[r].tolist() == [0, 0] and peak[r].item() == 0.0, f"row {r} (len {lens[r]})"
    assert bounds[4].tolist() == [0, 5] and peak[4].item() == x[4, :5].abs().max().item()
    rc, y, out_len = raw_apply(eng, x, bounds, peak, 0.95, L)
    assert rc == 0 and out_len.tolist() == [bounds[0, 1].item() - bounds[0, 0].item(), 0, 0, 0, 5]
    assert not y[1:4].any()
    hand = torch.tensor([[10, 5], [-1, 4], [0, L + 1], [3, 3], [2, 9]], dtype=torch.int32, device=DEV)     # start > end, start < 0, end > L
    rc, y, out_len = raw_apply(eng, x, hand, None, 0.0, 16)
    assert rc == 0 and out_len.tolist() == [0, 0, 0, 0, 7]
    assert not y[:4].any() and torch.equal(y[4, :7], x[4, 2:9]) and not y[4, 7:].any()


def test_parameter_violations_name_the_constraint(eng):
    x = torch.zeros(1, 9000, device=DEV)
    with pytest.raises(EvLibraryError, match="multiple of hop_length"):
        eng.trim_bounds(x, None, 60, 2000, 512)                          # F % H != 0
    with pytest.raises(EvLibraryError, match="hop_length=100 must be a multiple of 64"):
        eng.trim_bounds(x, None, 60, 2000, 100)
    with pytest.raises(EvLibraryError, match="hop_length=8192 .* at most 4096"):
        eng.trim_bounds(x, None, 60, 8192, 8192)
    with pytest.raises(EvLibraryError, match="exceeds 64"):
        eng.trim_bounds(x, None, 60, 8192, 64)                           # F / H = 128
    with pytest.raises(EvLibraryError, match="65535"):
        eng.trim_bounds(torch.zeros(65536, 8, device=DEV))
    b, _ = eng.trim_bounds(x, None, 60, 4096, 64)                        # F / H = 64 is the last that runs
    assert b.tolist() == [[0, 9000]]
    with pytest.raises(EvLibraryError, match="L_out"):
        eng.trim_apply(x, b, None, 0.0, out_len=0)


def test_scratch_is_allocated_once_per_shape():
    e = Engine(0)                                                        # no weights loaded
    x = padded_batch()
    n0 = e.alloc_count()
    b1, p1 = e.trim_bounds(x, LENGTHS)
    torch.cuda.synchronize()
    n1 = e.alloc_count()
    assert n1 - n0 <= 1
    b2, p2 = e.trim_bounds(x, LENGTHS)
    y, k = e.trim_apply(x, b2, p2, 0.95)
    e.trim_bounds(x[:3, :4000].contiguous())                             # a smaller shape fits the arena
    torch.cuda.synchronize()
    assert e.alloc_count() == n1 and torch.equal(b1, b2) and torch.equal(p1, p2)
    for setting in (16, 6, 0):                                           # ev_set_arithmetic does not reach these calls
        e.set_arithmetic(setting)
        b3, p3 = e.trim_bounds(x, LENGTHS)
        y3, k3 = e.trim_apply(x, b3, p3, 0.95)
        assert torch.equal(b3, b1) and torch.equal(p3, p1) and torch.equal(y3, y) and torch.equal(k3, k), f"arithmetic {setting}"
    assert e.alloc_count() == n1
    e.close()


def test_python_call_shapes():
    n = 5000
    x = torch.from_numpy(row(n)[0]).to(DEV)
    s, e = ref_bounds(n, 2048, 512)
    y, (gs, ge) = audio.trim_silence(x)
    assert (gs, ge) == (s, e) and torch.equal(y, x[s:e])
    batch, out_len, bounds = audio.trim_silence(padded_batch(), lengths=LENGTHS)
    want = [list(ref_bounds(m, 2048, 512)) for m in LENGTHS]
    assert bounds.tolist() == want and out_len.tolist() == [b - a for a, b in want] and batch.shape[1] == max(b - a for a, b in want)
    assert torch.equal(batch[5, : e - s], x[s:e]) and not batch[5, e - s:].any()
    lv = audio.peak_normalize(x, 0.95)
    assert torch.equal(lv, x * (torch.tensor(0.95) / x.abs().max().cpu()).to(DEV)) and abs(lv.abs().max().item() - 0.95) < 1e-6
    z = torch.zeros(3000, device=DEV)
    assert torch.equal(audio.peak_normalize(z), z) and audio.trim_silence(z)[1] == (0, 3000)


def _write_wav(path, x, rate, channels=1, width=2):
    """x (n,) or (n, channels) in [-1, 1] as 16- or 24-bit PCM."""
    x = np.clip(np.asarray(x, np.float64), -1, 1).reshape(-1)
    if width == 2:
        raw = np.round(x * 32767).astype("<i2").tobytes()
    else:
        q = np.round(x * (2 ** 23 - 1)).astype(np.int32)
        raw = (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw)


def test_cli_prepares_a_dataset_end_to_end(tmp_path):
    from emojivoice_amd.cli import cli

    raw = tmp_path / "raw"
    raw.mkdir()
    a = T.three_level_row(40000, seed=1, burst_rms=0.15)[0]
    _write_wav(raw / "a.wav", np.stack([a, 0.5 * a], axis=1), 44100, channels=2)          # 44.1 kHz stereo, 16 bit
    _write_wav(raw / "b.wav", T.three_level_row(16000, seed=2, burst_rms=0.1)[0], 22050)     # 22.05 kHz mono, 16 bit
    _write_wav(raw / "c.wav", T.three_level_row(12000, seed=3, burst_rms=0.2)[0], 22050, width=3)   # 24 bit
    flist = tmp_path / "raw.txt"
    flist.write_text(f"{raw / 'a.wav'}|3|first\nraw/b.wav|3|second\nraw/c.wav|5|third\n", encoding="utf-8")
    out = tmp_path / "clean"
    cli(["--prepare_dataset", str(flist), "--out_dir", str(out)])
    with open(f"{flist}.durations.json") as f:
        rep = json.load(f)
    lines = (out / "filelist.txt").read_text(encoding="utf-8").splitlines()
    assert [ln.split("|", 1)[1] for ln in lines] == ["3|first", "3|second", "5|third"]
    minutes = {"3": 0.0, "5": 0.0}
    for name, spk, ln, rec in zip("abc", "335", lines, rep["files"]):
        y, info = audio.prepare_recording(raw / f"{name}.wav", 22050, 60, 0.95, DEV)
        assert 0 < info["start"] < info["end"] and info["seconds_out"] < info["seconds_in"], "something was trimmed"
        assert abs(y.abs().max().item() - 0.95) <= 1e-6, "levelled: the loudest sample lies inside the kept part"
        with wave.open(ln.split("|")[0], "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 22050)
            q = np.frombuffer(w.readframes(w.getnframes()), "<i2")
        want = np.round(np.clip(y.cpu().numpy().astype(np.float64), -1, 1) * 32767).astype("<i2")
        assert np.array_equal(q, want), name
        assert rec["speaker"] == spk and rec["seconds_in"] == info["seconds_in"] and rec["seconds_out"] == info["seconds_out"] == len(q) / 22050
        minutes[spk] += info["seconds_out"] / 60.0
    assert set(rep["speakers"]) == {"3", "5"} and rep["below_two_minutes"] == ["3", "5"]
    for spk in minutes:
        assert abs(rep["speakers"][spk]["minutes"] - minutes[spk]) < 1e-12 and rep["speakers"][spk]["below_two_minutes"]
    assert abs(rep["total_minutes_out"] - sum(minutes.values())) < 1e-12
    cli(["--data_statistics", str(out / "filelist.txt"), "--batch_size", "2"])                # the new list feeds the statistics unchanged
    with open(f"{out / 'filelist.txt'}.stats.json") as f:
        stats = json.load(f)
    assert set(stats) == {"mel_mean", "mel_std"} and np.isfinite(stats["mel_mean"]) and stats["mel_std"] > 0
