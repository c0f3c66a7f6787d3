"""ev_resample and ev_mel_stats on the MI355X, through the C ABI.

Yardstick of the resampler: ``scipy.signal.resample_poly`` (padtype="constant") on the float64 copy of the input, with the engine's
float32 taps widened to float64 and handed over as ``window=taps / up`` (scipy multiplies an array filter by ``up`` itself;
tests/test_resample_host.py pins that call to the C ABI's formula).  Engine and yardstick therefore see the same numbers, and what is
left is the rounding of the accumulation.  Errors are max |d| and rms(d) over the whole case, both relative to the RMS of the case's
yardstick output.

Gate.  scipy's own float32 run — ``resample_poly`` on the float32 input and the float32 taps — measured against the yardstick on exactly
the CASES below (RSERR lines with -s: the float32 run measured live, then the engine):
    1/2 noise, 41 taps                          max 6.2e-7   rms 8.9e-8
    147/320 sines                               max 1.9e-6   rms 1.2e-7        <- the worst max
    320/147 chirp                               max 4.2e-7   rms 8.4e-8
    441/320 noise 1e-4; the same at 4.9 M       max 7.2e-7; 1.4e-6   rms 8.8e-8; 9.1e-8
    160/147 mixed B 64; L_out 1023, 1024, 1025  max 1.2e-6; 4.7e-7 .. 1.0e-6   rms 8.3e-8 .. 9.0e-8
    1/2, zeros=32 beta=12 (129 taps)            max 1.7e-6   rms 1.4e-7        <- the worst RMS
    3/7 L=50, 5/3 L=1                           max 1.7e-7, 5.3e-9
The engine is gated at 3x the worst figure, as the other modules gate at ~3x their worst measured value:
    GATE_MAX = 5.76e-6,  GATE_RMS = 4.20e-7   on every case,
and the live float32 figure must stay within 1.5x the recorded one (a stale gate is caught).
Mutants — the filter shifted by one tap, the gain ``up`` left out — are handed to the engine as taps and measured by the same function:
they exceed the gate on every case with up > 1, the shifted filter also at 1/2.

The engine's worst max / RMS on an MI355X: not measured yet — this module has not run on a GPU (the float32 figures above are CPU runs of
scipy and need none); the RSERR lines of a -s run carry the figures that belong here.

``TILE`` is the kernel's output tile (outputs per workgroup); three cases put L_out one below, at and one above a
multiple of it, and (441, 320, 1, 4 900 000) puts L_in * up past 2^31.  ev_mel_stats is compared with float64 numpy to 1e-9 relative:
float64 accumulation of n terms of one sign is off by at most n 2^-53 relative, 5.9e-10 for the 5.3 M terms of the largest case (the
squares; the plain sums have one sign too: log-mels around -5.5 +- 2).
"""
import json
import wave

import numpy as np
import pytest
import torch
from scipy import signal as sps

import analysis_gpu as A
import mel_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, EvLibraryError, _stream_ptr

pytestmark = pytest.mark.gpu

TILE = 1024
F32_MAX, F32_RMS = 1.92e-6, 1.40e-7              # scipy's float32 run: worst case over CASES (module docstring)
GATE_MAX, GATE_RMS = 3 * F32_MAX, 3 * F32_RMS
# (up, down, B, L, zeros, beta, signal)
CASES = [(1, 2, 3, 4097, 10, 5.0, "noise1"), (147, 320, 3, 5000, 10, 5.0, "sines"), (320, 147, 2, 3001, 10, 5.0, "chirp"),
         (441, 320, 1, 2500, 10, 5.0, "noise1e-4"), (160, 147, 64, 700, 10, 5.0, "mixed"), (3, 7, 1, 50, 10, 5.0, "noise1"),
         (5, 3, 1, 1, 10, 5.0, "noise1"), (1, 2, 2, 3000, 32, 12.0, "mixed"),
         (160, 147, 2, 939, 10, 5.0, "noise1"), (160, 147, 2, 940, 10, 5.0, "sines"), (160, 147, 2, 941, 10, 5.0, "noise1e-4"),   # L_out 1023, 1024, 1025
         (441, 320, 1, 4_900_000, 10, 5.0, "noise1")]
IDS = [f"{u}over{d}-B{b}-L{l}" + ("" if z == 10 else f"-z{z}") for u, d, b, l, z, _, _ in CASES]
_CACHE = {}


def l_out(L, up, down):
    return -(-L * up // down)


def case_data(case):
    """(x float32 (B, L), taps float32, yardstick float64 (B, L_out), scipy's float32 run): computed once per case, never modified."""
    if case not in _CACHE:
        up, down, B, L, zeros, beta, kind = case
        x = R.signal(kind, B, L, seed=B + L).numpy()
        taps = audio.resample_filter(up, down, zeros, beta)
        ref = sps.resample_poly(x.astype(np.float64), up, down, axis=-1, window=taps.astype(np.float64) / up, padtype="constant")
        f32 = sps.resample_poly(x, up, down, axis=-1, window=taps / np.float32(up), padtype="constant")
        assert ref.dtype == np.float64 and ref.shape == (B, l_out(L, up, down))
        _CACHE[case] = (x, taps, ref, f32)
    return _CACHE[case]


def errors(got, ref):
    """(max, rms) of got - ref relative to the RMS of ref."""
    d = np.asarray(got, dtype=np.float64) - ref
    scale = float(np.sqrt(np.mean(ref ** 2)))
    return float(np.abs(d).max()) / scale, float(np.sqrt(np.mean(d ** 2))) / scale


def engine_with(taps, up, down):
    eng = Engine(0)
    eng.load_resampler(taps, up, down)
    return eng


@pytest.fixture(scope="module")
def engines():
    for get in A.engines_on_demand(lambda key: engine_with(audio.resample_filter(*key), key[0], key[1])):
        yield lambda up, down, zeros=10, beta=5.0: get((up, down, zeros, beta))


def test_the_cases_cover_the_tile_boundary_and_the_31_bit_limit():
    louts = [l_out(c[3], c[0], c[1]) for c in CASES]
    assert {TILE - 1, TILE, TILE + 1} <= set(louts)
    assert any(c[3] * c[0] > 2 ** 31 and l_out(c[3], c[0], c[1]) * c[1] > 2 ** 31 for c in CASES)
    assert any(c[2] > 1 and l_out(c[3], c[0], c[1]) > TILE for c in CASES), "more than one workgroup per row"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_with_resample_poly(engines, case):
    up, down, B, L, zeros, beta, kind = case
    x, taps, ref, f32 = case_data(case)
    fmx, frms = errors(f32, ref)
    print(f"\nRSERR {up}/{down} B{B} L{L} {kind}: scipy float32 max {fmx:.2e} rms {frms:.2e}")
    assert f32.dtype == np.float32
    assert fmx <= 1.5 * F32_MAX and frms <= 1.5 * F32_RMS, "the float32 run moved: the gate constants are stale"
    got = engines(up, down, zeros, beta).resample(torch.from_numpy(x).to(DEV))
    assert tuple(got.shape) == ref.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    mx, rms = errors(got, ref)
    print(f"RSERR {up}/{down} B{B} L{L} {kind}: engine max {mx:.2e} rms {rms:.2e}  gate {GATE_MAX:.2e} / {GATE_RMS:.2e}")
    assert np.isfinite(got).all()
    assert mx <= GATE_MAX and rms <= GATE_RMS, (case, mx, rms)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mutants_exceed_the_gate(case):
    up, down, B, L, zeros, beta, kind = case
    x, taps, ref, _ = case_data(case)
    shifted = np.concatenate([np.zeros(1, np.float32), taps[:-1]])
    mutants = [("shifted by one tap", shifted)] + ([("gain up left out", taps / np.float32(up))] if up > 1 else [])
    for name, t in mutants:
        eng = engine_with(t, up, down)
        got = eng.resample(torch.from_numpy(x).to(DEV)).cpu().numpy()
        eng.close()
        mx, rms = errors(got, ref)
        print(f"\nRSERR mutant {name} on {up}/{down} B{B} L{L}: max {mx:.2e} rms {rms:.2e}")
        assert mx > GATE_MAX and rms > GATE_RMS, (name, case, mx, rms)


def test_two_calls_alone_and_in_a_batch_give_the_same_bits(engines):
    up, down = 147, 320
    eng = engines(up, down)
    x = R.signal("mixed", 64, 3100, seed=7).to(DEV)                      # 1424 outputs: two workgroups per row
    a, b = eng.resample(x), eng.resample(x)
    assert torch.equal(a, b), "two calls"
    for r in (0, 5, 63):
        assert torch.equal(eng.resample(x[r:r + 1].contiguous()), a[r:r + 1]), f"row {r} alone against the same row in the batch of 64"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = eng.resample(x)
    side.synchronize()
    assert torch.equal(a, c)
    for s in (16, 0, 6, 16):
        eng.set_arithmetic(s)
        assert torch.equal(eng.resample(x), a), "no fp16 / bf16 pieces in any arithmetic setting"


@pytest.mark.parametrize("up,down", [(441, 320), (1, 2), (320, 147)])
def test_ragged_batch_against_each_row_alone(engines, up, down):
    eng = engines(up, down)
    L = 3000
    lens = [3000, 1, 1500, 2999, 77, 1033]
    x = R.signal("noise1", len(lens), L, seed=3).to(DEV)                 # the padding behind a row is NOT zero: the lengths must mask it
    got = eng.resample(x, torch.tensor(lens))
    assert tuple(got.shape) == (len(lens), l_out(L, up, down))
    for r, n in enumerate(lens):
        alone = eng.resample(x[r:r + 1, :n].contiguous())
        k = l_out(n, up, down)
        assert alone.shape[1] == k
        assert torch.equal(got[r, :k], alone[0]), f"row {r} (len {n}): the prefix of a longer padded row, the same bits"
        assert not got[r, k:].any(), f"row {r}: zeros beyond ceil(len * up / down)"


def test_bad_and_empty_rows_sentinels_and_allocations():
    up, down, L = 147, 320, 2600
    eng = engine_with(audio.resample_filter(up, down), up, down)
    lens = [L, 0, L + 1, 5, -3, L]
    B, Lo, M = len(lens), l_out(L, up, down), 4096
    x = R.signal("noise1", B, L, seed=12).to(DEV)
    d_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    buf = torch.full((B * Lo + 2 * M,), 777.0, device=DEV)

    def call(lout=Lo):
        return eng.lib.ev_resample(eng.h, x.data_ptr(), d_len.data_ptr(), B, L, buf.data_ptr() + 4 * M, lout, _stream_ptr())

    assert call() == 0
    torch.cuda.synchronize()
    n0 = eng.alloc_count()
    assert call() == 0
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0 == 0, "the tap table is the only scratch: nothing is allocated by a call"
    assert bool((buf[:M] == 777.0).all()) and bool((buf[M + B * Lo:] == 777.0).all()), "sentinel margin"
    y = buf[M: M + B * Lo].reshape(B, Lo)
    for r in (1, 2, 4):
        assert not y[r].any(), f"row {r} (len {lens[r]}) is written as zeros"
    for r in (0, 5):
        assert torch.equal(y[r:r + 1], eng.resample(x[r:r + 1].contiguous())), "the neighbours of a bad row are unchanged"
    k = l_out(5, up, down)
    assert torch.equal(y[3, :k], eng.resample(x[3:4, :5].contiguous())[0]) and not y[3, k:].any()
    assert call(Lo + 1) != 0 and "L_out" in err_of(eng)
    assert call(Lo - 1) != 0 and "L_out" in err_of(eng)
    eng.close()


def test_refusals_name_the_constraint():
    eng = Engine(0)
    x = torch.zeros(1, 100, device=DEV)
    with pytest.raises(EvLibraryError, match="not loaded"):
        eng.resample(x)
    t = np.ones(21, np.float32)
    with pytest.raises(EvLibraryError, match="gcd"):
        eng.load_resampler(t, 2, 4)
    with pytest.raises(EvLibraryError, match="odd"):
        eng.load_resampler(np.ones(20, np.float32), 1, 2)
    with pytest.raises(EvLibraryError, match="65537"):
        eng.load_resampler(np.ones(65539, np.float32), 1, 2)
    with pytest.raises(EvLibraryError, match="640"):
        eng.load_resampler(t, 641, 2)
    with pytest.raises(EvLibraryError, match="640"):
        eng.load_resampler(t, 1, 0)
    with pytest.raises(EvLibraryError, match="not loaded"):
        eng.resample(x)
    eng.load_resampler(np.array([0.5], np.float32), 1, 1)                # up = down = 1 with one tap: a scaled copy
    y = R.signal("noise1", 2, 1500, seed=1).to(DEV)
    assert torch.equal(eng.resample(y), y * 0.5)
    eng.load_resampler(audio.resample_filter(1, 2), 1, 2)                # loading again replaces the filter
    fresh = engine_with(audio.resample_filter(1, 2), 1, 2)
    assert torch.equal(eng.resample(y), fresh.resample(y))
    with pytest.raises(EvLibraryError, match="GPU"):
        audio.resample(y.cpu(), 44100, 22050)
    eng.close()
    fresh.close()


def test_long_filters_take_the_fallback_paths():
    """Filters whose phase table or input span exceed the LDS budget of 16384 floats: the 256-output tile, the table
    and / or the samples read from global memory — every build of the kernel the parity cases do not reach.  Gated at 3x scipy's own
    float32 run on the same input, as the parity cases are, measured live (chains of up to 65537 taps round more than those of 21)."""
    for up, down, n_taps, L in ((640, 1, 65537, 37), (1, 40, 801, 50000), (3, 100, 20001, 40000), (1, 640, 12801, 20000), (1, 3, 65537, 1500)):
        g = np.random.default_rng(n_taps + up)
        taps = (g.standard_normal(n_taps) / np.sqrt(n_taps / up)).astype(np.float32)
        x = R.signal("noise1", 2, L, seed=L).numpy()
        ref = sps.resample_poly(x.astype(np.float64), up, down, axis=-1, window=taps.astype(np.float64) / up, padtype="constant")
        fmx, frms = errors(sps.resample_poly(x, up, down, axis=-1, window=taps / np.float32(up), padtype="constant"), ref)
        eng = engine_with(taps, up, down)
        got = eng.resample(torch.from_numpy(x).to(DEV)).cpu().numpy()
        eng.close()
        mx, rms = errors(got, ref)
        print(f"\nRSERR fallback {up}/{down} {n_taps} taps: scipy float32 max {fmx:.2e} rms {frms:.2e}  engine max {mx:.2e} rms {rms:.2e}")
        assert got.shape == ref.shape and mx <= 3 * fmx and rms <= 3 * frms, (up, down, n_taps, mx, rms, fmx, frms)


def _mel_like(B, Cn, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Cn, T, generator=g) * 2.1 - 5.5


def _row_sums64(mel, lens):
    m = mel.numpy().astype(np.float64)
    out = np.zeros((len(lens), 2))
    for b, n in enumerate(lens):
        if 1 <= n <= m.shape[2]:
            out[b] = [m[b, :, :n].sum(), (m[b, :, :n] ** 2).sum()]
    return out


@pytest.mark.parametrize("B,T,lens", [(5, 37, [37, 0, 1, 20, 36]), (2, 37, [38, 33]), (64, 516, None)])
def test_mel_stats_against_float64(B, T, lens):
    eng = Engine(0)
    if lens is None:
        lens = [int(v) for v in torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(2))]
        lens[0] = T
    mel = _mel_like(B, 80, T, seed=B + T)
    want = _row_sums64(mel, lens)
    a = eng.mel_stats(mel.to(DEV), torch.tensor(lens))
    n0 = eng.alloc_count()
    b = eng.mel_stats(mel.to(DEV), torch.tensor(lens))
    assert a.dtype == torch.float64 and tuple(a.shape) == (B, 2) and torch.equal(a, b), "two calls, the same bits"
    assert eng.alloc_count() == n0
    got = a.cpu().numpy()
    for r, n in enumerate(lens):
        if not 1 <= n <= T:
            assert got[r, 0] == 0.0 and got[r, 1] == 0.0, f"row {r} (len {n}) is written as zeros"
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"\nMELSTATS B{B} T{T}: max relative difference {rel[want != 0].max():.2e}")
    assert float(rel[want != 0].max()) <= 1e-9
    eng.close()


def test_data_statistics_over_two_batches():
    b1, l1 = _mel_like(4, 80, 50, seed=1), [50, 3, 27, 49]
    b2, l2 = _mel_like(3, 80, 33, seed=2), [33, 1, 16]
    got = audio.data_statistics([(b1.to(DEV), torch.tensor(l1)), (b2.to(DEV), torch.tensor(l2))], 80)
    s = _row_sums64(b1, l1).sum(0) + _row_sums64(b2, l2).sum(0)
    n = (sum(l1) + sum(l2)) * 80
    mean = s[0] / n
    std = float(np.sqrt(s[1] / n - mean ** 2))
    assert abs(got["mel_mean"] - mean) <= 1e-9 * abs(mean) and abs(got["mel_std"] - std) <= 1e-9 * std
    with pytest.raises(EvLibraryError):
        audio.data_statistics([(b1, torch.tensor(l1))], 80)


def _write_wav16(path, x, rate):
    q = np.round(np.clip(np.asarray(x, np.float64), -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(q.tobytes())


def test_recording_at_44100_hz_to_mel_and_cli(tmp_path):
    from emojivoice_amd.cli import cli

    n = 20001
    x = R.signal("noise1e-2", 1, n, seed=44)[0].numpy() * 10.0
    p = tmp_path / "rec.wav"
    _write_wav16(p, x, 44100)
    y = audio.load_audio(p, 22050, DEV)
    assert y.is_cuda and tuple(y.shape) == (1, (n + 1) // 2)
    samples, rate = audio.read_wav(p)
    ref = sps.resample_poly(samples.astype(np.float64), 1, 2, window=audio.resample_filter(1, 2).astype(np.float64) / 1, padtype="constant")
    mx, rms = errors(y[0].cpu().numpy(), ref)
    assert rate == 44100 and mx <= GATE_MAX and rms <= GATE_RMS
    frames = ((n + 1) // 2) // 256
    mel = audio.mel_spectrogram(y[:, : frames * 256].contiguous(), 1024, 80, 22050, 256, 1024, 0, 8000)
    assert tuple(mel.shape) == (1, 80, frames)
    cli(["--mel_from_wav", str(p)])
    saved = np.load(f"{p}.mel.npy")
    assert saved.shape == (80, frames) and np.array_equal(saved, mel[0].cpu().numpy())
    # the statistics of a two-file list: the same mel twice
    flist = tmp_path / "train.txt"
    flist.write_text(f"{p}|0|some text\nrec.wav|1|the same file, relative to the list\n", encoding="utf-8")
    cli(["--data_statistics", str(flist), "--batch_size", "1"])
    with open(f"{flist}.stats.json") as f:
        stats = json.load(f)
    m64 = saved.astype(np.float64)
    assert set(stats) == {"mel_mean", "mel_std"}
    assert abs(stats["mel_mean"] - m64.mean()) <= 1e-9 * abs(m64.mean()) and abs(stats["mel_std"] - m64.std()) <= 1e-8 * m64.std()


def test_cli_writes_the_wav_at_the_asked_rate(tmp_path):
    from emojivoice_amd.cli import cli

    out = tmp_path / "out"
    cli(["--synthetic", "--ids", "0 23 0 51 0 7 0 99 0", "--spk", "3", "--steps", "2", "--sample_rate", "44100", "--output_folder", str(out)])
    wavs = sorted(out.glob("*.wav"))
    assert len(wavs) == 1
    mel_len = np.load(str(wavs[0])[: -len(".wav")] + ".npy").shape[1]
    with wave.open(str(wavs[0]), "rb") as f:
        assert f.getframerate() == 44100 and f.getnchannels() == 1 and f.getsampwidth() == 3
        assert f.getnframes() == 2 * 256 * mel_len
    y, rate = audio.read_wav(wavs[0])
    assert rate == 44100 and np.isfinite(y).all() and float(np.abs(y).max()) > 0
