"""ev_modulation on the MI355X, through the C ABI, and what stands on it (audio.modulation, audio.voice_modulation,
audio.modulation_spectrum_distance, --voice_report --modulation, --evaluate_pairs --modulation).

Yardstick: tests/modulation_ref.py, the numpy restatement of the definition in include/emojivoice.h, in float64 (adding in the device's order)
and in longdouble.  The rule of every comparison (``check``):
  * d_count and d_weight EQUAL, the peak indices among them;
  * every entry of d_spec, d_peak and d_stat within 1e-9 max(|ref|, 1): the project's float64 margin;
  * exact zeros where the definition says zeros: the spectrum where no run resolves the frequency, a band without a candidate, the statistics
    without an analysed run, a row with a bad length.
The peak decisions compare powers that the device and the restatement form with different cospi / sinpi; tests/test_modulation_host.py holds every
case here to a decision margin of 1e-6 relative, four orders over what the library functions differ by.  Every case prints its worst figure.
Every raw call writes into buffers with 64-element sentinel margins (tests/analysis_gpu.py); NaN under a mask of ones lies behind every row's
length, so a read behind it would show as a dropped frame.
"""
import json

import numpy as np
import pytest
import torch

import analysis_gpu as A
import modulation_ref as R
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, _stream_ptr

pytestmark = pytest.mark.gpu

_REF, _CASES = {}, {}


def case(name):
    if not _CASES:
        _CASES.update(R.cases())
    return _CASES[name]


def ref_of(key, v, mask, lens, kw):
    """The restatements' results (float64, longdouble), computed once per case and never modified."""
    return A.frozen(_REF, key, lambda: (R.batch(v, mask, lens, **kw), R.batch(v, mask, lens, dtype=np.longdouble, **kw)))


def raw(eng, v, mask, lens, kw, null=(), **over):
    """ev_modulation into guarded buffers: (rc, spec, weight, peak, stat, count) on the host (peak None when NBAND == 0); an argument named in
    ``null`` is passed as NULL; ``over`` overrides B, K, F, NM, NBAND, nu0, dnu, min_run, min_cycles or bands as passed to the library (the
    buffers keep the sizes of ``kw``).  A failed call must have written nothing."""
    v = torch.as_tensor(np.asarray(v, dtype=np.float64)).to(DEV).contiguous()
    Bx, Kx, Fx = v.shape
    NM, NB = kw["NM"], len(kw["bands"])
    ba = np.ascontiguousarray(np.asarray(over.get("bands", kw["bands"]), dtype=np.int32).reshape(-1, 2))
    d_mask = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.uint8)).to(DEV).contiguous()
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    null = tuple(null) + (("peak",) if NB == 0 and "peak" not in null else ())
    out = A.Guarded({"spec": ((Bx, Kx, NM), torch.float64), "weight": ((Bx, Kx, NM), torch.int32), "peak": ((Bx, Kx, NB, 4), torch.float64),
                     "stat": ((Bx, Kx, 2), torch.float64), "count": ((Bx, Kx, 4 + NB), torch.int32)}, null)
    rc = eng.lib.ev_modulation(eng.h, None if "v" in null else v.data_ptr(), None if d_mask is None else d_mask.data_ptr(),
                               None if d_len is None else d_len.data_ptr(), over.get("B", Bx), over.get("K", Kx), over.get("F", Fx),
                               float(over.get("nu0", kw["nu0"])), float(over.get("dnu", kw["dnu"])), over.get("NM", NM),
                               over.get("min_run", kw["min_run"]), float(over.get("min_cycles", kw["min_cycles"])),
                               None if "band" in null or not len(ba) else ba.ctypes.data, over.get("NBAND", len(ba)), out.ptr("spec"), out.ptr("weight"),
                               out.ptr("peak"), out.ptr("stat"), out.ptr("count"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def check(dev, ref, what):
    """The comparison rule of the module docstring; prints the figures before it asserts."""
    sp, wg, pk, st, ct = dev
    r64, rld = ref
    assert np.array_equal(r64["count"], rld["count"]) and np.array_equal(r64["weight"], rld["weight"]), \
        f"{what}: the float64 and longdouble restatements disagree on a count, a weight or a peak index"
    NB = r64["peak"].shape[2]
    pk = np.zeros(r64["peak"].shape) if pk is None else pk
    e_sp, e_pk, e_st = R.err(sp, r64["spec"]), R.err(pk, r64["peak"].astype(np.float64)), R.err(st, r64["stat"])
    ld = max(R.err(r64["spec"], rld["spec"].astype(np.float64)), R.err(r64["peak"], rld["peak"].astype(np.float64)),
             R.err(r64["stat"], rld["stat"].astype(np.float64)))
    print(f"\nmodulation {what}: worst err {max(e_sp, e_pk, e_st):.3e} (d_spec {e_sp:.1e}, d_peak {e_pk:.1e}, d_stat {e_st:.1e}; gate {R.TOL:g})  "
          f"float64 against longdouble {ld:.3e}  counts differing {int((ct != r64['count']).sum())}  weights differing {int((wg != r64['weight']).sum())}  "
          f"contours {ct.shape[0] * ct.shape[1]}, analysed runs {int(r64['count'][..., 2].sum())} over {int(r64['count'][..., 3].sum())} frames, "
          f"dropped {int(r64['count'][..., 1].sum())}, peaks {int((r64['count'][..., 4:] >= 0).sum())} of {ct.shape[0] * ct.shape[1] * NB} bands")
    assert np.array_equal(ct, r64["count"]), f"{what}: d_count (the peak indices among them)"
    assert np.array_equal(wg, r64["weight"]), f"{what}: d_weight"
    assert np.isfinite(sp).all() and np.isfinite(pk).all() and np.isfinite(st).all(), f"{what}: every output is finite"
    assert max(e_sp, e_pk, e_st) <= R.TOL, f"{what}: d_spec, d_peak, d_stat"
    assert not sp[wg == 0].any(), f"{what}: exact zeros where no run resolves the frequency"
    assert not pk[ct[..., 4:] < 0].any(), f"{what}: exact zeros in a band without a candidate"
    assert not st[ct[..., 2] == 0].any(), f"{what}: exact zeros without an analysed run"


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


def run_case(eng, name):
    v, mask, lens, kw = case(name)
    rc, *dev = raw(eng, v, mask, lens, kw)
    assert rc == 0, err_of(eng)
    ref = ref_of(name, v, mask, lens, kw)
    check(dev, ref, f"{name} {v.shape} lens {lens} NM {kw['NM']} bands {kw['bands']}")
    return v, mask, lens, kw, dev, ref


# ---- 1. every case against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", R.SHAPES)
def test_shapes_against_the_restatement(eng, F):
    """(3, 4, F) with lengths F, F - 1 and (F + 1) / 2: the contour kinds (sinusoid on a line, two sinusoids, random walk, constant, integers with
    plateaus, signed zeros) and the mask kinds (ones, random runs, alternating, zeros, one run of exactly min_run, one of min_run - 1) cycle over
    the contours; F around one and four tiles of 256 and around a wave of 64; NM cycles over 1, 3, 64, 65, 128 and NBAND over 0, 1, 4."""
    run_case(eng, f"F{F}")


def test_one_run_of_4096_frames(eng):
    """One run across every tile of the scan, 64 terms per slot of the per-run sums and 1024 per chain; NM = 128 takes two passes of phase B."""
    v, mask, lens, kw, (sp, wg, pk, st, ct), _ = run_case(eng, "run4096")
    assert ct[0, 0, :4].tolist() == [4096, 0, 1, 4096] and (wg[0, 0] == 4096).all()
    assert ct[0, 0, 4] == -1 and ct[0, 0, 7] == -1 and ct[0, 0, 5] >= 1, "bands (0, 1) and (127, 128) can hold no candidate"


def test_a_run_that_puts_a_frequency_exactly_on_min_cycles(eng):
    v, mask, lens, kw, (sp, wg, pk, st, ct), _ = run_case(eng, "boundary")
    nu = R.grid(kw["nu0"], kw["dnu"], kw["NM"])
    assert nu[12] * 32.0 == kw["min_cycles"], "the run of 32 frames holds exactly two cycles of nu_12"
    assert wg[0, 0, 8] == 0 and wg[0, 0, 9] == 40 and wg[0, 0, 11] == 40 and wg[0, 0, 12] == 72, ">= resolves the boundary itself"


def test_non_finite_values_under_the_mask_are_dropped_and_counted(eng):
    v, mask, lens, kw, (sp, wg, pk, st, ct), _ = run_case(eng, "nonfinite")
    assert ct[0, 0, 1] == 5 and ct[0, 0, 0] == v.shape[2] - 6 and ct[0, 0, 2] == 5, "five dropped frames and a masked NaN split the row into runs"
    assert ct[1, 1].tolist() == [0, v.shape[2], 0, 0, -1] and not sp[1, 1].any()


def test_lengths_0_1_F_and_the_two_bad_ones(eng):
    v, mask, lens, kw, (sp, wg, pk, st, ct), _ = run_case(eng, "lengths")
    assert lens == [0, 1, 65, 66, -1]
    for b in (3, 4):
        assert not ct[b].any() and not sp[b].any() and not pk[b].any(), "d_len F + 1 and -1: rows of zeros, the peak indices included"
    assert ct[0, 0].tolist() == [0, 0, 0, 0, -1, -1, -1, -1] and ct[1, 0].tolist() == [1, 0, 0, 0, -1, -1, -1, -1]
    assert ct[2, 0, 0] == 65 and ct[2, 0, 2] == 1


@pytest.mark.parametrize("name", ("null-mask-null-lengths", "three-runs"))
def test_more_cases(eng, name):
    run_case(eng, name)


def test_a_band_without_a_candidate_and_a_peak_whose_neighbours_lie_outside_its_band(eng):
    v, mask, lens, kw, (sp, wg, pk, st, ct), _ = run_case(eng, "neighbours-outside")
    assert kw["bands"][0] == (20, 21) and ct[0, 0, 4:].tolist() == [20, -1, -1, 20]
    nu = kw["nu0"] + 20 * kw["dnu"]
    assert abs(pk[0, 0, 0, 0] - nu) < 0.1 * kw["dnu"] and abs(pk[0, 0, 0, 1] - 0.4) < 0.004, "rate and extent of the on-grid sinusoid"
    assert pk[0, 0, 0, 2] == sp[0, 0, 20] and np.array_equal(pk[0, 0, 0, :2], pk[0, 0, 3, :2])


def test_the_mutants_differ_from_the_device(eng):
    """What the host test shows of the restatement holds of the device: on its named case the device sides with the definition, not the mutant."""
    for mutant, (name, bk, what) in R.MUTANT_SHOWS.items():
        v, mask, lens, kw = case(name)
        rc, *dev = raw(eng, v, mask, lens, kw)
        assert rc == 0
        got = dict(zip(("spec", "weight", "peak", "stat", "count"), dev))[what][bk].astype(np.float64)
        bad = R.batch(v, mask, lens, mutant=mutant, **kw)[what][bk].astype(np.float64)
        good = ref_of(name, v, mask, lens, kw)[0][what][bk].astype(np.float64)
        assert R.err(got, good) <= R.TOL and R.err(got, bad) > 1e-6, (mutant, R.err(got, good), R.err(got, bad))


# ---- 2. the identities -------------------------------------------------------------------------------------------------------------------------------
def test_alone_in_a_batch_at_another_k_as_a_prefix_twice_and_under_every_arithmetic_give_the_same_bits(eng):
    v1, m1, _, kw = case("identity")
    c, cm, F = v1[0, 0], m1[0, 0], v1.shape[2]
    n0 = eng.alloc_count()
    _, _, _, _, alone, _ = run_case(eng, "identity")
    assert alone[4][0, 0, 2] > 3 and alone[4][0, 0, 4] >= 0
    rc, *again = raw(eng, c[None, None], cm[None, None], None, kw)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(alone, again)), "two calls"
    vb, mb = R.make(3, 4, F, seed=22, min_run=4)
    vb[1, 2], mb[1, 2] = c, cm
    vb[2, 0], mb[2, 0] = c, cm
    rc, *batch = raw(eng, vb, mb, None, kw)
    assert rc == 0
    Fp = 400
    vp, mp = R.make(2, 3, Fp, seed=23, min_run=4, lens=[Fp, F])
    vp[1, 1, :F], mp[1, 1, :F] = c, cm                                   # (NaN under mask 1 lies behind d_len = 257)
    assert np.isnan(vp[1, 1, F:]).all() and (mp[1, 1, F:] == 1).all()
    rc, *prefix = raw(eng, vp, mp, [Fp, F], kw)
    assert rc == 0
    for what, other, at in (("inside a batch", batch, (1, 2)), ("at another k", batch, (2, 0)), ("the d_len prefix of a longer F", prefix, (1, 1))):
        for i, out in enumerate(("d_spec", "d_weight", "d_peak", "d_stat", "d_count")):
            assert np.array_equal(alone[i][0, 0], other[i][at]), f"{out}: alone against {what}"
    base = eng.lib.ev_get_arithmetic(eng.h)
    try:
        for setting in (0, 3, 6):
            eng.set_arithmetic(setting)
            rc, *got = raw(eng, vb, mb, None, kw)
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, batch)), f"arithmetic {setting}"
    finally:
        eng.set_arithmetic(base)
    torch.cuda.synchronize()
    assert eng.alloc_count() == n0, "ev_alloc_count never moves"


def test_no_allocation_and_capturable():
    e = Engine(0)
    v, mask, lens, kw = case("F257")
    kw = dict(kw, NM=64, bands=R.bands_for(64, 4))
    args = (kw["nu0"], kw["dnu"], kw["NM"], kw["min_run"], kw["min_cycles"], kw["bands"])
    vd = torch.from_numpy(v).to(DEV)
    md = torch.from_numpy(mask).to(DEV)
    n0 = e.alloc_count()
    ref = e.modulation(vd, md, lens, *args)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        e.modulation(vd, md, ld, *args)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = e.modulation(vd, md, ld, *args)
        for t in out:
            t.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b), "the replay equals the eager call"
    r64 = ref_of("F257-64", v, mask, lens, kw)[0]
    assert np.array_equal(out[4].cpu().numpy(), r64["count"]) and np.array_equal(out[1].cpu().numpy(), r64["weight"])
    assert e.alloc_count() == n0
    e.close()


# ---- 3. limits -----------------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
BAD_CALL = [
    ("B=", dict(B=0)), ("B=", dict(B=65536)), ("K=", dict(K=0)), ("K=", dict(K=65536)), ("F=", dict(F=0)), ("F=", dict(F=4097)),
    ("NM=", dict(NM=0)), ("NM=", dict(NM=129)), ("nu0=", dict(nu0=0.0)), ("nu0=", dict(nu0=NAN)), ("nu0=", dict(nu0=INF)), ("nu0=", dict(nu0=-0.1)),
    ("dnu=", dict(dnu=0.0)), ("dnu=", dict(dnu=NAN)), ("dnu=", dict(dnu=INF)), ("over the limit 0.5", dict(nu0=0.4, dnu=0.02)),
    ("min_run=", dict(min_run=2)), ("min_run=", dict(min_run=17)), ("min_cycles=", dict(min_cycles=-1.0)), ("min_cycles=", dict(min_cycles=NAN)),
    ("min_cycles=", dict(min_cycles=INF)), ("NBAND=", dict(NBAND=-1)), ("NBAND=", dict(NBAND=5)), ("band must", dict(null=("band",))),
    ("band[1]", dict(bands=((0, 9), (5, 5)))), ("band[0]", dict(bands=((-1, 3), (0, 9)))), ("band[1]", dict(bands=((0, 9), (3, 10)))),
    ("d_v", dict(null=("v",))), ("d_spec", dict(null=("spec",))), ("d_weight", dict(null=("weight",))), ("d_peak", dict(null=("peak",))),
    ("d_stat", dict(null=("stat",))), ("d_count", dict(null=("count",))),
]


@pytest.mark.parametrize("word,over", BAD_CALL, ids=[f"{w.strip('=').replace(' ', '-')}-{i}" for i, (w, _) in enumerate(BAD_CALL)])
def test_each_limit_fails_with_a_message_naming_it_and_writes_nothing(eng, word, over):
    over = dict(over)
    null = over.pop("null", ())
    kw = dict(nu0=0.02, dnu=0.01, NM=9, min_run=4, min_cycles=2.0, bands=((0, 9), (2, 5)))
    n0 = eng.alloc_count()
    rc, *_ = raw(eng, np.zeros((2, 2, 16)), None, None, kw, null, **over)  # (a failed call writes nothing: raw checks that)
    msg = err_of(eng)
    assert rc != 0 and "ev_modulation" in msg and word in msg, msg
    assert eng.alloc_count() == n0


# ---- 4. through audio ----------------------------------------------------------------------------------------------------------------------------------
def test_audio_modulation_equals_the_raw_call(eng):
    v64, full, lens, kw = case("audio")
    v, mask = v64.astype(np.float32), full[:, :1, :] != 0                # float32 contours (exactly), (3, 1, F): one mask per row
    assert np.array_equal(v.astype(np.float64), v64, equal_nan=True)
    vd, md = torch.from_numpy(v).to(DEV), torch.from_numpy(mask).to(DEV)
    rate = R.AUDIO_RATE
    out = audio.modulation(vd, md, lens, rate, bands_hz=((4.0, 12.0), (2.0, 8.0)))
    nu0, dnu, NM = audio.modulation_grid(22050, 256)
    assert NM == 121 and out["spectrum"].shape == (3, 2, 121) and out["rate_hz"].shape == (3, 2, 2)
    assert (nu0, dnu, NM) == (kw["nu0"], kw["dnu"], kw["NM"])
    _, _, _, _, (sp, wg, pk, st, ct), _ = run_case(eng, "audio")
    assert np.array_equal(out["spectrum"].cpu().numpy(), sp) and np.array_equal(out["weight"].cpu().numpy(), wg)
    assert np.array_equal(out["peak_index"].cpu().numpy(), ct[..., 4:]) and np.array_equal(out["runs"].cpu().numpy(), ct[..., 2])
    has = ct[..., 4:] >= 0
    assert has.any() and not has[2].any()
    for key, want in (("rate_hz", pk[..., 0] * rate), ("extent", pk[..., 1]), ("band_mean", pk[..., 2]), ("prominence_db", 10.0 * np.log10(np.where(has, pk[..., 3], 1.0)))):
        got = out[key].cpu().numpy()
        assert np.array_equal(np.isnan(got), ~has) and np.allclose(got[has], want[has], rtol=1e-14, atol=0), key
    ran = ct[..., 2] > 0
    assert np.array_equal(np.isnan(out["residual_variance"].cpu().numpy()), ~ran) and np.array_equal(out["residual_variance"].cpu().numpy()[ran], st[..., 0][ran])
    assert abs(out["frequencies_hz"][24].item() - 4.0) < 1e-12 and abs(out["frequencies_hz"][-1].item() - 16.0) < 1e-12
    one = audio.modulation(vd[0, 0], md[0, 0], bands_hz=((4.0, 12.0),))
    assert one["spectrum"].shape == (1, 1, 121) and torch.equal(one["spectrum"][0, 0], out["spectrum"][0, 0])


def vibrato_vowel(sr=22050, rate_hz=5.5, extent_st=0.4, f0=140.0, segments=(0.9, 0.7, 0.8), gap=0.15):
    """A harmonic tone whose f0 swings by +-extent_st semitones at rate_hz, in voiced segments separated by silence; float32, peak about 0.5."""
    n_seg = [int(s * sr) for s in segments]
    n_gap = int(gap * sr)
    total = sum(n_seg) + n_gap * (len(n_seg) + 1)
    t = np.arange(total) / sr
    f = f0 * 2.0 ** (extent_st * np.sin(2 * np.pi * rate_hz * t) / 12.0)
    phase = 2 * np.pi * np.cumsum(f) / sr
    y = sum(np.sin(h * phase) / h for h in range(1, 11))
    env = np.zeros(total)
    at = n_gap
    for n in n_seg:
        env[at: at + n] = np.minimum(1.0, np.minimum(np.arange(n), np.arange(n)[::-1]) / (0.01 * sr))
        at += n + n_gap
    return (0.5 * y * env / np.max(np.abs(y))).astype(np.float32)


def test_voice_modulation_finds_the_vibrato_of_a_synthetic_vowel():
    """Through pitch_yin and auditory: the tremor figures are the restatement's on the device's own f0 contour (1e-9), and they are the vibrato
    that was put in: 5.5 Hz within 0.15 Hz, and between 0.7 and 1.05 of the 0.4 semitones: a pitch frame averages the swing over about 54 ms
    (1024 samples and the lag), which leaves sinc(pi 0.054 rate) of it, 0.86 at 5.5 Hz and 0.78 at 7 Hz.  The restatement alone recovers the
    extent of a clean contour within 1 % (tests/test_modulation_host.py)."""
    y = vibrato_vowel()
    x = torch.from_numpy(np.stack([y, 0.7 * y])).to(DEV)
    lens = [len(y), len(y) - 5000]
    x[1, lens[1]:] = 0.0
    pitch = audio.pitch_yin(x, lengths=lens)
    au = audio.auditory(x, lengths=lens)
    nf = [-(-n // 256) for n in lens]
    vm = audio.voice_modulation(pitch, au, nf)
    assert set(audio.VOICE_MODULATION_FIGURES) <= set(vm)
    voiced = pitch["voiced"].cpu().numpy() & (np.arange(pitch["f0"].shape[1])[None, :] < np.array(nf)[:, None])
    st = (12.0 * torch.log2(torch.where(torch.from_numpy(voiced).to(DEV), pitch["f0"].to(torch.float64), torch.full((), 27.5, dtype=torch.float64, device=DEV))
                            / 27.5)).cpu().numpy()
    nu0, dnu, NM = audio.modulation_grid(22050, 256)
    ref = R.batch(st[:, None, :], voiced[:, None, :].astype(np.uint8), nf, nu0=nu0, dnu=dnu, NM=NM, min_run=18, min_cycles=2.0, bands=((24, 89),))
    rate, ext = vm["tremor_rate_hz"].cpu().numpy(), vm["tremor_extent_st"].cpu().numpy()
    want_rate, want_ext = ref["peak"][:, 0, 0, 0] * 22050.0 / 256.0, ref["peak"][:, 0, 0, 1]
    print(f"\nmodulation voice_modulation: tremor {rate.tolist()} Hz, {ext.tolist()} st (put in: 5.5 Hz, 0.4 st), prominence "
          f"{vm['tremor_prominence_db'].cpu().numpy().round(1).tolist()} dB; against the restatement {R.err(rate, want_rate):.1e} / {R.err(ext, want_ext):.1e}; "
          f"analysed runs {vm['f0_semitones']['runs'].tolist()}, rhythm {vm['rhythm_rate_hz'].cpu().numpy().tolist()} Hz, "
          f"depth {vm['rhythm_depth'].cpu().numpy().tolist()}")
    assert (ref["count"][:, 0, 2] >= 2).all(), "several voiced runs are analysed"
    assert np.array_equal(vm["f0_semitones"]["peak_index"][:, 0].cpu().numpy(), ref["count"][:, 0, 4])
    assert R.err(rate, want_rate) <= R.TOL and R.err(ext, want_ext) <= R.TOL
    assert (np.abs(rate - 5.5) < 0.15).all() and (ext > 0.7 * 0.4).all() and (ext < 1.05 * 0.4).all()
    assert (vm["tremor_prominence_db"].cpu().numpy() > 3.0).all(), "the peak holds at least twice the mean power of its band"


def test_modulation_spectrum_distance_of_a_mel_and_its_moving_average():
    g = np.random.default_rng(41)
    T, lens = 400, [400, 330]
    mel = np.cumsum(g.standard_normal((2, 80, T)), axis=2) * 0.1 + g.standard_normal((2, 80, T)) * 0.3
    ker = np.ones(5) / 5.0
    smooth = np.stack([[np.convolve(row, ker, mode="same") for row in m] for m in mel])
    a, b = torch.from_numpy(mel).float().to(DEV), torch.from_numpy(smooth).float().to(DEV)
    same = audio.modulation_spectrum_distance(a, a, lens, lens)
    assert same["ms_distortion_db"].tolist() == [0.0, 0.0] and same["ms_shift_db"].tolist() == [0.0, 0.0] and (same["pairs"] > 0).all()
    d = audio.modulation_spectrum_distance(a, b, lens, lens)
    nu0, dnu, NM = audio.modulation_grid(22050, 256, *audio.MS_DISTANCE_GRID_HZ)
    assert NM == 125
    sides = []
    for m in (a, b):
        cep = audio.mel_cepstrum(m, 13).double().cpu().numpy()
        sides.append(R.batch(cep, None, lens, nu0=nu0, dnu=dnu, NM=NM, min_run=18, min_cycles=2.0))
    both = (sides[0]["weight"] > 0) & (sides[1]["weight"] > 0)
    diff = np.where(both, 10.0 * np.log10(np.where(both, sides[1]["spec"], 1.0)) - 10.0 * np.log10(np.where(both, sides[0]["spec"], 1.0)), 0.0)
    n = both.sum(axis=(1, 2))
    want_shift, want_dist = diff.sum(axis=(1, 2)) / n, np.sqrt((diff * diff).sum(axis=(1, 2)) / n)
    got_shift, got_dist = d["ms_shift_db"].cpu().numpy(), d["ms_distortion_db"].cpu().numpy()
    print(f"\nmodulation spectrum distance of a mel and its 5-frame moving average: shift {got_shift.tolist()} dB, distortion {got_dist.tolist()} dB over "
          f"{d['pairs'].tolist()} terms; against the restatement {R.err(got_shift, want_shift):.1e} / {R.err(got_dist, want_dist):.1e}")
    assert np.array_equal(d["pairs"].cpu().numpy(), n)
    assert (got_shift < -1.0).all(), "the smoothed side has less modulation power"
    assert R.err(got_shift, want_shift) <= R.TOL and R.err(got_dist, want_dist) <= R.TOL


# ---- 5. the CLI -----------------------------------------------------------------------------------------------------------------------------------------
def _wavs(tmp_path):
    import voice_stubs
    from emojivoice_amd import cli

    y = vibrato_vowel()
    sig = {"a.wav": y, "b.wav": vibrato_vowel(rate_hz=7.0, extent_st=0.25, f0=180.0, segments=(1.0, 0.9)),
           "c.wav": (0.01 * np.random.default_rng(22).standard_normal(6000)).astype(np.float32)}      # (noise alone: no voiced frame)
    flist = voice_stubs.filelist(tmp_path, sig)
    for name, s in sig.items():
        cli.write_wav_pcm16(tmp_path / name, s, 22050)
    return cli, flist, sig


def test_voice_report_with_modulation(tmp_path):
    cli, flist, sig = _wavs(tmp_path)
    plain = cli.cli(["--voice_report", str(flist), "--batch_size", "2"])
    with open(f"{flist}.voice.json", "rb") as f:
        plain_bytes = f.read()
    rep = cli.cli(["--voice_report", str(flist), "--batch_size", "2", "--modulation"])
    with open(f"{flist}.voice.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert [set(f_) - {"modulation"} for f_ in saved["files"]] == [set(f_) for f_ in plain["files"]] and "modulation" not in plain["files"][0]
    assert all(saved["files"][i][k] == plain["files"][i][k] for i in range(3) for k in plain["files"][i]), "the flag changes none of the other figures"
    assert set(saved["overall"]) - {"modulation"} == set(plain["overall"]) and set(saved) == set(plain)
    a, b, c = (f_["modulation"] for f_ in saved["files"])
    print(f"\nmodulation --voice_report --modulation: {a} / {b} / {c}")
    assert all(tuple(m) == audio.VOICE_MODULATION_FIGURES for m in (a, b, c))
    assert abs(a["tremor_rate_hz"] - 5.5) < 0.15 and 0.7 * 0.4 < a["tremor_extent_st"] < 1.05 * 0.4
    assert abs(b["tremor_rate_hz"] - 7.0) < 0.15 and 0.7 * 0.25 < b["tremor_extent_st"] < 1.05 * 0.25      # (the tracker's frame: the vowel test)
    assert c["tremor_rate_hz"] is None and c["tremor_extent_st"] is None and c["f0_residual_sd_st"] is None, "noise: no voiced run, nulls"
    s7, s12 = saved["speakers"]["7"]["modulation"], saved["speakers"]["12"]["modulation"]
    assert s7["tremor_rate_hz"]["files"] == 2 and abs(s7["tremor_rate_hz"]["mean"] - 0.5 * (a["tremor_rate_hz"] + b["tremor_rate_hz"])) < 1e-12
    assert s12["tremor_rate_hz"] == {"mean": None, "files": 0} and saved["overall"]["modulation"]["tremor_rate_hz"] == s7["tremor_rate_hz"]
    again = cli.cli(["--voice_report", str(flist), "--batch_size", "2"])
    with open(f"{flist}.voice.json", "rb") as f:
        assert f.read() == plain_bytes and again == plain, "without the flag the report is what it was"
    both = cli.cli(["--voice_report", str(flist), "--batch_size", "3", "--modulation", "--auditory"])
    assert both["files"][0]["modulation"] == a, "on --auditory's frames, in one batch of three: the same figures"


def test_evaluate_pairs_with_modulation(tmp_path):
    cli, flist, sig = _wavs(tmp_path)
    y = sig["a.wav"]
    cli.write_wav_pcm16(tmp_path / "a_syn.wav", vibrato_vowel(extent_st=0.2), 22050)
    cli.write_wav_pcm16(tmp_path / "b_syn.wav", sig["b.wav"][: len(sig["b.wav"]) - 3000], 22050)
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(f"{tmp_path / 'a.wav'}|{tmp_path / 'a_syn.wav'}|7\n{tmp_path / 'b.wav'}|{tmp_path / 'b_syn.wav'}|7\n", encoding="utf-8")
    plain = cli.cli(["--evaluate_pairs", str(pairs), "--batch_size", "2"])
    with open(f"{pairs}.eval.json", "rb") as f:
        plain_bytes = f.read()
    rep = cli.cli(["--evaluate_pairs", str(pairs), "--batch_size", "2", "--modulation"])
    with open(f"{pairs}.eval.json") as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(rep))
    assert all({k: v for k, v in p.items() if k != "modulation"} == q for p, q in zip(saved["pairs"], plain["pairs"])), "the flag changes no other figure"
    m0, m1 = saved["pairs"][0]["modulation"], saved["pairs"][1]["modulation"]
    print(f"\nmodulation --evaluate_pairs --modulation: {m0} / {m1}")
    assert tuple(m0) == ("recorded", "synthesised", "delta", "ms_distortion_db", "ms_shift_db")
    assert tuple(m0["recorded"]) == audio.VOICE_MODULATION_FIGURES
    assert abs(m0["delta"]["tremor_extent_st"] + 0.2) < 0.06, "the synthesised side has half the vibrato"
    assert abs(m0["delta"]["tremor_extent_st"] - (m0["synthesised"]["tremor_extent_st"] - m0["recorded"]["tremor_extent_st"])) < 1e-15
    assert m1["ms_distortion_db"] is not None and m1["ms_distortion_db"] < 3.0 and abs(m1["delta"]["tremor_rate_hz"]) < 0.1, "a truncated copy is close"
    o = saved["overall"]["modulation"]
    assert o["ms_shift_db"]["pairs"] == 2 and abs(o["ms_shift_db"]["mean"] - 0.5 * (m0["ms_shift_db"] + m1["ms_shift_db"])) < 1e-12
    assert abs(o["tremor_extent_st"]["mean_delta"] - 0.5 * (m0["delta"]["tremor_extent_st"] + m1["delta"]["tremor_extent_st"])) < 1e-12
    assert saved["speakers"]["7"]["modulation"] == o
    cli.cli(["--evaluate_pairs", str(pairs), "--batch_size", "2"])
    with open(f"{pairs}.eval.json", "rb") as f:
        assert f.read() == plain_bytes, "without the flag the report is what it was"


def test_modulation_without_a_report_is_rejected():
    import argparse

    from emojivoice_amd import cli

    with pytest.raises(AssertionError, match="--modulation"):
        cli.validate_args(argparse.Namespace(modulation=True, evaluate_pairs=None, voice_report=None, sample_rate=None, prepare_dataset=None))
