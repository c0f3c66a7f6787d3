"""ev_pyin_observe and ev_pyin_decode on the MI355X, through the C ABI.

Yardstick: tests/pyin_ref.py, the numpy float64 restatement of the header's semantics (librosa is not a dependency).

Observation.  The device forms d' as ev_pitch_yin does (the same exact float64 squares summed in another order than numpy's: a few 2^-53
relative), its exp, log2 and divisions differ from numpy's by an ulp or so, and P_k is a sum of at most n_thr = 100 positive terms that
are each at most w_t <= 0.07: |obs - ref| <= 1e-9 and |pv - ref| <= 1e-9, absolute, seven orders above that rounding, on every frame that is
not FRAGILE (pyin_ref.fragile_frames: a trough's d' within 1e-7 of a threshold, a trough test within 1e-7 relative of flipping, a
candidate within 1e-7 of the border between two bins: there a rounding may move a whole P_k).  Fragile frames are held to obs >= 0 and
0 <= pv <= 1 only; tests/test_pyin_host.py asserts on the CPU that they are at most 2 % of each input's frames (they are none).

Decoding is fed the REFERENCE's obs and pv, so it stands alone: d_loglik within 1e-9 relative of the reference's optimum; the score of the
device's path under the reference model (pyin_ref.path_score) within 1e-9 relative of it; the voiced flag, and the bin where voiced, EQUAL
to the reference's on every frame, a differing frame being tolerated only where the two paths' scores agree to 1e-12 relative and on at
most 1 % of the frames.  The bin of an unvoiced frame is compared through the score only: unvoiced emissions are equal over the bins by
construction, so where an unvoiced stretch sits is decided by roundings of the host tables alone.

Every raw call writes into buffers with sentinel margins (tests/analysis_gpu.py); inputs carry loud garbage behind each row's d_len samples.
Times: not gated here (tools/pyin_bench.py).
"""
import math

import numpy as np
import pytest
import torch

import analysis_gpu as A
import pitch_ref as P
import pyin_ref as Y
from analysis_gpu import DEV, err_of
from emojivoice_amd import audio
from emojivoice_amd._lib import Engine, EvLibraryError, _stream_ptr

pytestmark = pytest.mark.gpu

GARBAGE = P.GARBAGE
_REF = {}


def cached(key, make):
    """A reference result, computed once and never modified."""
    return A.frozen(_REF, key, make)


def observed(name):
    x, lens, kw = {"std": Y.std_case, "small": Y.small_case}[name]()
    return x, lens, kw, cached(("observe", name), lambda: Y.observe(x, lens, **kw))


def raw_observe(eng, x, lens, frame_length, hop_length, tau_min, tau_max, sr, fmin, bins_per_octave, n_bins, w, boltzmann, no_trough_prob):
    """ev_pyin_observe into guarded buffers: (rc, obs (B, F, n_bins), pv (B, F)) on the host."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    B, L = x.shape
    F = -(-L // hop_length)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = A.Guarded({"obs": ((B, F, n_bins), torch.float64), "pv": ((B, F), torch.float64)})
    rc = eng.lib.ev_pyin_observe(eng.h, x.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, frame_length, hop_length, tau_min, tau_max,
                                 float(sr), float(fmin), bins_per_octave, n_bins, w.ctypes.data, w.size, boltzmann, no_trough_prob,
                                 out.ptr("obs"), out.ptr("pv"), _stream_ptr())
    return (rc, *out.collect(rc).values())


def raw_decode(eng, obs, pv, lens, L, hop_length, tables):
    """ev_pyin_decode into guarded buffers: (rc, state (B, F) int32, loglik (B,)) on the host."""
    obs_d = torch.as_tensor(np.array(obs, dtype=np.float64)).to(DEV)
    pv_d = torch.as_tensor(np.array(pv, dtype=np.float64)).to(DEV)
    B, F, nb = obs_d.shape
    assert F == -(-L // hop_length)
    d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = A.Guarded({"back": ((B, F, 2 * nb), torch.uint8), "state": ((B, F), torch.int32), "loglik": ((B,), torch.float64)}, fills={"back": 201})
    lt, lz = np.ascontiguousarray(tables["log_tri"]), np.ascontiguousarray(tables["log_Z"])
    rc = eng.lib.ev_pyin_decode(eng.h, obs_d.data_ptr(), pv_d.data_ptr(), None if d_len is None else d_len.data_ptr(), B, L, hop_length, nb,
                                tables["R"], lt.ctypes.data, lz.ctypes.data, tables["log_stay"], tables["log_switch"], out.ptr("back"),
                                out.ptr("state"), out.ptr("loglik"), _stream_ptr())
    got = out.collect(rc)
    return rc, got["state"], got["loglik"]


@pytest.fixture(scope="module")
def eng():
    yield from A.one_engine()


# ---- 1. the observation against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["std", "small"])
def test_observe_parity_with_the_restatement(eng, name):
    x, lens, kw, ref = observed(name)
    rc, obs, pv = raw_observe(eng, x, lens, **kw)
    assert rc == 0, err_of(eng)
    keep = ~ref["fragile"]
    e_o = float(np.max(np.abs(obs - ref["obs"])[keep])) if keep.any() else 0.0
    e_p = float(np.max(np.abs(pv - ref["pv"])[keep])) if keep.any() else 0.0
    print(f"\nPYIN observe {name}: frames {keep.size} fragile {int((~keep).sum())} |obs - ref| {e_o:.3e} |pv - ref| {e_p:.3e} max pv {float(pv.max()):.6f}")
    assert int((~keep).sum()) <= 0.02 * keep.size
    assert np.all(obs >= 0) and np.all(pv >= 0) and np.all(pv <= 1), "every frame, the fragile ones included"
    assert e_o <= 1e-9, "d_obs"
    assert e_p <= 1e-9, "d_pv"
    assert float(ref["pv"].max()) > 0.9 and int((ref["obs"] > 0).sum()) >= int((ref["pv"] > 0).sum()) >= 0.5 * keep.size, "the case is not empty"
    for b, n in enumerate(lens):
        nf = -(-n // kw["hop_length"])
        assert not obs[b, nf:].any() and not pv[b, nf:].any(), "frames past the row are zeros"


# ---- 2. the decoding against the restatement, on the restatement's observation -----------------------------------------------------------------
def decode_cases():
    """name -> (obs (B, F, n_bins), pv (B, F), lens, L, H, tables)."""
    def from_observation(name):
        x, lens, kw, ref = observed(name)
        return ref["obs"], ref["pv"], lens, x.shape[1], kw["hop_length"], Y.tables_for(kw)

    def random(nb, R, F, seed, lens):
        obs, pv, tables = Y.random_model(nb, R, F, seed)
        obs2, pv2, _ = Y.random_model(nb, R, F, seed + 100)
        return np.stack([obs, obs2]), np.stack([pv, pv2]), lens, F * 64, 64, tables

    return {
        "std": lambda: from_observation("std"),
        "small": lambda: from_observation("small"),
        "74-states-R-beyond-the-bins": lambda: random(37, 40, 9, 21, [9 * 64, 61]),        # 2 n_bins no multiple of 64; R >= n_bins; a one-frame row
        "R0": lambda: random(37, 0, 9, 22, [9 * 64 - 5, 9 * 64]),
        "two-states-per-thread": lambda: random(600, 5, 6, 23, [6 * 64, 3 * 64]),         # 1200 states on 1024 threads; log_Z in its compressed form
    }


@pytest.mark.parametrize("name", ["std", "small", "74-states-R-beyond-the-bins", "R0", "two-states-per-thread"])
def test_decode_parity_with_the_restatement(eng, name):
    obs, pv, lens, L, H, tables = cached(("decode-in", name), decode_cases()[name])
    nb = tables["n_bins"]
    F = obs.shape[1]
    nfs = [-(-n // H) for n in lens]
    ref = cached(("decode-ref", name), lambda: [Y.viterbi_fast(obs[b, :nf], pv[b, :nf], tables) for b, nf in enumerate(nfs)])
    rc, state, loglik = raw_decode(eng, obs, pv, lens, L, H, tables)
    assert rc == 0, err_of(eng)
    differing = total = 0
    for b, nf in enumerate(nfs):
        want, best = ref[b]
        got = state[b, :nf]
        assert np.all(state[b, nf:] == -1), "-1 past the row's frames"
        assert np.all((got >= 0) & (got < 2 * nb)), "states of the row"
        score = Y.path_score(got, obs[b, :nf], pv[b, :nf], tables)
        e_l, e_s = abs(loglik[b] - best) / abs(best), abs(score - best) / abs(best)
        v_dev, v_ref = got < nb, want < nb
        diff = (v_dev != v_ref) | (v_ref & (got != want))
        print(f"\nPYIN decode {name} row {b}: frames {nf} voiced {int(v_ref.sum())} loglik {best:.6f} rel err {e_l:.3e} path score rel err {e_s:.3e} "
              f"differing frames {int(diff.sum())}")
        assert e_l <= 1e-9, "d_loglik"
        assert e_s <= 1e-9, "the device's path under the reference model"
        if diff.any():
            assert e_s <= 1e-12, "frames may differ only between paths of equal score"
        differing += int(diff.sum())
        total += nf
    assert differing <= 0.01 * total
    if name == "74-states-R-beyond-the-bins":
        assert nfs[1] == 1 and tables["R"] >= nb
    if name in ("std", "small"):
        assert sum(int((r[0] < nb).sum()) for r in ref) >= 0.5 * total, "the case has voiced stretches"


# ---- 3. audio.pitch_pyin end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f0", [110.0, 220.0])
def test_audio_pitch_pyin_recovers_the_tones(f0):
    y = torch.from_numpy(P.harmonic_tone(f0, 8192)).to(DEV)
    out = audio.pitch_pyin(y)
    f, v, pr = out["f0"].cpu().numpy(), out["voiced"].cpu().numpy(), out["voiced_prob"].cpu().numpy()
    assert f.shape == v.shape == pr.shape == (1, 32) and out["f0"].dtype == torch.float32 and out["voiced"].dtype == torch.bool
    assert out["voiced_prob"].dtype == torch.float32
    it = P.interior_frames(32, 8192)
    assert v[0][it].all() and np.all(f[~v] == 0)
    bins = 120 * np.log2(f[0][it] / f0)
    print(f"\nPYIN audio.pitch_pyin {f0} Hz: voiced {int(v.sum())}/32, interior frames off by {float(np.abs(bins).max()):.3f} bins at most")
    assert np.all(np.abs(bins) <= 1.0), "within one bin of the tone"
    assert np.all(pr[0][it] > 0.5)


def test_audio_pitch_pyin_on_silence():
    out = audio.pitch_pyin(torch.zeros(2, 4096, device=DEV), lengths=[4096, 1000])
    assert out["voiced"].shape == (2, 16) and not out["voiced"].any() and not out["f0"].any() and not out["voiced_prob"].any()


def test_audio_pitch_pyin_in_slices_equals_one_pass(monkeypatch):
    x, lens, _, _ = observed("std")
    xd = torch.from_numpy(x).to(DEV)
    whole = audio.pitch_pyin(xd, lengths=lens)
    monkeypatch.setattr(audio, "PYIN_SLICE_BYTES", 32 * 385 * 10)        # one row at a time
    sliced = audio.pitch_pyin(xd, lengths=lens)
    for k in whole:
        assert torch.equal(whole[k], sliced[k]), k
    ref = cached("pitch_pyin-std", lambda: Y.pitch_pyin(x, lengths=lens))
    v = whole["voiced"].cpu().numpy()
    assert (v != ref["voiced"]).sum() <= 1 and v.sum() >= 40, "the whole chain against the restatement's"


# ---- 4. conventions ----------------------------------------------------------------------------------------------------------------------------
def test_row_alone_in_a_batch_and_as_a_prefix_give_the_same_bits(eng):
    x, lens, kw, ref = observed("std")
    n = lens[2]
    row = x[2, :n]
    nf = -(-n // 256)
    tables = Y.tables_for(kw)
    rc, o_alone, p_alone = raw_observe(eng, row[None], None, **kw)
    assert rc == 0
    rc, o_again, p_again = raw_observe(eng, row[None], None, **kw)
    assert rc == 0 and np.array_equal(o_alone, o_again) and np.array_equal(p_alone, p_again), "two calls"
    rc, o_batch, p_batch = raw_observe(eng, x, lens, **kw)
    assert rc == 0
    longer = np.full((2, n + 777), GARBAGE, np.float32)
    longer[1, :n] = row
    longer[0] = P.chirp(100.0, 300.0, n + 777)
    rc, o_pre, p_pre = raw_observe(eng, longer, [n + 777, n], **kw)
    assert rc == 0
    assert o_alone.shape[1] == nf
    assert np.array_equal(o_alone[0], o_batch[2, :nf]) and np.array_equal(p_alone[0], p_batch[2, :nf]), "alone against inside a batch"
    assert np.array_equal(o_alone[0], o_pre[1, :nf]) and np.array_equal(p_alone[0], p_pre[1, :nf]), "alone against the prefix of a padded row"
    assert not o_pre[1, nf:].any() and not p_pre[1, nf:].any()
    # the decoding, on the device's own observation; behind the row's frames obs and pv are garbage
    rc, s_alone, l_alone = raw_decode(eng, o_alone, p_alone, None, n, 256, tables)
    assert rc == 0
    rc, s_again, l_again = raw_decode(eng, o_alone, p_alone, None, n, 256, tables)
    assert rc == 0 and np.array_equal(s_alone, s_again) and np.array_equal(l_alone, l_again), "two calls"
    rc, s_batch, l_batch = raw_decode(eng, o_batch, p_batch, lens, x.shape[1], 256, tables)
    assert rc == 0
    Fl = -(-(n + 777) // 256)
    o_g, p_g = np.full((2, Fl, kw["n_bins"]), 0.001), np.full((2, Fl), 0.385)
    o_g[1], p_g[1] = -3.0, 7.0                                           # (garbage behind the row's frames)
    o_g[1, :nf], p_g[1, :nf] = o_alone[0], p_alone[0]
    rc, s_pre, l_pre = raw_decode(eng, o_g, p_g, [n + 777, n], n + 777, 256, tables)
    assert rc == 0
    assert np.array_equal(s_alone[0], s_batch[2, :nf]) and l_alone[0] == l_batch[2], "alone against inside a batch"
    assert np.array_equal(s_alone[0], s_pre[1, :nf]) and l_alone[0] == l_pre[1] and np.all(s_pre[1, nf:] == -1), "alone against a prefix"


def test_bad_rows_are_zeros_and_minus_one(eng):
    kw = Y.geometry(22050, 65.0, 600.0, 1024, 256, 0.1)
    L = 3000
    good = P.harmonic_tone(200.0, L)
    x = np.stack([np.full(L, GARBAGE, np.float32), good, np.full(L, GARBAGE, np.float32), np.full(L, GARBAGE, np.float32)])
    rc, o1, p1 = raw_observe(eng, good[None], None, **kw)
    assert rc == 0
    rc, o, p = raw_observe(eng, x, [0, L, -3, L + 1], **kw)
    assert rc == 0
    assert not o[[0, 2, 3]].any() and not p[[0, 2, 3]].any(), "bad rows are zeros"
    assert np.array_equal(o[1], o1[0]) and np.array_equal(p[1], p1[0]), "the good row next to them is unchanged"
    tables = Y.tables_for(kw)
    rc, s1, l1 = raw_decode(eng, o1, p1, None, L, 256, tables)
    assert rc == 0
    rc, s, l = raw_decode(eng, np.where(o == 0, 0.25, o), p, [0, L, -3, L + 1], L, 256, tables)
    assert rc == 0
    assert np.all(s[[0, 2, 3]] == -1) and not l[[0, 2, 3]].any(), "bad rows: no path, log-likelihood 0"
    rc, s, l = raw_decode(eng, o, p, [0, L, -3, L + 1], L, 256, tables)
    assert rc == 0 and np.array_equal(s[1], s1[0]) and l[1] == l1[0]
    assert (s1[0] < kw["n_bins"]).sum() >= 8, "the tone is voiced"


OBSERVE_BAD = [
    ("B=", dict(shape=(0, 512))), ("B=", dict(shape=(65536, 64), n_bins=2)),
    ("hop_length", dict(hop_length=0)), ("hop_length", dict(hop_length=100)), ("hop_length", dict(hop_length=4160)),
    ("frame_length", dict(frame_length=0)), ("frame_length", dict(frame_length=1000)), ("frame_length", dict(frame_length=4160)),
    ("tau_min", dict(tau_min=0)), ("tau_min", dict(tau_min=341)), ("tau_max", dict(tau_max=2049)),
    ("n_thr", dict(w=np.zeros(0))), ("n_thr", dict(w=np.full(129, 1 / 129))),
    ("n_bins", dict(n_bins=1)), ("n_bins", dict(n_bins=1025)),
    ("boltzmann", dict(boltzmann=0.0)), ("boltzmann", dict(boltzmann=float("nan"))),
    ("no_trough_prob", dict(no_trough_prob=-0.1)), ("no_trough_prob", dict(no_trough_prob=1.5)),
]


@pytest.mark.parametrize("word,kw", OBSERVE_BAD, ids=[f"{w}-{i}" for i, (w, _) in enumerate(OBSERVE_BAD)])
def test_each_limit_of_observe_fails_with_a_message_naming_it(eng, word, kw):
    kw = dict(kw)
    x = torch.zeros(kw.pop("shape", (2, 2048)), device=DEV)
    args = Y.geometry(22050, 65.0, 600.0, 1024, 256, 0.1)
    args.update(kw)
    with pytest.raises(EvLibraryError, match=word):
        eng.pyin_observe(x, None, **args)


def test_null_outputs_fail(eng):
    kw = Y.geometry(22050, 65.0, 600.0, 1024, 256, 0.1)
    x = torch.zeros(1, 2048, device=DEV)
    w = kw["w"]
    out = torch.zeros(8 * 385, dtype=torch.float64, device=DEV)
    for obs_p, pv_p in ((None, out.data_ptr()), (out.data_ptr(), None)):
        rc = eng.lib.ev_pyin_observe(eng.h, x.data_ptr(), None, 1, 2048, 1024, 256, 36, 340, 22050.0, 65.0, 120, 385, w.ctypes.data, 100, 2.0, 0.01,
                                     obs_p, pv_p, _stream_ptr())
        assert rc != 0 and "output" in err_of(eng)
    t = Y.transition_tables(385, 25)
    back = torch.zeros(8 * 770, dtype=torch.uint8, device=DEV)
    st = torch.zeros(8, dtype=torch.int32, device=DEV)
    for st_p, ll_p in ((None, out.data_ptr()), (st.data_ptr(), None)):
        rc = eng.lib.ev_pyin_decode(eng.h, out.data_ptr(), out.data_ptr(), None, 1, 2048, 256, 385, 25, t["log_tri"].ctypes.data, t["log_Z"].ctypes.data,
                                    t["log_stay"], t["log_switch"], back.data_ptr(), st_p, ll_p, _stream_ptr())
        assert rc != 0 and "output" in err_of(eng)
    rc = eng.lib.ev_pyin_decode(eng.h, out.data_ptr(), out.data_ptr(), None, 1, 2048, 256, 385, 25, t["log_tri"].ctypes.data, t["log_Z"].ctypes.data,
                                t["log_stay"], t["log_switch"], None, st.data_ptr(), out.data_ptr(), _stream_ptr())
    assert rc != 0 and "d_back" in err_of(eng)
    torch.cuda.synchronize()


DECODE_BAD = [
    ("B=", dict(B=0)), ("hop_length", dict(hop_length=100)), ("hop_length", dict(hop_length=4160)),
    ("n_bins", dict(n_bins=1)), ("n_bins", dict(n_bins=1025)), ("R=", dict(R=-1)), ("R=", dict(R=64)),
    ("switch_prob", dict(log_stay=0.0)), ("switch_prob", dict(log_switch=0.0)), ("switch_prob", dict(log_switch=float("-inf"))),
    ("log_Z", dict(bend_Z=True)),
]


@pytest.mark.parametrize("word,kw", DECODE_BAD, ids=[f"{w}-{i}" for i, (w, _) in enumerate(DECODE_BAD)])
def test_each_limit_of_decode_fails_with_a_message_naming_it(eng, word, kw):
    B, nb, R, H = kw.get("B", 1), kw.get("n_bins", 385), kw.get("R", 25), kw.get("hop_length", 256)
    L = 4 * 256
    F = -(-L // H)
    obs = torch.zeros((B, F, nb), dtype=torch.float64, device=DEV)
    pv = torch.zeros((B, F), dtype=torch.float64, device=DEV)
    lt, lz = np.zeros(max(R + 1, 0)), np.full(nb, 1.0)
    if kw.get("bend_Z"):
        lz[200] = 2.0
    with pytest.raises(EvLibraryError, match=word):
        eng.pyin_decode(obs, pv, None, L, H, R, lt, lz, kw.get("log_stay", math.log(0.99)), kw.get("log_switch", math.log(0.01)))


def test_no_allocation_and_both_calls_in_one_graph():
    e = Engine(0)
    x, lens, kw, _ = observed("std")
    tables = Y.tables_for(kw)
    xd = torch.from_numpy(x).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    dec = (x.shape[1], 256, tables["R"], tables["log_tri"], tables["log_Z"], tables["log_stay"], tables["log_switch"])
    n0 = e.alloc_count()
    obs, pv = e.pyin_observe(xd, ld, **kw)
    state, loglik = e.pyin_decode(obs, pv, ld, *dec)
    small_x, small_lens, small_kw, _ = observed("small")
    e.pyin_observe(torch.from_numpy(small_x).to(DEV), small_lens, **small_kw)
    big = Y.geometry(22050, 10.8, 600.0, 4096, 4096, 1.0)                # tau_max 2042: more LDS than the default grant (the attribute, no allocation)
    e.pyin_observe(xd[:2, :4096].contiguous(), None, **big)
    torch.cuda.synchronize()
    assert e.alloc_count() == n0
    s = torch.cuda.Stream(device=DEV)
    back = torch.empty((3, 32, 2 * kw["n_bins"]), dtype=torch.uint8, device=DEV)
    with torch.cuda.stream(s):
        e.pyin_decode(*e.pyin_observe(xd, ld, **kw), ld, *dec, back=back)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            g_obs, g_pv = e.pyin_observe(xd, ld, **kw)
            g_state, g_ll = e.pyin_decode(g_obs, g_pv, ld, *dec, back=back)
        for t in (g_obs, g_pv, g_ll):
            t.fill_(-5)
        g_state.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in ((g_obs, obs), (g_pv, pv), (g_state, state), (g_ll, loglik)):
        assert torch.equal(a, b), "the replay equals the eager call"
    assert e.alloc_count() == n0
    e.close()
