"""ev_text_encoder, the duration rounding of MatchaTTS._durations and ev_align on the MI355X against the fp64 restatement
(tests/text_encoder_ref.py), at gates set from the float32 reference's own measured error.

What is compared: ``mu_x`` and ``logw`` of ev_text_encoder on every valid token of every row, against ``encode`` of text_encoder_ref in
fp64 (RoPE angle table in fp32, as the reference and the engine define it), run through torch on the GPU and cached; outside the
lengths both outputs are exactly 0.  The error of a call is (RMS, max) over its valid tokens, absolute, held to text_encoder_ref.GATE
of the checkpoint: 3x the float32 CPU oracle's worst error against the same yardstick (tests/test_text_encoder_reference.py).

Cases (text_encoder_ref.cases; "std" the standard synthetic weights, "peak" conv_q / conv_k x 3: peaked softmaxes):
  bench     bench.time_text_encoder's ids and speakers (seed 77, 64 x 151) with full and with ragged lengths (1, 63, 64, 65, 128, 150,
            151 among them), arithmetic settings 16, 6 and 0, both checkpoints; which builds ran is read from the profiled launches.
  edges     Tx in {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 257, 513} at B = 1 and as a ragged B = 3 (Tx, 1, Tx // 2): every side
            of the attention's 64-key tiles and of its 4 queries per workgroup.  2 x 1200 (1200, 333).  A zero-length row between
            full rows.  A single-speaker checkpoint (C = 192).
  durations ceil(exp(logw)) per token against fp64, and mel_lengths through MatchaTTS._durations at length scales 1.0, 0.8 and 1.37:
            no flip outside the exclusion band, exact mel_lengths for utterances without an excluded token (standard checkpoint).
  alignment ev_align on the engine's own w_ceil and mu_x: attn == the restated generate_path, mu_y bit-equal to the gather.
  state     large, small, large on one handle; reserve() then no allocation; a text beyond the attention's LDS limit is refused.
  mutant    one fp16 rounding of the speaker rows exceeds the gate on the bench batch.

Measured on an MI355X (TEERR / TEPATH / TEWORST lines print with -s): see NOTES.md, "Text encoder against fp64".
"""
import os
import time

import pytest
import torch

import text_encoder_ref as R
from emojivoice_amd._lib import EvLibraryError
from emojivoice_amd.matcha_tts import MatchaTTS, fix_len_compatibility

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SETTINGS = (16, 6, 0)
N_CONV = 4 + 4 * R.N_LAYERS + 1 + 3        # conv launches of one call: prenet 3 + proj, (qkv, out, ffn 1, ffn 2) a layer, proj_m, duration predictor 3
_WORST = {}
_CASES = {c[0]: c for c in R.cases()}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    print(f"\nTECLOCK wall {time.perf_counter() - t0:.1f} s")
    for k, v in sorted(_WORST.items(), key=str):
        print(f"TEWORST {k}: mu rms {v[0]:.2e} max {v[1]:.2e}  logw rms {v[2]:.2e} max {v[3]:.2e}")


@pytest.fixture(scope="module")
def sds():
    return R.states()


@pytest.fixture(scope="module")
def models(sds):
    return {w: MatchaTTS(sd, device=DEV) for w, sd in sds.items()}


@pytest.fixture(scope="module")
def refs(sds):
    """ref(w, name) -> (mu, logw) in fp64 on the CPU for a case of the list, computed once through torch on the GPU."""
    e64 = {w: R.encoder_state(sd, torch.float64, DEV) for w, sd in sds.items()}
    cache = {}

    def ref(w, name):
        if (w, name) not in cache:
            _, ids, L, sid = _CASES[name]
            mu, lw = R.encode(sds[w], ids, L, R.speaker_rows(sds[w], sid), device=DEV, esd=e64[w])
            cache[(w, name)] = (mu.cpu(), lw.cpu())
        return cache[(w, name)]
    return ref


def _spk(model, sid):
    return model._sd["spk_emb.weight"][sid.to(DEV)].float().contiguous()


def _run(model, ids, L, spk, setting=16, profile=None):
    """(mu, logw) of one ev_text_encoder call under one arithmetic setting; with ``profile`` (a file path) also
    (profiled launches, launches on the bf16 / fp16 pipes, {build code: launches})."""
    eng = model.engine
    eng.set_arithmetic(setting)
    info = None
    try:
        if profile:
            eng.profile_enable(True)
        mu, lw = eng.text_encoder(ids.to(DEV), L.to(DEV), spk)
        eng.text_encoder_status()
        torch.cuda.synchronize()
        if profile:
            split = eng.profile_read_split()[2]
            if os.path.exists(profile):
                os.remove(profile)
            os.environ["EV_PROFILE_DUMP"] = str(profile)
            try:
                n = eng.profile_read()[2]
            finally:
                del os.environ["EV_PROFILE_DUMP"]
            cfgs = {}
            for line in open(profile):
                f = line.split()
                if f and f[0] == "conv":
                    cfgs[int(f[5])] = cfgs.get(int(f[5]), 0) + int(f[7])
            info = (n, split, cfgs)
    finally:
        if profile:
            eng.profile_enable(False)
        eng.set_arithmetic(16)
    return mu, lw, info


def _check(tag, w, mu, lw, ref, L, bad, rows=None, record=True, key=None):
    """Errors of one call over its valid tokens against the gate of checkpoint ``w``; exact zeros outside the lengths; finite."""
    rmu, rlw = ref if rows is None else (ref[0][rows], ref[1][rows])
    em, el = R.errors(mu, rmu, L), R.errors(lw, rlw, L)
    g = R.GATE[w]
    if not (em[0] <= g["mu"][0] and em[1] <= g["mu"][1] and el[0] <= g["logw"][0] and el[1] <= g["logw"][1]):
        bad.append((tag, w, "gate", em, el))
    if not (bool(torch.isfinite(mu).all()) and bool(torch.isfinite(lw).all())):
        bad.append((tag, w, "non-finite"))
    pad = (torch.arange(mu.shape[-1])[None, :] >= L.cpu()[:, None]).unsqueeze(1)
    if bool((mu.cpu() * pad).ne(0).any()) or bool((lw.cpu() * pad).ne(0).any()):
        bad.append((tag, w, "not 0 outside the lengths"))
    if record:
        key = key or (w, tag.rsplit(" s", 1)[-1] if " s" in tag else "")
        o = _WORST.get(key, (0, 0, 0, 0))
        _WORST[key] = (max(o[0], em[0]), max(o[1], em[1]), max(o[2], el[0]), max(o[3], el[1]))
    print(f"TEERR {tag:<34s} {w:<4s} mu rms {em[0]:.2e} max {em[1]:.2e} ({em[1] / g['mu'][1]:.2f} gate)  "
          f"logw rms {el[0]:.2e} max {el[1]:.2e} ({el[1] / g['logw'][1]:.2f} gate)")
    return em, el


# ---------------------------------------------------------------------------------------------------------------------
# the bench batch: 64 x 151, seed 77
# ---------------------------------------------------------------------------------------------------------------------
def test_bench_batch_every_row(models, refs, tmp_path):
    bad, paths = [], {}
    for w in ("std", "peak"):
        m = models[w]
        for name in ("bench full", "bench ragged"):
            _, ids, L, sid = _CASES[name]
            for s in SETTINGS:
                mu, lw, info = _run(m, ids, L, _spk(m, sid), s, profile=tmp_path / "prof.txt")
                _check(f"{name} s{s}", w, mu, lw, refs(w, name), L, bad, key=(w, f"bench s{s}"))
                paths[(w, name, s)] = info
    _, ids, L, sid = _CASES["bench full"]
    m = models["std"]
    for s in SETTINGS:      # the 4 x 37 call of tests/test_gpu_configs.py's size: what a small call takes
        paths[("small", s)] = _run(m, ids[:4, :37], torch.full((4,), 37), _spk(m, sid[:4]), s, profile=tmp_path / "prof.txt")[2]
    for k, v in paths.items():
        print(f"TEPATH {k}: conv launches {v[0]}, on the bf16 / fp16 pipes {v[1]}, per build code {dict(sorted(v[2].items()))}")
    assert not bad, bad
    for k, (n, split, cfgs) in paths.items():
        assert n == N_CONV and sum(cfgs.values()) == N_CONV, (k, n, cfgs)
        if k[-1] == 0:
            assert split == 0 and not set(cfgs) & {40, 41, 43, 46, 47, 49, 60, 66}, (k, split, cfgs)     # setting 0: every product on the fp32 MFMA
    for w in ("std", "peak"):
        for name in ("bench full", "bench ragged"):
            # the bench shape takes the balanced persistent builds of the split pipes, which the 4 x 37 call never reaches:
            # fp16 pieces (code 66) under setting 16, bf16 pieces (code 60) under setting 6
            assert paths[(w, name, 16)][2].get(66, 0) > 0 and paths[(w, name, 16)][1] == paths[(w, name, 16)][2][66], paths[(w, name, 16)]
            assert paths[(w, name, 6)][2].get(60, 0) > 0 and paths[(w, name, 6)][1] == paths[(w, name, 6)][2][60], paths[(w, name, 6)]
            assert paths[(w, name, 16)][2][66] == paths[(w, name, 6)][2][60]
    for s in SETTINGS:
        assert paths[("small", s)][1] == 0 and paths[("small", s)][2] == paths[("small", 0)][2], paths[("small", s)]
        assert set(paths[("std", "bench full", s)][2]) - set(paths[("small", s)][2]), s          # builds the small call does not take


def test_gate_sees_one_fp16_rounding_of_the_speaker_rows(models, refs):
    """The gate is not vacuous: the speaker rows rounded once to fp16 (a 2^-11 relative error of 64 of the 256 input channels of
    every layer) must fail it on the bench batch."""
    _, ids, L, sid = _CASES["bench full"]
    m, bad = models["std"], []
    mu, lw, _ = _run(m, ids, L, _spk(m, sid).half().float())
    em, el = _check("bench full s16 speaker rows in fp16", "std", mu, lw, refs("std", "bench full"), L, bad, record=False)
    assert any(b[2] == "gate" for b in bad), (em, el)


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tx", R.EDGE_TX)
def test_edge_lengths(models, refs, Tx):
    name = f"edge {Tx}"
    _, ids, L, sid = _CASES[name]
    bad = []
    for w, settings in (("std", SETTINGS), ("peak", (16, 0))):
        m = models[w]
        spk = _spk(m, sid)
        for s in settings:
            mu, lw, _ = _run(m, ids, L, spk, s)
            _check(f"{name} B=3 s{s}", w, mu, lw, refs(w, name), L, bad)
            mu, lw, _ = _run(m, ids[:1], L[:1], spk[:1], s)
            _check(f"{name} B=1 s{s}", w, mu, lw, refs(w, name), L[:1], bad, rows=slice(0, 1))
    assert not bad, bad


def test_long_call(models, refs):
    _, ids, L, sid = _CASES["long 2x1200"]
    bad = []
    for w, settings in (("std", SETTINGS), ("peak", (16, 0))):
        for s in settings:
            mu, lw, _ = _run(models[w], ids, L, _spk(models[w], sid), s)
            _check(f"long 2x1200 s{s}", w, mu, lw, refs(w, "long 2x1200"), L, bad)
    assert not bad, bad


def test_zero_length_row_between_full_rows(models, refs):
    """The reference (the oracle, and text_encoder_ref: pinned on the CPU) returns zeros for a row of length 0 and leaves its
    neighbours alone; so does the engine, and MatchaTTS._durations gives the row the one frame of clamp_min(., 1)."""
    _, ids, L, sid = _CASES["zero-length row"]
    bad = []
    for w in ("std", "peak"):
        m = models[w]
        for s in SETTINGS:
            mu, lw, _ = _run(m, ids, L, _spk(m, sid), s)
            _check(f"zero-length row s{s}", w, mu, lw, refs(w, "zero-length row"), L, bad)
            assert not bool(mu[1].any()) and not bool(lw[1].any())
            two, two_lw, _ = _run(m, ids[[0, 2]], L[[0, 2]], _spk(m, sid[[0, 2]]), s)
            _check(f"zero-length row's neighbours s{s}", w, two, two_lw, refs(w, "zero-length row"), L[[0, 2]], bad, rows=[0, 2])
    y = models["std"]._durations(ids, L, sid, 1.0)[5]
    assert int(y[1]) == 1
    assert not bad, bad


def test_single_speaker_checkpoint(sds):
    sd, ids, L = R.single_speaker_case()
    m = MatchaTTS(sd, device=DEV)
    assert m.n_spks == 1
    ref = tuple(t.cpu() for t in R.encode(sd, ids, L, None, device=DEV))
    bad = []
    for s in SETTINGS:
        mu, lw, _ = _run(m, ids, L, None, s)
        _check(f"single speaker 4x100 s{s}", "std", mu, lw, ref, L, bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# durations
# ---------------------------------------------------------------------------------------------------------------------
DURATION_CASES = ["bench full", "bench ragged"] + [f"edge {t}" for t in R.EDGE_TX]


def test_durations_against_fp64(models, refs):
    """Standard checkpoint, the bench batch and the edge shapes.  Per token: ceil(exp(logw)) of the engine's logw equals the fp64
    one outside the exclusion band.  Per utterance without an excluded token: mel_lengths of MatchaTTS._durations at length scales
    1.0, 0.8 and 1.37 equal the reference's rounding of the fp64 durations."""
    m = models["std"]
    tokens = excluded = flips = flips_in_band = utts = utts_checked = 0
    bad = []
    for name in DURATION_CASES:
        _, ids, L, sid = _CASES[name]
        frames64 = R.token_frames(refs("std", name)[1], L)
        near = R.near_integer(refs("std", name)[1], L, R.GATE["std"]["logw"][1])
        clean = ~near.any(1)
        for ls in R.LENGTH_SCALES:
            _, _, w_ceil, _, _, y, y_max = m._durations(ids, L, sid, ls)
            if ls == 1.0:
                got = w_ceil.cpu().reshape(frames64.shape).double()
                diff = got != frames64
                tokens += int(L.sum()); excluded += int(near.sum())
                flips += int((diff & ~near).sum()); flips_in_band += int((diff & near).sum())
                if bool((diff & ~near).any()):
                    bad.append((name, "duration flips outside the band", torch.nonzero(diff & ~near).tolist()[:4]))
            want_w, want_y = R.mel_lengths(frames64, ls)
            utts += len(L); utts_checked += int(clean.sum())
            if not torch.equal(y.cpu()[clean], want_y[clean]):
                bad.append((name, ls, "mel_lengths", y.cpu()[clean].tolist(), want_y[clean].tolist()))
            if y_max != int(y.max()):
                bad.append((name, ls, "y_max"))
    print(f"TEDUR tokens {tokens}  in the exclusion band {excluded}  flips outside it {flips}  inside it {flips_in_band}  "
          f"mel_lengths checked on {utts_checked} of {utts} utterance x scale pairs")
    assert not bad, bad
    assert excluded <= R.CAP_TOKENS * tokens and utts_checked >= (1 - R.CAP_UTTERANCES) * utts


# ---------------------------------------------------------------------------------------------------------------------
# alignment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows,ls", [("bench ragged", None, 1.37), ("bench full", None, 1.37), ("bench ragged", None, 1.0), ("bench full", None, 0.8),
                                          ("edge 1", slice(0, 1), 1.0), ("edge 1", slice(0, 1), 1.37), ("edge 513", None, 1.0), ("edge 513", None, 1.37)])
def test_align_on_the_engines_own_durations(models, name, rows, ls):
    m = models["std"]
    _, ids, L, sid = _CASES[name]
    if rows is not None:
        ids, L, sid = ids[rows], L[rows], sid[rows]
    _, mu_x, w_ceil, _, _, y, y_max = m._durations(ids, L, sid, ls)
    Tp = fix_len_compatibility(y_max)
    want_attn = R.path(w_ceil.cpu()[:, 0], L, y.cpu(), Tp)
    want_mu = R.expand(want_attn, mu_x)
    mu_y, attn = m.engine.align(w_ceil, mu_x, L.to(DEV), y, Tp, want_attn=True)
    mu_y2, none = m.engine.align(w_ceil, mu_x, L.to(DEV), y, Tp, want_attn=False)
    torch.cuda.synchronize()
    print(f"TEALIGN {name} x{ls}: B {len(L)} Tx {ids.shape[1]} Tp {Tp} mel_lengths {int(y.min())}..{int(y.max())}")
    assert none is None and attn.shape == (len(L), 1, ids.shape[1], Tp)
    assert torch.equal(attn.cpu()[:, 0], want_attn)
    assert torch.equal(mu_y.cpu(), want_mu) and torch.equal(mu_y2.cpu(), want_mu)
    for r, n in enumerate(y.tolist()):
        assert not bool(mu_y[r, :, n:].any()) and not bool(attn[r, :, :, n:].any())
        assert torch.equal(attn[r, 0, :int(L[r])].sum(0)[:n].cpu(), torch.ones(n) if int(L[r]) else torch.zeros(n))


# ---------------------------------------------------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------------------------------------------------
def test_large_small_large_on_one_handle(models):
    m = models["std"]
    _, ids, L, sid = _CASES["bench ragged"]
    _, ids_s, L_s, sid_s = _CASES["edge 5"]
    a = _run(m, ids, L, _spk(m, sid))
    s1 = _run(m, ids_s, L_s, _spk(m, sid_s))
    b = _run(m, ids, L, _spk(m, sid))
    s2 = _run(m, ids_s, L_s, _spk(m, sid_s))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])


def test_reserve_then_the_bench_call_allocates_nothing(sds):
    m = MatchaTTS(sds["std"], device=DEV)
    m.engine.reserve(R.B_BENCH, R.TX_BENCH, 0, 0)
    n0 = m.engine.alloc_count()
    _, ids, L, sid = _CASES["bench full"]
    for s in SETTINGS:
        _run(m, ids, L, _spk(m, sid), s)
    assert m.engine.alloc_count() == n0, (n0, m.engine.alloc_count())


def _lds_token_limit(kc):
    """The longest text run_text_encoder accepts: enc_attention_kernel's dynamic LDS, (64 * (kc | 4) + 4 * kc + 4 * ceil64(Tx)) floats,
    may not exceed 160 KiB."""
    return (160 * 1024 // 4 - 64 * (kc | 4) - 4 * kc) // 4 // 64 * 64


def test_text_beyond_the_lds_limit_is_refused(models, refs):
    """An argument check that returns before the attention launch; the handle serves the next call."""
    m = models["std"]
    limit = _lds_token_limit(256 // R.N_HEADS)
    assert limit == 8000
    ids, sid = R.random_inputs(1, limit + 1, 8001)
    with pytest.raises(EvLibraryError, match="text too long"):
        m.engine.text_encoder(ids.to(DEV), torch.tensor([limit + 1]), _spk(m, sid))
    bad = []
    _, ids_s, L_s, sid_s = _CASES["edge 65"]
    mu, lw, _ = _run(m, ids_s, L_s, _spk(m, sid_s))
    _check("edge 65 after a refused call", "std", mu, lw, refs("std", "edge 65"), L_s, bad, record=False)
    # the longest text that fits (all 160 KiB of a CU's LDS) is served, and is right
    L = torch.tensor([limit])
    ref = tuple(t.cpu() for t in R.encode(m._cpu_sd, ids[:, :limit], L, R.speaker_rows(m._cpu_sd, sid), device=DEV))
    mu, lw, _ = _run(m, ids[:, :limit], L, _spk(m, sid))
    _check(f"1 x {limit} s16", "std", mu, lw, ref, L, bad, record=False)
    assert not bad, bad
