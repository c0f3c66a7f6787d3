"""Every build of the U-Net's self-attention on a real MI355X, per query row against the fp64 restatement of tests/attention_ref.py.

What each test reaches (launch_attn / launch_attn_out in ev_engine.hip; the build is ASSERTED from what the op reports, never assumed):
  test_unfused_builds     ev_op_attention2 -> launch_attn, heads = 2, B = 3 ragged unless stated
                            attention_kernel                                   T = 1, 31, 32, 33, 96 (scratch given: < 4 key tiles never split),
                                                                               127, 128, 129, 260 (scratch withheld), and every split shape below
                            attention_part_kernel + attention_merge_kernel     T = 97, 128 (KS 2), 129 (KS 3: parts of 2, 2, 1 tiles), 516 (KS 9: part 7 =
                                                                               tiles 7, 16), 1030 (KS capped at 16), 1 x 4096 (64 workgroups, 8 tiles per part)
                            EV_ATTN_TPW = 1 and 3 on fresh handles             T = 516: KS 16 (part 0 = tiles 0, 16) and KS 6
                            the 64-workgroup edge                              6 x 516 splits (60 workgroups), 7 x 516 (70) does not
  test_fused_builds       ev_op_attn_out2 -> launch_attn_out under arithmetic 16 (attn_out_h16_kernel + attn_tail_path<true>), arithmetic 16 with the
                          fp16 attention off and arithmetic 0 (attn_out_kernel + attn_tail_path<false>): T = 32, 64, 65, 96 (key halves of 1 + 0, 1 + 1,
                          2 + 1 tiles), 33 .. 36 (ntail 1 .. 4), 37 (ragged full-size tile), 258, 516, 4 (one tile, no tail path), B = 8, 16 (xcd_map)
                          against 5, 9 at T = 36
  test_fused_all_classes  4 x 132 and 4 x 36, every input class, scales from the data and — fp16 builds — from a bound 2^10 above it (below_bound)
  test_*_bits             padded geometry (P = 2, S = T + 4 and P = 0, S = T + 3; pad rows of q / k / v hold NaN, pad rows of the outputs a sentinel that
                          must survive), bit-equality with the S = T call, isolation from an inf / NaN in another utterance's q, k or v, an utterance
                          alone against the same utterance in a batch, three calls giving the same bits — on every build

Gates: attention_ref's — per query row (ALL B x T rows of a case, the rows beyond the length included), RMS and L-inf, 4 x the worst error of the plain
fp32 evaluation on the same case and class (fp16 builds: plus the representation error of the fp16 form — q, k, v, and for attn_out_h16_kernel Wout and
the attention rows it re-quantises at v's scale), floor 2^-21 of the row's fp64 L-inf; derived
in-process, never from a kernel.  With -s the module prints ATTNERR lines per (build, shape, class) and, at the end, ATTNRATIO lines per (build, class):
the worst kernel error / yardstick (the gate is at 4).

Worst ratio per (build, class) measured on an MI355X — see profiles/attention_fp64_errors.txt for the figures per shape:
  attention_kernel                               randn 1.21  peaked 2.15  flat 1.11  mask_decides 1.32  pad_heavy 1.54  quiet_keys 1.82  quiet_values 1.88  large 1.50  tile_skew 1.18
  attention_part_kernel + attention_merge_kernel randn 1.04  peaked 1.21  flat 0.87  mask_decides 1.31  pad_heavy 1.41  quiet_keys 1.61  quiet_values 1.02  large 1.75  tile_skew 3.74
  attn_out_h16_kernel                            randn 1.15  peaked 1.49  flat 1.02  mask_decides 0.99  pad_heavy 1.01  quiet_keys 1.33  quiet_values 1.46  large 0.94  tile_skew 0.77
  attn_out_kernel (f32_arith0)                   randn 1.56  peaked 3.38  flat 2.14  mask_decides 1.25  pad_heavy 1.87  quiet_keys 2.08  quiet_values 1.69  large 2.36  tile_skew 1.17
  attn_out_kernel (f32_arith16)                  randn 1.56  peaked 3.38  flat 2.14  mask_decides 1.25  pad_heavy 1.87  quiet_keys 2.08  quiet_values 1.69  large 2.36  tile_skew 1.17
  attn_tail_path<false> (f32_arith0)             randn 1.09  peaked 0.72  flat 2.11  mask_decides 0.37  pad_heavy 1.12  quiet_keys 1.14  quiet_values 1.18  large 0.39  tile_skew 0.98
  attn_tail_path<false> (f32_arith16)            randn 1.09  peaked 0.72  flat 2.11  mask_decides 0.37  pad_heavy 1.12  quiet_keys 1.14  quiet_values 1.18  large 0.39  tile_skew 0.98
  attn_tail_path<true>                           randn 1.14  peaked 0.29  flat 1.90  mask_decides 0.42  pad_heavy 0.96  quiet_keys 1.01  quiet_values 1.11  large 0.29  tile_skew 0.92
Maximum 3.74 (split-key, 3 x 1030, KS = 16, the tile_skew rows): the dominant key sits in tile 32, which belongs to part 0, so the merge — ascending
part order — starts from l = 1.0 and adds fifteen terms of about one ulp of it, each of which loses up to half an ulp (9e-7 in l in all, where
attention_kernel folds the small terms together before the dominant tile arrives and rounds once).  test_attention_reference.py writes both
orders in fp32 torch on the CPU and shows the same (test_split_key_merge_order_in_fp32_stays_inside_the_gate prints its figures with -s);
1 x 4096, whose dominant tile belongs to the LAST part, stands at 1.02.  Fifteen half-ulps is the most this order can
lose, and it is inside the gate: arithmetic, not a defect, and the kernel is left as it is.  attn_out_kernel is bit-identical under arithmetic 16 and 0.
Before the attention rows' re-quantisation at v's scale was part of the fp16 yardstick, attn_out_h16_kernel stood at 4.74 on the quiet_keys rows of
4 x 132 under below_bound scales (attention_ref's docstring); no case exposed a bug, no gate was widened.
"""
import os

import pytest
import torch

import attention_ref as A
from emojivoice_amd._lib import Engine

pytestmark = pytest.mark.gpu

_RATIOS = {}
_REFS = {}
MODES = {"h16": (16, True), "f32_arith16": (16, False), "f32_arith0": (0, True)}


def _note(build, shape, ratios):
    by_cls = {}
    for (cls, kind), r in ratios.items():
        by_cls[cls] = max(by_cls.get(cls, 0.0), r)
        _RATIOS[(build, cls)] = max(_RATIOS.get((build, cls), 0.0), r)
    print(f"ATTNERR {build} {shape}: " + "  ".join(f"{c} {r:.2f}" for c, r in by_cls.items()))


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, spk_emb_dim=64)
    arith = e.arithmetic()
    yield e
    e.set_arithmetic(arith)
    e.set_attn_h16(True)
    e.close()
    for build in sorted({k[0] for k in _RATIOS}):
        print(f"\nATTNRATIO {build}: " + "  ".join(f"{c} {_RATIOS[(build, c)]:.2f}" for c in A.CLASSES if (build, c) in _RATIOS))
    if _RATIOS:
        print(f"ATTNRATIO max {max(_RATIOS.values()):.2f}")


def _refs(c, key, fused, scales=None):
    """fp64 reference and yardsticks of a case: computed once, shared by every test that runs the case, never modified."""
    k = (key, fused, scales)
    if k not in _REFS:
        _REFS[k] = A.references(c, fused, scales)
    return _REFS[k]


def _lay(x, S, P, fill):
    """(B, T, W) -> (B*S, W) on the GPU: utterance b's frame t in row b*S + P + t, every other row = fill"""
    B, T, W = x.shape
    buf = torch.full((B, S, W), fill, dtype=torch.float32)
    buf[:, P:P + T] = x
    return buf.reshape(B * S, W).cuda()


def _valid(buf, B, S, P, T):
    return buf.reshape(B, S, -1)[:, P:P + T].reshape(B * T, -1)


SENTINEL = -12345.678


def _pads_intact(buf, B, S, P, T):
    full = buf.reshape(B, S, -1)
    return bool((full[:, :P] == SENTINEL).all()) and bool((full[:, P + T:] == SENTINEL).all())


def _unfused(e, c, scratch, S=None, P=0, qkv=None):
    """-> ((B*T, 128) rows on the CPU, what ran).  Padded geometry: NaN in the pad rows of qkv, a sentinel in those of the output."""
    B, T = c["B"], c["T"]
    S = T if S is None else S
    out = torch.full((B * S, 128), SENTINEL, dtype=torch.float32).cuda()
    out, ran = e.op_attention2(_lay(c["qkv"] if qkv is None else qkv, S, P, float("nan")), c["lengths"].cuda(), S, P, T, 2, scratch, out)
    out = out.cpu()
    assert _pads_intact(out, B, S, P, T), "pad rows of the output were written"
    return _valid(out, B, S, P, T), ran


def _fused(e, c, scales=None, S=None, P=0, qkv=None):
    B, T = c["B"], c["T"]
    S = T if S is None else S
    hid = _lay(c["hid"], S, P, SENTINEL)
    hid, ran = e.op_attn_out2(_lay(c["qkv"] if qkv is None else qkv, S, P, float("nan")), c["lengths"].cuda(), c["w_out"], c["b_out"], hid, S, P, T, scales)
    hid = hid.cpu()
    assert _pads_intact(hid, B, S, P, T), "pad rows of the hidden tensor were written"
    return _valid(hid, B, S, P, T), ran


# ---------------------------------------------------------------------------------------------------------------------
# the un-fused op: attention_kernel and the split-key pair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,tpw,scratch,want", A.UNFUSED, ids=[f"{B}x{T}-tpw{tpw}-{'scratch' if sc else 'noscratch'}" for B, T, tpw, sc, _ in A.UNFUSED])
def test_unfused_builds(eng, B, T, tpw, scratch, want):
    c = A.unfused_case(B, T)
    refs = _refs(c, ("u", B, T), False)
    e = eng
    if tpw != 2:                                    # tiles per part are read when a handle is created
        os.environ["EV_ATTN_TPW"] = str(tpw)
        try:
            e = Engine(0, spk_emb_dim=64)
        finally:
            del os.environ["EV_ATTN_TPW"]
    try:
        got, ran = _unfused(e, c, scratch)
    finally:
        if e is not eng:
            e.close()
    assert (ran["split"], ran["KS"]) == want == A.plan_attn(B, T, tpw=tpw, scratch=scratch), (ran, want)
    build = f"attention_part+merge KS={ran['KS']}" if ran["split"] else "attention_kernel"
    bad, ratios = A.failures(got, c, refs, tag=f"{build} {B}x{T}")
    _note("attention_part_kernel + attention_merge_kernel" if ran["split"] else "attention_kernel", f"{B}x{T} tpw {tpw} KS {ran['KS']}", ratios)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the fused op: attn_out_kernel / attn_out_h16_kernel and the two attn_tail_path instantiations
# ---------------------------------------------------------------------------------------------------------------------
def _set_mode(e, mode):
    arith, h16 = MODES[mode]
    e.set_arithmetic(arith)
    e.set_attn_h16(h16)


def _check_fused(e, mode, c, key, want, scales, what):
    B, T = c["B"], c["T"]
    fp16 = mode == "h16"
    used = (A.data_scales(c["qkv"]) if scales is None else scales) if fp16 else None
    refs = _refs(c, key, True, used)
    _set_mode(e, mode)
    got, ran = _fused(e, c, scales if fp16 else None)
    nq, ntail = want
    assert (ran["h16"], ran["nq"], ran["ntail"]) == (fp16, nq, ntail) and want == A.plan_attn_out(T), (mode, ran, want)
    tail = (torch.arange(B * T) % T) >= 32 * nq if ntail else torch.zeros(B * T, dtype=torch.bool)
    main_name = "attn_out_h16_kernel" if fp16 else f"attn_out_kernel ({mode})"
    tail_name = "attn_tail_path<true>" if fp16 else f"attn_tail_path<false> ({mode})"
    bad, ratios = A.failures(got, c, refs, fp16=fp16, tag=f"{main_name} {what}", keep=~tail)
    _note(main_name, what, ratios)
    if ntail:
        assert int(tail.sum()) == B * ntail
        bad_t, ratios = A.failures(got, c, refs, fp16="tail" if fp16 else False, tag=f"{tail_name} {what}", keep=tail)
        _note(tail_name, what, ratios)
        bad += bad_t
    assert not bad, bad


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B,T,want", A.FUSED, ids=[f"{B}x{T}" for B, T, _ in A.FUSED])
def test_fused_builds(eng, mode, B, T, want):
    c = A.case(B, T, A.fused_first(B, T))
    _check_fused(eng, mode, c, ("f", B, T), want, None, f"{B}x{T}")


@pytest.mark.parametrize("mode,scaling", [(m, "data") for m in MODES] + [("h16", "below_bound")])
@pytest.mark.parametrize("B,T,first,want", A.FUSED_ALL, ids=[f"{B}x{T}-from-{A.CLASSES[f]}" for B, T, f, _ in A.FUSED_ALL])
def test_fused_all_classes(eng, mode, scaling, B, T, first, want):
    c = A.case(B, T, first)
    scales = A.bound_scales(c["qkv"]) if scaling == "below_bound" else None
    _check_fused(eng, mode, c, ("fa", B, T, first), want, scales, f"{B}x{T} {scaling} scales")


# ---------------------------------------------------------------------------------------------------------------------
# bits: padded geometry, isolation, alone against in a batch, determinism — on every build
# ---------------------------------------------------------------------------------------------------------------------
def _poisoned(c, which):
    """The case's qkv with an inf / NaN / -inf in utterance 1's q, k or v (frames inside and beyond its length)"""
    x = c["qkv"].clone()
    T, L = c["T"], int(c["lengths"][1])
    col = {"q": 0, "k": 128, "v": 256}[which]
    x[1, 0, col + 5] = float("inf")
    x[1, min(T - 1, L), col + 70] = float("nan")
    x[1, T - 1, col + 127] = float("-inf")
    return x


def _bits(run, run_alone, c, what):
    """run(c, S, P, qkv) -> (rows, ran); run_alone(c1) likewise for a one-utterance case."""
    B, T = c["B"], c["T"]
    base, ran = run(c, None, 0, None)
    assert bool(torch.isfinite(base).all()), what
    for _ in range(2):
        again, ran2 = run(c, None, 0, None)
        assert ran2 == ran and torch.equal(again, base), f"{what}: a repeated call gives other bits"
    for S, P in ((T + 4, 2), (T + 3, 0)):
        got, ran2 = run(c, S, P, None)
        assert ran2 == ran, (what, S, P, ran, ran2)
        assert torch.equal(got, base), f"{what}: S = {S}, P = {P} differs from the S = T call"
    keep = (torch.arange(B * T) // T) != 1
    for which in ("q", "k", "v"):
        got, ran2 = run(c, T + 4, 2, _poisoned(c, which))
        assert ran2 == ran
        assert torch.equal(got[keep], base[keep]), f"{what}: a non-finite {which} in utterance 1 reached another utterance"
        assert not bool(torch.isfinite(got[~keep]).all()), f"{what}: the non-finite {which} left no trace in its own utterance"
    for b in (0, B - 1):
        one = {**c, "B": 1, "qkv": c["qkv"][b:b + 1], "hid": c["hid"][b:b + 1], "lengths": c["lengths"][b:b + 1]}
        got, ran1 = run_alone(one)
        if ran1 == ran:
            assert torch.equal(got, base[b * T:(b + 1) * T]), f"{what}: utterance {b} alone and in the batch differ"
        else:
            pytest.fail(f"{what}: alone ran {ran1}, in the batch {ran}")


@pytest.mark.parametrize("scratch,T", [(False, 129), (True, 129), (True, 516)], ids=["attention_kernel", "split-KS3", "split-KS9"])
def test_unfused_bits(eng, scratch, T):
    c = A.case(3, T, classes=("randn", "peaked", "quiet_values"), lengths=(T, T // 2, T - 1), seed=77 + T)
    want = A.plan_attn(3, T, scratch=scratch)
    run = lambda cc, S, P, qkv: _unfused(eng, cc, scratch, S, P, qkv)   # noqa: E731
    _bits(run, lambda one: _unfused(eng, one, scratch), c, f"un-fused, scratch {scratch}, T {T}")
    assert (lambda r: (r["split"], r["KS"]))(run(c, None, 0, None)[1]) == want


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("T", [36, 37, 65])
def test_fused_bits(eng, mode, T):
    """T = 36: one full tile + attn_tail_path with 4 queries; 37: a ragged second tile whose tail rows are the next utterance's; 65: ntail 1."""
    c = A.case(3, T, classes=("randn", "peaked", "quiet_values"), lengths=(T, T // 2, T - 1), seed=99 + T)
    scales = A.data_scales(c["qkv"]) if mode == "h16" else None      # explicit: alone and in the batch must pack alike
    _set_mode(eng, mode)
    run = lambda cc, S, P, qkv: _fused(eng, cc, scales, S, P, qkv)   # noqa: E731
    _bits(run, lambda one: _fused(eng, one, scales), c, f"fused {mode}, T {T}")
    ran = run(c, None, 0, None)[1]
    assert (ran["h16"], ran["nq"], ran["ntail"]) == (mode == "h16",) + A.plan_attn_out(T)


def test_old_entry_points_are_the_new_ones_at_s_equal_t(eng):
    c = A.case(3, 129, 0)
    x, L = c["qkv"].cuda(), c["lengths"].cuda()
    new, ran = _unfused(eng, c, False)
    assert not ran["split"] and torch.equal(eng.op_attention(x, L, 2).cpu().reshape(-1, 128), new)
    for mode in MODES:
        _set_mode(eng, mode)
        new, _ = _fused(eng, c)
        assert torch.equal(eng.op_attn_out(x, L, c["w_out"], c["b_out"], c["hid"].cuda()).cpu().reshape(-1, 256), new), mode


def test_bad_arguments_are_refused(eng):
    c = A.case(2, 40, 0)
    x, L = c["qkv"].reshape(-1, 384).cuda(), c["lengths"].cuda()
    from emojivoice_amd._lib import EvLibraryError
    with pytest.raises(EvLibraryError):
        eng.op_attention2(x, L, 40, 2, 40)                             # S < P + T
    with pytest.raises(EvLibraryError):
        eng.op_attn_out2(x, L, c["w_out"], c["b_out"], c["hid"].reshape(-1, 256).cuda(), 40, 0, 40, scales=(3.0, 1.0, 1.0))
    with pytest.raises(EvLibraryError, match="all zero"):
        eng.op_attn_out2(x, L, c["w_out"], c["b_out"], c["hid"].reshape(-1, 256).cuda(), 40, 0, 40, scales=(4.0, 0.0, 1.0))
    with pytest.raises(EvLibraryError, match="heads = 2"):
        eng.op_attention2(torch.zeros(80, 768).cuda(), L, 40, 0, 40, heads=4)
    with pytest.raises(EvLibraryError, match="ev_op_attention:"):       # the old entry point reports under its own name
        eng.op_attention(torch.zeros(0, 40, 384).cuda(), L[:0], 2)
    got, _ = _unfused(eng, c, True)                                    # the handle serves the next call
    assert bool(torch.isfinite(got).all())
