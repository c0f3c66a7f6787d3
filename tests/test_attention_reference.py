"""tests/attention_ref.py proves itself on the CPU: the fp64 restatement is the reference's attention, the yardsticks are non-trivial, every
row of every case is gated against something, mutants of the five code paths trip the gate, and the shape table of the GPU test maps to
the builds it is meant to reach — before a GPU is involved."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_ref as A
from oracle import matcha_oracle as O

F64, F32 = torch.float64, torch.float32


def test_restatement_is_sdpa_with_the_float_mask_added_and_the_oracle():
    c = A.case(3, 45, first=0)
    x, L = c["qkv"].double(), c["lengths"]
    q, k, v = A.split_heads(x)
    am = A.key_mask(L, 45, F64)[:, None, None, :]
    sdpa = F.scaled_dot_product_attention(q, k, v, attn_mask=am).transpose(1, 2).reshape(3, 45, 128)
    got = A.attention(x, L)
    assert float((got - sdpa).abs().max()) <= 1e-13
    # the oracle's attention on the same tensors: to_q / to_k / to_v pick the three 128-column blocks of x
    eye = torch.eye(384, dtype=F64)
    sd = {"a.to_q.weight": eye[:128], "a.to_k.weight": eye[128:256], "a.to_v.weight": eye[256:],
          "a.to_out.0.weight": c["w_out"].double(), "a.to_out.0.bias": c["b_out"].double()}
    want = O.attention(sd, "a", x, A.key_mask(L, 45, F64)[:, None, :], heads=2)
    fused = A.attn_out(x, L, c["w_out"].double(), c["b_out"].double(), c["hid"].double())
    assert float((fused - c["hid"].double() - want).abs().max()) <= 1e-13
    # rows beyond the length have values of their own, and padded keys matter
    assert float(got[1, int(L[1]):].abs().min()) > 0
    x2 = x.clone()
    x2[1, int(L[1]):, 256:] += 1.0
    assert float((A.attention(x2, L)[1, 0] - got[1, 0]).abs().max()) > 1e-3


def _all_cases():
    seen = {}
    for B, T, _, _, _ in A.UNFUSED:
        seen.setdefault(("u", B, T), (False, B, T, None))
    for B, T, _ in A.FUSED:
        seen.setdefault(("f", B, T), (True, B, T, A.fused_first(B, T)))
    for B, T, first, _ in A.FUSED_ALL:
        seen.setdefault(("fa", B, T, first), (True, B, T, first))
    return list(seen.values())


@pytest.mark.parametrize("fused,B,T,first", _all_cases())
def test_every_row_is_gated_against_something(fused, B, T, first):
    """The plain fp32 evaluation is finite and differs from fp64 on every class (a yardstick of 0 would leave only the floor), and every
    one of the B x T rows — the rows beyond the length too — has an fp64 RMS above RMS_FLOOR."""
    c = A.unfused_case(B, T) if first is None else A.case(B, T, first)
    refs = A.references(c, fused, scales=A.bound_scales(c["qkv"]) if fused else None)
    assert refs["term"].shape[0] == B * T and bool(torch.isfinite(refs["ref"]).all())
    rms = refs["term"].pow(2).mean(dim=1).sqrt()
    assert float(rms.min()) > A.RMS_FLOOR, (float(rms.min()), c["classes"][int(rms.argmin()) // T])
    for k in set(int(i) for i in c["cls"]):
        assert bool(torch.isfinite(refs["yard32"][:, k]).all())
        if T > 1:
            assert float(refs["yard32"][0, k]) > 0, A.CLASSES[k]
            assert float(refs["yard32"][1, k]) < 1e-3, A.CLASSES[k]
        if fused:
            assert float(refs["yard16"][0, k]) > float(refs["yard32"][0, k])
    # the plain fp32 evaluation passes its own gate
    bad, _ = A.failures(A.evaluate(c, fused, F32), c, refs)
    assert not bad, bad


def test_every_class_is_what_it_says():
    T = 129
    c = A.case(len(A.CLASSES), T, first=0)
    assert tuple(c["classes"]) == A.CLASSES
    x, L = c["qkv"].double(), c["lengths"]
    q, k, v = A.split_heads(x)
    s = q @ k.transpose(-1, -2) / 8.0
    p = torch.softmax(s + A.key_mask(L, T, F64)[:, None, None, :], dim=-1)
    i = A.CLASSES.index
    assert float(x[:, T - 1, 128:].abs().min()) > 0                                       # keys and values are non-zero at the padded frames
    assert float(p[i("peaked")].amax(dim=-1).median()) > 0.9 and float(s[i("peaked")].abs().max()) > 60
    lf = int(L[i("flat")])
    assert lf < T and abs(float(p[i("flat"), 0, 0, T - 1] / p[i("flat"), 0, 0, 0]) - math.exp(-1)) < 1e-12
    b = i("mask_decides")
    lm = int(L[b])
    assert lm < T and bool((s[b].argmax(dim=-1) >= lm).all()) and bool((p[b].argmax(dim=-1) < lm).all())
    assert int(L[i("pad_heavy")]) == 1 and float(p[i("pad_heavy"), :, :, 1:].sum(dim=-1).median()) > 0.9
    assert float(x[i("quiet_keys"), ::2, 128:256].abs().max()) < 2.0 ** -9 and float(x[i("quiet_values"), ::2, 256:].abs().max()) < 2.0 ** -9
    assert float(x[i("large"), :, 128:].abs().max()) > 1000 and float(s[i("large")].abs().max()) < 400
    b = i("tile_skew")
    assert bool((p[b].argmax(dim=-1) == T - 1).all()) and float(s[b, :, :, :T - 1].abs().max()) < 3 and float(s[b, :, :, T - 1].min()) > 15


def test_the_fp16_form_model():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4096, generator=g) * torch.logspace(-8, 0, 4096, base=2.0) * 3.0
    for shift in (0, A.BOUND_SHIFT, 20):
        s = A.pow2_scale(float(x.abs().max()), shift=shift)
        assert 16384 / 2.0 ** shift < float(x.abs().max()) * s <= 32768 / 2.0 ** shift
        h0, h1 = A.pack(x, s)
        assert float(h0.abs().max()) <= 32768 and bool((h0.half().float() == h0).all()) and bool((h1.half().float() == h1).all())
        err = (A.unpack(h0, h1, s) - x.double()).abs()
        assert bool((err <= torch.maximum(2.0 ** -22 * x.double().abs(), torch.tensor(2.0 ** -25 / s, dtype=F64))).all())
        if shift == 20:
            assert float(err.max()) > 0                        # far below the bound the floor is what is left
    w = torch.randn(256, 128, generator=g) / 128 ** 0.5
    assert 8192 <= float(w.abs().max()) * A.weight_scale(w) < 16384
    assert float((A.quantised_weight(w) - w.double()).abs().max()) <= 2.0 ** -22 * float(w.abs().max())
    # attn_mask_split: two fp16-representable powers of two whose product is 8 sq sk, for every scale the cases use
    scales = []
    for B, T, first, _ in A.FUSED_ALL:
        c = A.case(B, T, first)
        scales += [A.data_scales(c["qkv"]), A.bound_scales(c["qkv"])]
    for B, T, _ in A.FUSED:
        c = A.case(B, T, A.fused_first(B, T))
        scales.append(A.data_scales(c["qkv"]))
    for sq, sk, sv in scales:
        ma, mb = A.mask_split(sq, sk)
        assert ma * mb == 8 * sq * sk
        for m in (ma, mb):
            assert 2.0 ** -14 <= m <= 2.0 ** 15 and math.frexp(m)[0] == 0.5 and float(torch.tensor(m).half()) == m
    assert A.mask_split(2.0 ** 20, 2.0 ** 20) is None and A.mask_split(3.0, 1.0) is None
    assert A.mask_split(2.0 ** -9, 2.0 ** -9) == (2.0 ** -7, 2.0 ** -8)          # e = -15: truncation toward zero, as in C++


# ---------------------------------------------------------------------------------------------------------------------
# mutants: every one evaluates in fp64, so only the mutation separates it from the reference
# ---------------------------------------------------------------------------------------------------------------------
def _scores(c, scale=0.125, mask="add", qkv=None):
    x = (c["qkv"] if qkv is None else qkv).double()
    q, k, v = A.split_heads(x)
    m = A.key_mask(c["lengths"], c["T"], F64)[:, None, None, :]
    s = q @ k.transpose(-1, -2) * scale
    if mask == "add":
        s = s + m
    elif mask == "mul":
        s = s * m
    elif mask == "bool":
        s = s.masked_fill(m == 0, float("-inf"))
    return s, v


def _heads_out(o, swap=False):
    B, H, T, D = o.shape
    if swap:
        o = o.flip(1)
    return o.transpose(1, 2).reshape(B * T, H * D)


def _finish(c, att, fused, bias=1):
    if not fused:
        return att.float()
    return (c["hid"].double().reshape(-1, 256) + att @ c["w_out"].double().T + bias * c["b_out"].double()).float()


def _grouped(c, groups, weighted=True):
    """Online softmax over groups of 32-key tiles, each group with its own maximum, merged in ascending order: exact when weighted."""
    s, v = _scores(c)
    T = c["T"]
    ms, ls, os_ = [], [], []
    for tiles in groups:
        keys = torch.cat([torch.arange(32 * t, min(T, 32 * t + 32)) for t in tiles]) if tiles else torch.zeros(0, dtype=torch.long)
        if len(keys) == 0:
            continue
        sp = s[..., keys]
        mp = sp.amax(dim=-1, keepdim=True)
        pp = torch.exp(sp - mp)
        ms.append(mp), ls.append(pp.sum(dim=-1, keepdim=True)), os_.append(pp @ v[:, :, keys])
    mmax = torch.stack(ms).amax(dim=0)
    w = [torch.exp(m - mmax) if weighted else torch.ones_like(m) for m in ms]
    return sum(wi * oi for wi, oi in zip(w, os_)) / sum(wi * li for wi, li in zip(w, ls))


def _halves(T):
    nkt = (T + 31) // 32
    nh0 = (nkt + 1) // 2
    return [list(range(nh0)), list(range(nh0, nkt))]


def m_mask_multiplied(c, fused):
    s, v = _scores(c, mask="mul")
    return _finish(c, _heads_out(torch.softmax(s, -1) @ v), fused)


def m_padded_keys_dropped(c, fused):
    s, v = _scores(c, mask="bool")
    return _finish(c, _heads_out(torch.softmax(s, -1) @ v), fused)


def m_mask_missing(c, fused):
    s, v = _scores(c, mask="none")
    return _finish(c, _heads_out(torch.softmax(s, -1) @ v), fused)


def m_scale_sqrt128(c, fused):
    s, v = _scores(c, scale=128 ** -0.5)
    return _finish(c, _heads_out(torch.softmax(s, -1) @ v), fused)


def m_heads_swapped(c, fused):
    s, v = _scores(c)
    return _finish(c, _heads_out(torch.softmax(s, -1) @ v, swap=True), fused)


def m_merge_without_weights(c, fused):
    return _finish(c, _heads_out(_grouped(c, A.part_tiles(c["T"], A.plan_attn(c["B"], c["T"])[1]), weighted=False)), fused)


def m_last_strided_tile_dropped(c, fused):
    groups = [t[:-1] if len(t) > 1 else t for t in A.part_tiles(c["T"], A.plan_attn(c["B"], c["T"])[1])]
    return _finish(c, _heads_out(_grouped(c, groups)), fused)


def m_halves_without_rescaling(c, fused):
    return _finish(c, _heads_out(_grouped(c, _halves(c["T"]), weighted=False)), fused)


def m_tail_reads_next_utterance(c, fused):
    nq, ntail = A.plan_attn_out(c["T"])
    assert ntail > 0
    x = c["qkv"].clone()
    x[:, 32 * nq:, :128] = c["qkv"].roll(-1, dims=0)[:, 32 * nq:, :128]
    s, v = _scores(c, qkv=x)
    return _finish(c, _heads_out(torch.softmax(s, -1) @ v), fused)


def m_h1_dropped(c, fused):
    s, v = _scores(c, qkv=A.quantised(c["qkv"], A.data_scales(c["qkv"]), pieces=1))
    return _finish(c, _heads_out(torch.softmax(s, -1) @ v), fused)


def m_bias_twice(c, fused):
    s, v = _scores(c)
    return _finish(c, _heads_out(torch.softmax(s, -1) @ v), fused, bias=2)


# (mutant, fused?, B, T, classes, the class whose rows must trip)
MUTANTS = [
    (m_mask_multiplied, False, 3, 129, ("randn", "flat", "quiet_keys"), "flat"),
    (m_padded_keys_dropped, False, 3, 129, ("randn", "flat", "pad_heavy"), "pad_heavy"),
    (m_mask_missing, False, 3, 129, ("randn", "mask_decides", "flat"), "mask_decides"),
    (m_scale_sqrt128, False, 3, 33, ("randn", "peaked", "large"), "randn"),
    (m_heads_swapped, True, 3, 36, ("randn", "flat", "tile_skew"), "flat"),
    (m_merge_without_weights, False, 3, 516, ("randn", "tile_skew", "peaked"), "tile_skew"),
    (m_last_strided_tile_dropped, False, 3, 516, ("randn", "tile_skew", "quiet_values"), "randn"),
    (m_halves_without_rescaling, True, 3, 65, ("randn", "tile_skew", "peaked"), "tile_skew"),
    (m_tail_reads_next_utterance, True, 3, 36, ("randn", "flat", "quiet_keys"), "randn"),
    (m_h1_dropped, True, 3, 132, ("randn", "quiet_keys", "large"), "randn"),
    (m_bias_twice, True, 3, 36, ("randn", "large", "peaked"), "large"),
]


@pytest.mark.parametrize("mutant,fused,B,T,classes,trips", MUTANTS, ids=[m[0].__name__[2:] for m in MUTANTS])
def test_mutants_trip_the_gate(mutant, fused, B, T, classes, trips):
    c = A.case(B, T, classes=classes, seed=T)
    refs = A.references(c, fused, scales=A.data_scales(c["qkv"]) if fused else None)
    fp16 = mutant is m_h1_dropped                              # (held to the wider of the two gates)
    # the unmutated evaluation in the same form passes
    s, v = _scores(c)
    ok, _ = A.failures(_finish(c, _heads_out(torch.softmax(s, -1) @ v), fused), c, refs, fp16=fp16)
    assert not ok, ok
    if mutant in (m_merge_without_weights, m_last_strided_tile_dropped):
        assert A.plan_attn(B, T)[0]
        exact, _ = A.failures(_finish(c, _heads_out(_grouped(c, A.part_tiles(T, A.plan_attn(B, T)[1]))), fused), c, refs)
        assert not exact, exact                                # the split itself, merged with its weights, is the reference
    bad, _ = A.failures(mutant(c, fused), c, refs, fp16=fp16)
    assert any(len(b) > 2 and b[1] == trips for b in bad), (trips, bad)


# ---------------------------------------------------------------------------------------------------------------------
# the split-key merge's order, in fp32: what the largest recorded ratio of the device test rests on
# ---------------------------------------------------------------------------------------------------------------------
def _flash_fp32(c, KS):
    """The kernels' arithmetic in fp32 torch: log2-domain scores from a pre-scaled q, 32-key tiles with a running maximum, exp2; KS = 0:
    all tiles in one sequence (attention_kernel); KS > 0: part p takes tiles p, p + KS, ... and the (m, l, O) states are merged in ascending
    part order with weights 2^(m_p - m_max) (attention_part_kernel + attention_merge_kernel)."""
    B, T, L2E = c["B"], c["T"], 1.4426950408889634
    q, k, v = A.split_heads(c["qkv"])
    m = A.key_mask(c["lengths"], T, F32)[:, None, None, :] * torch.tensor(L2E, dtype=F32)
    qs = q * torch.tensor(0.125 * L2E, dtype=F32)
    states = []
    for tiles in (A.part_tiles(T, KS) if KS else [list(range((T + 31) // 32))]):
        mr, lr, o = torch.full((B, 2, T, 1), -1e30), torch.zeros(B, 2, T, 1), torch.zeros(B, 2, T, 64)
        for t in tiles:
            ks = slice(32 * t, min(T, 32 * t + 32))
            sc = qs @ k[:, :, ks].transpose(-1, -2) + m[..., ks]
            mn = torch.maximum(mr, sc.amax(-1, keepdim=True))
            al, p = torch.exp2(mr - mn), torch.exp2(sc - mn)
            lr, o, mr = lr * al + p.sum(-1, keepdim=True), o * al + p @ v[:, :, ks], mn
        states.append((mr, lr, o))
    if not KS:
        out, l = states[0][2] * (1.0 / states[0][1]), states[0][1]
    else:
        mm = torch.stack([st[0] for st in states]).amax(0)
        l, o = torch.zeros_like(mm), torch.zeros(B, 2, T, 64)
        for mr, lr, op in states:
            w = torch.exp2(mr - mm)
            l, o = l + lr * w, o + op * w
        out = o * (1.0 / l)
    return out.transpose(1, 2).reshape(B * T, 128), l


def test_split_key_merge_order_in_fp32_stays_inside_the_gate():
    """3 x 1030, KS = 16, the tile_skew utterance: the dominant key sits in tile 32 = part 0, so the ascending merge starts from l ~ 1 and adds
    fifteen terms of about an ulp of it; the one-sequence order folds the small terms together first and rounds once.  Both orders, written
    in fp32 here, pass the gate; the merge order costs more of it (the device test records the kernel's own figure), and what it loses in l
    is bounded by fifteen half-ulps."""
    B, T = 3, 1030
    split, KS = A.plan_attn(B, T)
    assert split and KS == 16 and 32 in A.part_tiles(T, KS)[0]
    c = A.unfused_case(B, T)
    b = c["classes"].index("tile_skew")
    refs = A.references(c, False)
    seq, l_seq = _flash_fp32(c, 0)
    par, l_par = _flash_fp32(c, KS)
    bad_s, r_s = A.failures(seq, c, refs)
    bad_p, r_p = A.failures(par, c, refs)
    assert not bad_s and not bad_p, (bad_s, bad_p)
    worst = lambda r: max(v for (cls, _), v in r.items() if cls == "tile_skew")   # noqa: E731
    print(f"fp32 emulation, tile_skew rows of 3 x 1030: one sequence {worst(r_s):.2f}, split-key merge KS 16 {worst(r_p):.2f} (gate {A.MARGIN:.0f})")
    assert worst(r_s) < worst(r_p) < A.MARGIN
    # l in fp64 from the same tiles: the merge's l is short of it by at most 15 half-ulps of ~1 (+ the tiles' own roundings, one more ulp)
    s64 = A.split_heads(c["qkv"][b:b + 1].double())
    sc = s64[0] @ s64[1].transpose(-1, -2) / 8.0 + A.key_mask(c["lengths"][b:b + 1], T, F64)[:, None, None, :]
    l64 = torch.exp(sc - sc.amax(-1, keepdim=True)).sum(-1, keepdim=True)
    assert float((l_par[b:b + 1].double() - l64).abs().max()) <= (15 * 0.5 + 2) * 2.0 ** -23 * float(l64.max())


# ---------------------------------------------------------------------------------------------------------------------
# the shape table
# ---------------------------------------------------------------------------------------------------------------------
def test_shape_table_reaches_the_intended_builds():
    for B, T, tpw, scratch, want in A.UNFUSED:
        assert A.plan_attn(B, T, tpw=tpw, scratch=scratch) == want, (B, T, tpw, scratch)
        for S in (T + 4, T + 3):
            assert A.plan_attn(B, T, S=S, tpw=tpw, scratch=scratch) == want, (B, T, S)
    got = {(B, T, tpw): ks for B, T, tpw, sc, (split, ks) in A.UNFUSED if split}
    assert {got[(3, 97, 2)], got[(3, 128, 2)]} == {2} and got[(3, 129, 2)] == 3
    assert [len(t) for t in A.part_tiles(129, 3)] == [2, 2, 1]
    p = A.part_tiles(516, got[(3, 516, 2)])
    assert p[7] == [7, 16] and p[8] == [8]
    assert sorted(len(t) for t in A.part_tiles(1030, got[(3, 1030, 2)])) == [2] * 15 + [3] and got[(3, 1030, 2)] == A.MAXPARTS
    assert ((4096 + 127) // 128) * 2 * 1 == 64 and all(len(t) == 8 for t in A.part_tiles(4096, got[(1, 4096, 2)]))
    assert A.plan_attn(1, 4097) == (False, 0)                                  # (66 workgroups: 4096 is the last shape that splits)
    assert A.part_tiles(516, got[(3, 516, 1)])[0] == [0, 16] and got[(3, 516, 3)] == 6
    assert A.plan_attn(6, 516) == (True, 9) and A.plan_attn(7, 516) == (False, 0)
    assert A.plan_attn(3, 96) == (False, 0) and A.plan_attn(3, 97) == (True, 2)            # the nkt >= 4 threshold
    assert any(split for *_, (split, _) in A.UNFUSED) and any(not split for *_, (split, _) in A.UNFUSED)
    for B, T, want in A.FUSED:
        assert A.plan_attn_out(T) == want, T
    for B, T, first, want in A.FUSED_ALL:
        assert A.plan_attn_out(T) == want, T
    assert {nt for _, _, (_, nt) in A.FUSED} == {0, 1, 2, 3, 4}
    assert A.plan_attn_out(4) == (1, 0) and A.plan_attn_out(37) == (2, 0)
    assert {B % 8 == 0 for B, T, _ in A.FUSED if T == 36} == {True, False}
    # every class meets every path: both un-fused builds, the fused main path and the tail path
    for split in (False, True):
        seen = set()
        for B, T, tpw, sc, (sp, _) in A.UNFUSED:
            if sp == split:
                seen |= set(A.unfused_case(B, T)["classes"])
        assert seen == set(A.CLASSES), (split, set(A.CLASSES) - seen)
    for T in (132, 36):
        assert {n for B, TT, first, _ in A.FUSED_ALL if TT == T for n in A.case(B, T, first)["classes"]} == set(A.CLASSES)
