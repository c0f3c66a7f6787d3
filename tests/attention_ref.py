"""The U-Net's self-attention restated in plain torch, the inputs that stress it, and the per-row gates its kernels are held to.

What is restated (Matcha-TTS matcha/models/components/transformer.py:262-271, diffusers Attention with a FLOAT mask; the repository's own
statement of it is oracle/matcha_oracle.py:194-216, and the kernels cite the same lines):

    scores[q, key] = q . k / 8 + m[key]          m = 1.0 for key < length, 0.0 for the padded frames (length <= key < T)
    p = softmax over ALL T keys                  (the mask is ADDED: padded frames stay live keys, e^-1 lighter)
    att = concat_heads(p v)                      (two heads of 64)
    fused form: hid + att Wout^T + bout

Every one of the T query rows has a value, the rows t >= length too: the mask acts on keys only.  Nothing here imports the engine; every
function runs in the dtype of its inputs, so the same code gives the fp64 reference and the fp32 yardstick.

Gates.  Per QUERY ROW — the 128-wide attention output of the un-fused op, the 256-wide attention term (out - hid - bout) of the fused op, so
that the residual cannot hide it — and for both the RMS and the L-inf of (kernel - fp64):

    error <= max(MARGIN x yardstick x this row's fp64 RMS, FLOOR x this row's fp64 L-inf)          MARGIN = 4, FLOOR = 2^-21

The yardstick is a relative error, the worst over the rows of the same input class in the same case, derived here and never from a kernel:
  * fp32 builds (attention_kernel, attention_part_kernel + attention_merge_kernel, attn_out_kernel, attn_tail_path<false>): the error of
    the plain fp32 evaluation of the functions below on the CPU.
  * fp16 builds (attn_out_h16_kernel, attn_tail_path<true>): that, PLUS the representation error of the fp16 form — q, k, v and Wout replaced
    by what two fp16 pieces times a power of two hold (pack(), restating qkv_pack_kernel and pack_conv's weight pieces), evaluated in fp64
    and compared with the fp64 result of the original operands.  Where a tensor's scale comes from a bound far above the data
    (below_bound), the form's absolute floor 2^-25 / scale is what this term carries.  attn_out_h16_kernel holds a THIRD tensor in the form:
    the merged, normalised attention rows, which it splits into two fp16 pieces in units of sv (evh_split4 on O sv) as the B operand of its
    fp16 projection.  Under data-derived scales that is 2^-22 relative like everything else; under below_bound scales the rows sit 2^10 and
    more below the range and keep the same absolute floor 2^-25 / sv as v itself (measured before this term was modelled: 4.74 x the
    q / k / v / Wout yardstick on the quiet_keys rows of 4 x 132, whose attention term is small; error 1.2e-6 = the floor 2^-19 through the
    projection).  So the model quantises the attention rows too: pack(att, sv) between the softmax and the projection.  attn_tail_path<true>
    decodes q, k, v to fp32 and projects in fp32 with the fp32 weights: its rows get the q / k / v representation error only.
MARGIN = 4 covers what separates a flash-style fp32 evaluation (32-key tiles, running maximum, exp2 on log2-domain scores, MFMA
accumulation order) from torch's row-at-a-time softmax: a different order of the same roundings.  No term beyond these is in the yardstick.

Input classes (CLASSES; each fills one utterance, a case mixes them; data is non-zero at the padded frames throughout):
  randn         N(0, 1)
  peaked        q, k x 5: scores of +-60, one key takes the softmax
  flat          q = 0: only the mask shapes the softmax, padded keys weigh e^-1
  mask_decides  the key that wins q . k / 8 (by 0.5) is a padded frame; the best valid key overtakes it only through the +1.0
  pad_heavy     length 1: T - 1 padded keys carry the mass
  quiet_keys    every other key 2^-12 below the rest          quiet_values   every other value 2^-12 below the rest
  large         x 300, q x 1e-3 on top: values near the top of any scaled range, scores still moderate (fp32 rounding of a score near 300
                is 3e-5, and it sits in an exponent: the plain fp32 evaluation carries it, so the yardstick does)
  tile_skew     one dominant key (score 20 above the rest) at frame T - 1, in the last 32-key tile; all other scores are tiny, so every
                other key tile / key half / split-key part has a running maximum ~20 below the merged one
below_bound is not a class but a choice of scales (fp16 builds only): bound_scales(), the powers of two qkv_pack_scales would derive from a
weight bound 2^10 above the data's maxima.
"""
import math

import torch

import norm_ref as N

MARGIN = N.MARGIN
FLOOR = N.FLOOR
RMS_FLOOR = 1e-3          # every gated row's fp64 RMS is above this (asserted on the CPU): no row is gated against nothing
HEADS = 2
HD = 64
CLASSES = ("randn", "peaked", "flat", "mask_decides", "pad_heavy", "quiet_keys", "quiet_values", "large", "tile_skew")
BOUND_SHIFT = 10          # below_bound: the weight bound sits 2^10 above the data's maximum


# ---------------------------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------------------------
def key_mask(lengths, T, dtype):
    """(B, T): 1.0 inside the length, 0.0 on the padded frames — a float that is ADDED to the scores."""
    return (torch.arange(T)[None, :] < lengths.long()[:, None]).to(dtype)


def split_heads(qkv):
    """(B, T, 384) -> q, k, v each (B, 2, T, 64)"""
    B, T, _ = qkv.shape
    return tuple(qkv[..., i * 128:(i + 1) * 128].reshape(B, T, HEADS, HD).transpose(1, 2) for i in range(3))


def attention(qkv, lengths):
    """(B, T, 384), (B,) -> (B, T, 128): softmax(q k^T / 8 + m[key]) v over all T keys, heads concatenated."""
    B, T, _ = qkv.shape
    q, k, v = split_heads(qkv)
    s = q @ k.transpose(-1, -2) / 8.0 + key_mask(lengths, T, qkv.dtype)[:, None, None, :]
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, HEADS * HD)


def attn_out(qkv, lengths, w_out, b_out, hid):
    """hid + attention(qkv) Wout^T + bout: (B, T, 256)"""
    return hid + attention(qkv, lengths) @ w_out.T + b_out


# ---------------------------------------------------------------------------------------------------------------------
# the fp16 form: x s = h0 + h1, two fp16 numbers; decoded (h0 + h1) / s
# ---------------------------------------------------------------------------------------------------------------------
def pack(x, s):
    """qkv_pack_kernel's arithmetic on fp32 x: c = x s (fp32), h0 = fp16(c), h1 = fp16(c - h0).  Returns (h0, h1) as fp32 tensors."""
    c = x.float() * float(s)
    h0 = c.half().float()
    h1 = (c - h0).half().float()
    return h0, h1


def unpack(h0, h1, s):
    return (h0.double() + h1.double()) / float(s)


def pow2_scale(mx, top=32768.0, shift=0):
    """The power of two that maps mx 2^shift into (top / 2, top] (ev_op_attn_out: mx = the data's maximum; qkv_pack_scales: mx 2^shift = the
    weight bound), exponent clamped to +-40 as the engine clamps it."""
    if not mx > 0.0:
        return 1.0
    e = int(math.floor(math.log2(top / (mx * 2.0 ** shift))))
    return 2.0 ** min(40, max(-40, e))


def data_scales(qkv, shift=0):
    """(sq, sk, sv) from the maxima of the three tensors (shift = BOUND_SHIFT: as from a weight bound that far above them)."""
    return tuple(pow2_scale(float(qkv[..., i * 128:(i + 1) * 128].abs().max()), shift=shift) for i in range(3))


def bound_scales(qkv):
    return data_scales(qkv, BOUND_SHIFT)


def weight_scale(w):
    """pack_conv's power of two for the fp16 weight pieces: the largest |w| lands in [8192, 16384)."""
    mx = float(w.abs().max())
    if not mx > 0.0:
        return 1.0
    _, ex = math.frexp(mx)
    return 2.0 ** max(-40, min(40, 14 - ex))


def mask_split(sq, sk):
    """attn_mask_split restated: the frame mask in accumulator units is 8 sq sk, an exact power of two, split into two fp16 NUMBERS
    (normal range 2^-14 .. 2^15).  Returns (mask_a, mask_b) or None where no such split exists."""
    mq, eq = math.frexp(sq)
    mk, ek = math.frexp(sk)
    if not (sq > 0 and sk > 0 and mq == 0.5 and mk == 0.5):
        return None
    e = 3 + (eq - 1) + (ek - 1)
    ea = min(15, max(-14, int(e / 2)))          # (C++ integer division truncates toward zero)
    eb = e - ea
    if eb < -14 or eb > 15:
        return None
    return 2.0 ** ea, 2.0 ** eb


def quantised(qkv, scales, pieces=2):
    """q, k, v as the fp16 form holds them, in fp64 (pieces = 1: the h1 piece dropped)."""
    out = torch.empty_like(qkv, dtype=torch.float64)
    for i, s in enumerate(scales):
        h0, h1 = pack(qkv[..., i * 128:(i + 1) * 128], s)
        out[..., i * 128:(i + 1) * 128] = unpack(h0, h1 if pieces == 2 else torch.zeros_like(h1), s)
    return out


def quantised_weight(w, pieces=2):
    s = weight_scale(w)
    h0, h1 = pack(w, s)
    return unpack(h0, h1 if pieces == 2 else torch.zeros_like(h1), s)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def fill(cls, T, L, g):
    """One utterance of class cls: (qkv (T, 384), length).  pad_heavy forces length 1, mask_decides a length below T."""
    x = torch.randn(T, 384, generator=g)
    if cls == "randn":
        pass
    elif cls == "peaked":
        x[:, :256] *= 5.0
    elif cls == "flat":
        x[:, :128] = 0.0
    elif cls == "pad_heavy":
        L = 1
    elif cls == "quiet_keys":
        x[::2, 128:256] *= 2.0 ** -12
    elif cls == "quiet_values":
        x[::2, 256:384] *= 2.0 ** -12
    elif cls == "large":
        x *= 300.0
        x[:, :128] *= 1e-3
    elif cls in ("mask_decides", "tile_skew"):
        if cls == "mask_decides" and T > 1:
            L = min(L, T - 1)
        for h in range(HEADS):
            u = torch.randn(HD, generator=g)
            u /= u.norm()
            q = slice(h * HD, (h + 1) * HD)
            k = slice(128 + h * HD, 128 + (h + 1) * HD)
            x[:, q] = 8.0 * u + 0.3 * x[:, q]                 # q . u = 8 (+ noise): a key c u scores c
            x[:, k] *= 0.1                                    # every other key: scores of ~0.1
            if cls == "tile_skew":
                x[T - 1, k] = 20.0 * u
            elif T > 1:
                x[T - 1, k] = 12.0 * u                        # a padded frame (T - 1 >= L): 12 before the mask
                x[(L - 1) // 2, k] = 11.5 * u                 # a valid frame: 11.5, 12.5 with the +1.0
    else:
        raise ValueError(cls)
    return x, L


def case(B, T, first=0, seed=None, classes=None, lengths=None):
    """A case: B utterances of T frames, utterance j of class CLASSES[(first + j) % 9] (or classes[j]), ragged lengths (T, 2T/3, T - 1 or 1 by
    turns; or lengths[j]), one projection and one hidden tensor.  Deterministic in its arguments."""
    g = torch.Generator().manual_seed(1000 * T + 10 * B + first if seed is None else seed)
    names = [CLASSES[(first + j) % len(CLASSES)] for j in range(B)] if classes is None else list(classes)
    qkv = torch.empty(B, T, 384)
    L = []
    for j, name in enumerate(names):
        want = (T, max(1, (2 * T) // 3), 1 if (first + j) % 2 else max(1, T - 1))[j % 3] if lengths is None else int(lengths[j])
        qkv[j], l = fill(name, T, want, g)
        L.append(l)
    return {"B": B, "T": T, "qkv": qkv, "lengths": torch.tensor(L, dtype=torch.int32), "classes": names,
            "cls": torch.tensor([CLASSES.index(n) for n in names]).repeat_interleave(T),
            "hid": 0.25 * torch.randn(B, T, 256, generator=g), "w_out": torch.randn(256, 128, generator=g) / 128 ** 0.5,
            "b_out": 0.1 * torch.randn(256, generator=g)}


def evaluate(c, fused, dtype, qkv=None, w_out=None):
    """The restatement on case c in dtype: (B*T, 128) attention rows, or (B*T, 256) rows of the fused form.  qkv / w_out override the case's
    (the quantised operands)."""
    x = (c["qkv"] if qkv is None else qkv).to(dtype)
    if not fused:
        return attention(x, c["lengths"]).reshape(c["B"] * c["T"], 128)
    w = (c["w_out"] if w_out is None else w_out).to(dtype)
    return attn_out(x, c["lengths"], w, c["b_out"].to(dtype), c["hid"].to(dtype)).reshape(c["B"] * c["T"], 256)


def residual(c):
    """What the fused form adds the attention term to: hid + bout, fp64, (B*T, 256)"""
    return (c["hid"].double() + c["b_out"].double()).reshape(c["B"] * c["T"], 256)


# ---------------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------------
def references(c, fused, scales=None):
    """Everything a gate needs, computed once per (case, form, scales) and never changed: the fp64 rows, the rows the error is taken
    relative to (fused: the attention term), and the two yardsticks as (2, classes) worst relative (rms, linf) errors.  scales: the
    (sq, sk, sv) of the fp16 form (None: no fp16 yardstick)."""
    ref = evaluate(c, fused, torch.float64)
    base = residual(c) if fused else torch.zeros_like(ref)
    term = ref - base
    n = len(CLASSES)
    y32 = N.class_worst(N.row_errors(evaluate(c, fused, torch.float32).double() - base, term), c["cls"], n)
    out = {"ref": ref, "base": base, "term": term, "yard32": y32, "yard16": None, "yard16_tail": None}
    if scales is not None:
        xq = quantised(c["qkv"], scales)
        if fused:
            att = attention(xq, c["lengths"])
            h0, h1 = pack(att, scales[2])                                  # the attention rows in the form, at v's scale
            rep = (c["hid"].double() + unpack(h0, h1, scales[2]) @ quantised_weight(c["w_out"]).T + c["b_out"].double()).reshape(ref.shape)
            rep_tail = evaluate(c, True, torch.float64, qkv=xq)
        else:
            rep = rep_tail = evaluate(c, False, torch.float64, qkv=xq)
        out["yard16"] = y32 + N.class_worst(N.row_errors(rep - base, term), c["cls"], n)
        out["yard16_tail"] = y32 + N.class_worst(N.row_errors(rep_tail - base, term), c["cls"], n)
    return out


def failures(got, c, refs, fp16=False, tag="", keep=None):
    """Rows of got (fp32, (B*T, width)) over their gate.  fp16 picks the yardstick:
      False    the plain fp32 evaluation (every fp32 build)
      True     that plus the representation error of q, k, v, Wout and the attention rows at v's scale (attn_out_h16_kernel)
      "tail"   that plus the representation error of q, k, v only (attn_tail_path<true>)
    Every row of the case is gated; keep is a row mask for a caller that reports the rows of two code paths apart — between them its calls
    cover every row, and the yardstick stays the whole class's.  Returns (failures, {(class, kind): worst error / (yardstick x row RMS)}):
    the ratio is a report (the gate sits at MARGIN), the gate is what is asserted."""
    yard = refs["yard32"] if not fp16 else (refs["yard16_tail"] if fp16 == "tail" else refs["yard16"])
    err = N.row_errors(got.double().reshape(refs["ref"].shape) - refs["base"], refs["term"])
    bad, ratios = [], {}
    if not bool(torch.isfinite(err[:2]).all()):
        bad.append((tag, "non-finite output"))
    for k, name in enumerate(CLASSES):
        sel = (c["cls"] == k) if keep is None else ((c["cls"] == k) & keep)
        if not bool(sel.any()):
            continue
        for i, kind in enumerate(("rms", "linf")):
            gate = torch.maximum(MARGIN * yard[i, k] * err[2][sel], FLOOR * err[3][sel])
            e = err[i][sel]
            over = ~(e <= gate)
            if bool(over.any()):
                j = int((e / gate).nan_to_num(nan=float("inf")).argmax())
                bad.append((tag, name, kind, f"{int(over.sum())} of {int(sel.sum())} rows over the gate; worst error {float(e[j]):.3e} gate "
                                             f"{float(gate[j]):.3e} yardstick (relative) {float(yard[i, k]):.3e}"))
            ratios[(name, kind)] = float((e / torch.maximum(yard[i, k] * err[2][sel], FLOOR * err[3][sel] / MARGIN)).nan_to_num(nan=float("inf")).max())
    return bad, ratios


# ---------------------------------------------------------------------------------------------------------------------
# the launch rules, restated from launch_attn and launch_attn_out (ev_engine.hip), and the shapes the GPU test runs
# ---------------------------------------------------------------------------------------------------------------------
MAXPARTS, MAXROWS, TAILQ = 16, 8192, 4


def plan_attn(B, T, S=None, tpw=2, scratch=True, heads=HEADS):
    """launch_attn: (split-key?, KS)."""
    S = T if S is None else S
    nwg, nkt = ((T + 127) // 128) * heads * B, (T + 31) // 32
    if scratch and nwg <= 64 and nkt >= 4 and B * S <= MAXROWS:
        return True, min(MAXPARTS, (nkt + tpw - 1) // tpw)
    return False, 0


def part_tiles(T, KS):
    """attention_part_kernel: the key tiles of part p are p, p + KS, ..."""
    nkt = (T + 31) // 32
    return [list(range(p, nkt, KS)) for p in range(KS)]


def plan_attn_out(T):
    """launch_attn_out: (nq, ntail) — a last tile of 1..4 queries goes to attn_tail_path, unless it is the only tile."""
    nq = (T + 31) // 32
    last = T - 32 * (nq - 1)
    if nq >= 2 and last <= TAILQ:
        return nq - 1, last
    return nq, 0


# un-fused op: (B, T, tpw, scratch, (split, KS))
UNFUSED = (
    # attention_kernel: the 32-key tile, the 128-query workgroup, the inactive waves.  T <= 96 has fewer than 4 key tiles: one launch even with scratch
    [(3, T, 2, True, (False, 0)) for T in (1, 31, 32, 33, 96)] + [(3, T, 2, False, (False, 0)) for T in (127, 128, 129, 260)]
    # split-key, 2 tiles per part: 97 / 128 two parts; 129 uneven parts (2, 2, 1); 516 part 7 = tiles 7, 16, part 8 = tile 8; 1030 KS capped;
    # 4096 x 1: 64 workgroups, the last shape that splits, 8 tiles per part.  And the one-launch kernel at the same shapes.
    + [(B, T, 2, sc, (sc, KS if sc else 0)) for B, T, KS in ((3, 97, 2), (3, 128, 2), (3, 129, 3), (3, 516, 9), (3, 1030, 16), (1, 4096, 16))
       for sc in (True, False)]
    # other tiles per part, on fresh handles: KS = 16 (part 0 = tiles 0, 16), KS = 6
    + [(3, 516, 1, True, (True, 16)), (3, 516, 3, True, (True, 6))]
    # the nwg <= 64 edge: 60 workgroups split, 70 do not
    + [(6, 516, 2, True, (True, 9)), (7, 516, 2, True, (False, 0))]
)
# fused op: (B, T, (nq, ntail)) — run under arithmetic 16 with the fp16 attention on and off, and under arithmetic 0
FUSED = (
    # key halves: one key tile (half 1 of each head empty), 2, 3 (halves of 2 and 1; a tail of 1 beside it), 3 tiles
    [(3, T, plan) for T, plan in ((32, (1, 0)), (64, (2, 0)), (65, (2, 1)), (96, (3, 0)))]
    # the tail path and its neighbours: ntail 1..4; 37 a ragged full-size tile; the model's 258 and 516; T = 4 a single tile, no tail path
    + [(3, T, plan) for T, plan in ((33, (1, 1)), (34, (1, 2)), (35, (1, 3)), (36, (1, 4)), (37, (2, 0)), (258, (8, 2)), (516, (16, 4)), (4, (1, 0)))]
    # xcd_map (B % 8 == 0) on and off, tail present
    + [(B, 36, (1, 4)) for B in (8, 16, 5, 9)]
)
# fused op, every class, data-derived and below-bound scales: (B, T, first class, (nq, ntail))
FUSED_ALL = [(4, T, first, plan) for T, plan in ((132, (4, 4)), (36, (1, 4))) for first in (0, 4, 8)]


def _first(table, B, T):
    keys = list(dict.fromkeys((b, t) for b, t, *_ in table))
    return (3 * keys.index((B, T))) % len(CLASSES)


def unfused_first(B, T):
    """The class of utterance 0 of the un-fused case (B, T): the table's shapes take the classes three at a time, by turns."""
    return _first(UNFUSED, B, T)


def fused_first(B, T):
    return _first(FUSED, B, T)


def unfused_case(B, T):
    """The un-fused case of shape (B, T).  The one utterance of 4096 frames is a tile_skew one: 128 key tiles, 16 parts."""
    return case(B, T, classes=("tile_skew",)) if B == 1 else case(B, T, unfused_first(B, T))
