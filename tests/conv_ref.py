"""fp64 restatement of the conv GEMM family with its fused epilogue, the inputs that stress it, the per-frame gates and the mutants.

Restatement (plain torch, no engine code; every function runs in the dtype of its inputs: fp64 for the reference, fp32 on the CPU for the
yardstick the gates are derived from).  The conv is a sum over taps of shifted matmuls, not F.conv1d:
  same    on the flattened padded axis the kernels walk: utterance b, frame t is row b * S + P + t, S = T + 2 P, pad rows zero, and
          v[n] = sum_k X[n + k d - (K - 1) d / 2] W_k^T — the pad rows ARE the zero padding (ev_kernels.h).  Any P >= the halo gives the same sums.
  s2      k = 3, stride 2, padding 1:   v[t'] = W_0 x[2t' - 1] + W_1 x[2t'] + W_2 x[2t' + 1]
  T       ConvTranspose1d, K - 2 p = s:  v[s q + k - p] += W_k^T x[q]
then the epilogue in the order documented above ConvParams:
  +bias, act, *mask1, *scale, +R, +Yold, /3, lrelu(act2_slope), *mask2      and      Y2 = v * rowmask.

Magnitude.  A(b, c, t) is the same expression over |lrelu_pro(x)|, |w|, |bias|, |scale|, |R|, |Yold| (masks left out; the activation as the
bound of its slope: 1 for none / leaky-relu / tanh, 1.1 for SiLU and Mish, 1 + alpha_exp * beta_inv per channel for SnakeBeta; /3 kept).  It is
the natural scale of an output element — what its rounding errors are proportional to — and includes whatever the frame's halo reaches, so a
quiet frame is judged at its own scale.

Input classes (fill): randn | mixed (every 7th frame x 1e-3) | rows (utterances at 1e-3, 1, 1e3) | channels (10^(-1.5 .. 1.5) across Cin) |
offset (mean 50) | zero | tiny (1e-6) | huge (1e4).  Within any window of 256 + halo rows of the flattened axis the frame scales stay within
2^12 (window_range; asserted in tests/test_conv_reference.py), so the absolute floor of DESIGN section 3.1 never applies; wider ranges are
the subject of tests/test_gpu_precision.py.

Gates.  Per output frame (b, t), for the L-inf and the RMS over channels of (got - fp64):
    error <= max(MARGIN x yardstick x rms_c A(b, :, t),  FLOOR x max_c |fp64(b, :, t)|)  +  c_pipe x {max_c A | rms_c A}
yardstick = the worst (error of the plain fp32 evaluation / rms_c A) over the frames of the same case (one case = one layer, class and
epilogue), MARGIN = 4, FLOOR = 2^-21: the rule of norm_ref.py; no build has a wider margin.  The plain fp32 evaluation takes the SAME sums
in the order of an accumulator (conv_chain): one chain per output element that starts at the bias — the lean epilogues preload it — and
adds one (tap, input channel) product at a time, n = Cin K roundings at the magnitude of the running sum.  A blocked matmul is no such
evaluation: its partial sums are short, the bias joins last, and which blocks it takes depends on the BLAS of the machine.  Against it the
exact fp32 MFMA chain of a 512-channel 11-tap layer stands 8 x off, and a bias of 0.1 over a conv sum of 1e-6 (class tiny) 60 x — both are
the order of summation, not errors; the chain is the fp32 evaluation of that order, and it is the same on every machine.  MARGIN then
covers what remains: k-chunks and taps in another sequence, two products per MFMA step, split-K partial tiles, the bias added last in the
generic epilogues.
c_pipe is 0 on the fp32 pipe (builds 0, 1, 2, 5, 6, 8, 9, 19, 56).  On the 16-bit pipes it is derived from the piece arithmetic alone:
  fp16 (46, 47, 66)   C_FP16 = 3 x 2^-22 per product: each operand is two fp16 pieces good to 2^-22, and the dropped
                      h1 g1 is at most 2^-22 |x w|.  Every |x w| is a term of A, so the sum of the per-product bounds is C_FP16 x A.
  bf16 (40, 41, 60)   x = x0 + x1 + x2 exactly, each piece a truncation to 8 significand bits: |x1| < 2^-7 |x|, |x2| < 2^-14 |x|, the same for
                      w.  Six products are kept (piece indices summing to <= 2); dropped are x1 w2 and x2 w1 (< 2^-21 |x w| each) and x2 w2
                      (< 2^-28): C_BF16 = 2^-20 + 2^-28.
c_pipe x A is a worst-case bound: it grows with the length n = Cin K of the contraction, a random-sign slip only with sqrt(n).  So the
16-bit gates tell x rounded to fp16 apart (30 .. 110 x) but not a lost third bf16 piece (4.5 x on the shortest contraction, the 64 -> 128
k1 layer; 1.4 x at Cin K = 1792): that mutant is held to the fp32-pipe gate, which it exceeds 13 x on k1 (tests/test_conv_reference.py
prints every ratio).  What the 16-bit pipes lose beyond their pieces is measured by tests/test_gpu_precision.py.
Masked frames are part of the gate: exactly 0 where the mask comes last (or nothing is added after mask1), exactly R (+ Yold) in fp32 where
mask1 is followed by +R, and Y2 exactly y * m.  Nothing here is derived from a kernel's output.

Mutants (wrong references, evaluated in fp64; MUTANTS maps each to the case that shows it):
  tapdrop      last tap dropped on the frames at rows 127 / 128 of the flattened axis
  padleak      the pad row in front of utterances 1.. holds the previous utterance's last frame
  prohalo      prologue leaky-relu skipped on rows outside the 128-row tile of the output row (a tile's halo rows)
  biasshift    bias of channel c + 1 on the last, partial 64-channel tile
  scale_late   scale applied after +R           mask_late   mask1 applied after +R          div3_early   /3 before +Yold
  act2_slope   act2 slope 0.1 in place of the caller's          snake_swap   SnakeBeta with alpha_exp and beta_inv swapped
  x_fp16       x rounded to fp16 (second piece lost)            x_bf16x2     x truncated to two bf16 pieces"""
import torch

MARGIN = 4.0
FLOOR = 2.0 ** -21
C_FP16 = 3.0 * 2.0 ** -22
C_BF16 = 2.0 ** -20 + 2.0 ** -28
A_RMS_FLOOR = 1e-3            # every gated frame's rms_c A is above this (asserted on the CPU): no frame is gated against nothing
WINDOW = 256                  # largest tile (rows) of any build; the dynamic-range window is WINDOW + halo rows
RANGE_LIMIT = 2.0 ** 12

FP32_BUILDS = (0, 1, 2, 5, 6, 8, 9, 19, 56)
FP16_BUILDS = (46, 47, 66)
BF16_BUILDS = (40, 41, 60)


def c_pipe(build):
    return C_FP16 if build in FP16_BUILDS else C_BF16 if build in BF16_BUILDS else 0.0


CLASSES = ("randn", "mixed", "rows", "channels", "offset", "zero", "tiny", "huge")

# ---------------------------------------------------------------------------------------------------------------------
# layers: form same | s2 | T; B utterances of T input frames, P pad rows a side (input frames)
# T and P are chosen so that S = T + 2 P is no multiple of 32: the 32-, 64-, 128-, 192- and 256-row tiles straddle utterances and the last
# tile of the B S rows is partial.  S > 256 + halo on the layers that carry the `rows` class.
# ---------------------------------------------------------------------------------------------------------------------
def _layer(form, Cin, Cout, K, d=1, stride=1, padding=None, B=3, T=333, P=0):
    if padding is None:
        padding = (K - 1) * d // 2 if form == "same" else 1
    return {"form": form, "Cin": Cin, "Cout": Cout, "K": K, "d": d, "stride": stride, "padding": padding, "B": B, "T": T, "P": P}


LAYERS = {
    "k3": _layer("same", 128, 128, 3, T=333, P=1),                 # S = 335: rows 127 / 128 are frames of utterance 0
    "k7d3": _layer("same", 256, 256, 7, d=3, T=301, P=10),         # S = 321
    "k11d5": _layer("same", 512, 128, 11, d=5, T=190, P=25),       # S = 240, halo 50 rows in all
    "k1": _layer("same", 64, 128, 1, T=333, P=0),                  # no pad rows at all
    "c224": _layer("same", 224, 80, 3, T=333, P=2),                # Kpad 256 > Cin, Cout = 80: a partial 64-channel tile
    "c80": _layer("same", 80, 64, 7, T=333, P=4),                  # Kpad 96 > Cin
    "c32": _layer("same", 32, 32, 3, T=333, P=1),
    "post": _layer("same", 32, 1, 7, T=333, P=3),                  # Cout = 1: scalar stores
    "s2": _layer("s2", 128, 128, 3, stride=2, T=332, P=2),         # pair view: 168 rows an utterance
    "t2": _layer("T", 128, 32, 4, stride=2, padding=1, T=300, P=1),     # packed Cout 64
    "t8": _layer("T", 128, 24, 16, stride=8, padding=4, T=150, P=1),    # packed Cout 192
    "k7_t1": _layer("same", 256, 256, 7, d=3, T=1, P=9),           # one frame an utterance
    "k7_t5": _layer("same", 256, 256, 7, d=3, T=5, P=9),           # T shorter than the halo
    # the balanced builds, by the engine's own choice at 256 CUs (derivation: tests/test_gpu_conv.py)
    "bal56": _layer("same", 128, 512, 3, B=16, T=500, P=8),        # 8256 rows
    "bal3": _layer("same", 256, 256, 3, B=16, T=500, P=8),         # 3 taps: nine staging passes of the fp16 balanced build
    "bal7": _layer("same", 256, 256, 7, d=3, B=16, T=484, P=16),   # 7 taps, halo 18: twelve
}


def out_frames(L):
    return L["T"] if L["form"] == "same" else L["T"] // 2 if L["form"] == "s2" else L["T"] * L["stride"]


def halo_rows(L):
    """halo rows a side of the view the kernel walks"""
    if L["form"] == "same":
        return (L["K"] - 1) * L["d"] // 2
    return 1 if L["form"] == "s2" else max((L["K"] - 1 - L["padding"]) // L["stride"], (L["stride"] - 1 + L["padding"]) // L["stride"])


# ---------------------------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------------------------
def lrelu(v, slope):
    return torch.where(v >= 0, v, v * slope)


def mish(x):
    sp = torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))
    return x * torch.tanh(sp)


def flatten(x, P):
    """(B, C, T) -> (B S, C) rows b S + P + t, pad rows zero"""
    B, Cc, T = x.shape
    Xf = torch.zeros(B, T + 2 * P, Cc, dtype=x.dtype)
    Xf[:, P:P + T] = x.transpose(1, 2)
    return Xf.reshape(B * (T + 2 * P), Cc)


def conv_same(x, w, d, P, pro_slope=-1.0, mut=None):
    """'same' conv on the flattened padded axis; x (B, Cin, T), w (Cout, Cin, K) -> (B, Cout, T)"""
    B, Cin, T = x.shape
    K = w.shape[2]
    S, H = T + 2 * P, (K - 1) * d // 2
    assert P >= H, "pad rows fewer than the halo"
    Xf = flatten(x, P)
    if mut == "padleak":
        for b in range(1, B):
            Xf[b * S + P - 1] = x[b - 1, :, T - 1]
    Xl = lrelu(Xf, pro_slope) if pro_slope >= 0 else Xf
    n = B * S
    z = torch.zeros(H, Cin, dtype=x.dtype)
    Xp, Xr = torch.cat([z, Xl, z]), torch.cat([z, Xf, z])
    rows = torch.arange(n)
    v = torch.zeros(n, w.shape[0], dtype=x.dtype)
    for k in range(K):
        off = k * d - H
        src = Xp[H + off:H + off + n]
        if mut == "prohalo":
            outside = ((rows + off) // 128) != (rows // 128)
            src = torch.where(outside[:, None], Xr[H + off:H + off + n], src)
        term = src @ w[:, :, k].T
        if mut == "tapdrop" and k == K - 1:
            term[127:129] = 0
        v = v + term
    return v.reshape(B, S, -1)[:, P:P + T].transpose(1, 2).contiguous()


def conv_s2(x, w):
    B, Cin, T = x.shape
    xp = torch.zeros(B, Cin, T + 2, dtype=x.dtype)
    xp[:, :, 1:T + 1] = x
    v = 0
    for k in range(3):
        v = v + w[:, :, k] @ xp[:, :, k:k + T:2]
    return v


def conv_T(x, w, s, p):
    """w (Cin, Cout, K)"""
    B, Cin, T = x.shape
    K = w.shape[2]
    full = torch.zeros(B, w.shape[1], (T - 1) * s + K, dtype=x.dtype)
    for k in range(K):
        full[:, :, k:k + (T - 1) * s + 1:s] += w[:, :, k].T @ x
    return full[:, :, p:p + T * s].contiguous()


def conv(L, x, w, pro_slope=-1.0, mut=None, P=None):
    if L["form"] == "same":
        return conv_same(x, w, L["d"], L["P"] if P is None else P, pro_slope, mut)
    if pro_slope >= 0:
        x = lrelu(x, pro_slope)
    return conv_s2(x, w) if L["form"] == "s2" else conv_T(x, w, L["stride"], L["padding"])


# epilogues: the combinations production uses (ev_engine.hip, the Epi sites).  Keys absent = off.
DT = 0.1
EPIS = {
    "plain": {},
    "nobias": {"bias": False},
    "pro_R": {"pro": 0.1, "R": True},
    "pro_lrelu": {"pro": 0.1, "act": "lrelu", "act_slope": 0.1},
    "relu_m1": {"act": "lrelu", "act_slope": 0.0, "mask1": True},
    "m1_R": {"mask1": True, "R": True},
    "R_m2": {"R": True, "mask2": True},
    "snake": {"act": "snake"},
    "mrf0": {"pro": 0.1, "R": True},
    "mrf1": {"pro": 0.1, "R": True, "accum": True},
    "mrf2": {"pro": 0.1, "R": True, "accum": True, "div3": True, "act2": 0.25},
    "sum3": {"R": True, "accum": True, "div3": True, "act2": 0.25},            # the accumulate flavour without a prologue (conv_sk32_kernel takes none)
    "euler": {"mask1": True, "scale": DT, "R": True, "y2": True},
    "tanh": {"act": "tanh"},
    "silu": {"act": "silu"},
    "mish": {"act": "mish"},
}
LEAN_EPIS = ("plain", "nobias", "pro_R", "pro_lrelu", "relu_m1", "m1_R", "R_m2", "snake", "mrf1", "mrf2", "sum3")   # lean_ok on a Cout % 4 == 0 layer
ACC_EPIS = ("mrf1", "mrf2")                                                                                    # the accumulate flavour (3)
FULL_EPIS = ("tanh", "silu", "mish")
ACT_LIP = {"none": 1.0, "lrelu": 1.0, "tanh": 1.0, "silu": 1.1, "mish": 1.1}


def conv_chain(L, x, w, bias, pro_slope=-1.0):
    """The conv sum as ONE accumulator chain per output element, in the dtype of x: the accumulator starts at the bias (as the kernels'
    lean epilogues preload it) and takes one (tap, input channel) product at a time — the order of an MFMA accumulator, which a blocked
    matmul is not.  In fp32 this is the yardstick of the gates; bias may be None."""
    if pro_slope >= 0:
        x = lrelu(x, pro_slope)
    B, Cin, T = x.shape
    K, form = L["K"], L["form"]
    Cout = w.shape[1] if form == "T" else w.shape[0]
    b0 = torch.zeros(Cout, dtype=x.dtype) if bias is None else bias
    if form == "T":
        s, p = L["stride"], L["padding"]
        acc = b0[None, :, None].expand(B, Cout, (T - 1) * s + K).contiguous()
        for k in range(K):
            view = acc[:, :, k:k + (T - 1) * s + 1:s]
            for ci in range(Cin):
                view.addcmul_(x[:, ci:ci + 1, :], w[ci, :, k][None, :, None])
        return acc[:, :, p:p + T * s].contiguous()
    To = T if form == "same" else T // 2
    H = (K - 1) * L["d"] // 2 if form == "same" else 1
    xp = torch.zeros(B, Cin, T + 2 * H, dtype=x.dtype)
    xp[:, :, H:H + T] = x
    acc = b0[None, :, None].expand(B, Cout, To).contiguous()
    for k in range(K):
        xs = (xp[:, :, k * L["d"]:k * L["d"] + T] if form == "same" else xp[:, :, k:k + T:2]).contiguous()
        for ci in range(Cin):
            acc.addcmul_(xs[:, ci:ci + 1, :], w[:, ci, k][None, :, None])
    return acc


def epilogue(v, c, E, dtype, mut=None, mag=False, biased=False):
    """v (B, Cout, Tout) the conv sum (or, mag, its magnitude; biased: the bias is in it already); c the case's tensors; returns (y, y2 or None)"""
    t = lambda k: c[k].to(dtype)   # noqa: E731
    act = E.get("act", "none")
    if E.get("bias", True) and not biased:
        b = t("bias")
        if mut == "biasshift":
            c0 = (b.numel() // 64) * 64
            b = torch.cat([b[:c0], b[c0 + 1:], b[-1:]])
        v = v + (b.abs() if mag else b)[None, :, None]
    a, bi = t("alpha_exp"), t("beta_inv")
    if mut == "snake_swap":
        a, bi = bi, a
    if mag:
        v = v * ((1.0 + a * bi)[None, :, None] if act == "snake" else ACT_LIP[act])
    elif act == "lrelu":
        v = lrelu(v, E["act_slope"])
    elif act == "tanh":
        v = torch.tanh(v)
    elif act == "silu":
        v = v * torch.sigmoid(v)
    elif act == "mish":
        v = mish(v)
    elif act == "snake":
        v = v + bi[None, :, None] * torch.sin(v * a[None, :, None]) ** 2
    m = c["mask"].to(dtype)
    scale = float(torch.tensor(E.get("scale", 1.0), dtype=torch.float32))     # the fp32 value the kernel multiplies by
    if mag:
        scale = abs(scale)
    late_mask = mut == "mask_late" and E.get("mask1")
    if E.get("mask1") and not mag and not late_mask:
        v = v * m
    if mut != "scale_late":
        v = v * scale
    if E.get("R"):
        v = v + (t("R").abs() if mag else t("R"))
    if mut == "scale_late":
        v = v * scale
    if late_mask:
        v = v * m
    if mut == "div3_early":
        v = v / 3 + t("yold")
    else:
        if E.get("accum"):
            v = v + (t("yold").abs() if mag else t("yold"))
        if E.get("div3"):
            v = v / 3
    if "act2" in E and not mag:
        v = lrelu(v, 0.1 if mut == "act2_slope" else E["act2"])
    if E.get("mask2") and not mag:
        v = v * m
    return v, (v * m if E.get("y2") and not mag else None)


def truncate_bf16(x, pieces):
    """x (fp32) as the sum of its first `pieces` bf16 truncation pieces"""
    out, r = torch.zeros_like(x), x.clone()
    for _ in range(pieces):
        p = (r.view(torch.int32) & -65536).view(torch.float32)
        out, r = out + p, r - p
    return out


_SUMS = {}    # conv sums per (layer, class, prologue slope, dtype, mag): the epilogues of a layer share them


def evaluate(c, dtype, mut=None, mag=False, chain=False):
    """The case in `dtype` (fp64: the reference), a mutant of it, its magnitude A (mag; y2 is None), or (chain, fp32: the yardstick) the
    same sums taken as one accumulator chain from the bias on (conv_chain)."""
    L, E = LAYERS[c["layer"]], EPIS[c["epi"]]
    x = c["x"]
    if chain:
        key = (c["layer"], c["cls"], E.get("pro", -1.0), dtype, "chain", E.get("bias", True))
        if key not in _SUMS:
            _SUMS[key] = conv_chain(L, x.to(dtype), c["w"].to(dtype), c["bias"].to(dtype) if E.get("bias", True) else None, E.get("pro", -1.0))
        return epilogue(_SUMS[key], c, E, dtype, biased=True)
    if mut == "x_fp16":
        x = x.half().float()
    elif mut == "x_bf16x2":
        x = truncate_bf16(x, 2)
    pro = E.get("pro", -1.0)
    key = (c["layer"], c["cls"], pro, dtype, mag)
    plain = mut not in ("x_fp16", "x_bf16x2", "tapdrop", "padleak", "prohalo")
    if plain and key in _SUMS:
        v = _SUMS[key]
    else:
        x, w = x.to(dtype), c["w"].to(dtype)
        if mag:
            x, w, pro = (lrelu(x, pro) if pro >= 0 else x).abs(), w.abs(), -1.0
        v = conv(L, x, w, pro, mut if mut in ("tapdrop", "padleak", "prohalo") else None)
        if plain:
            _SUMS[key] = v
    return epilogue(v, c, E, dtype, mut, mag)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def frame_scales(cls, B, T):
    """(B, T) the scale of every input frame of a class (0: the zero class)"""
    s = torch.ones(B, T)
    if cls == "mixed":
        s[:, ::7] = 1e-3
    elif cls == "rows":
        s *= torch.tensor([10.0 ** (3 * (-1, 0, 1, 0)[b % 4]) for b in range(B)])[:, None]       # (neighbours differ by 1e3 at any B)
    elif cls == "zero":
        s *= 0
    elif cls == "tiny":
        s *= 1e-6
    elif cls == "huge":
        s *= 1e4
    return s


def fill(cls, B, Cin, T, g):
    x = torch.randn(B, Cin, T, generator=g)
    if cls == "offset":
        x = x + 50.0
    if cls == "channels":
        x = x * (10.0 ** torch.linspace(-1.5, 1.5, Cin))[None, :, None]
    return x * frame_scales(cls, B, T)[:, None, :]


def window_range(cls, L):
    """Largest ratio of two non-zero frame scales within any window of WINDOW + halo rows of the flattened axis (the channel spread of
    `channels` included).  A layer whose utterances are shorter than the window does not carry the `rows` class."""
    B, T, P = L["B"], L["T"], L["P"]
    s = frame_scales(cls, B, T)
    flat = torch.zeros(B, T + 2 * P)
    flat[:, P:P + T] = s
    flat = flat.reshape(-1)
    W = WINDOW + 2 * halo_rows(L)
    worst = 1.0
    for n0 in range(0, max(1, flat.numel() - W + 1)):
        v = flat[n0:n0 + W]
        v = v[v > 0]
        if v.numel():
            worst = max(worst, float(v.max() / v.min()))
    return worst * (10.0 ** 3 if cls == "channels" else 1.0)


def lengths_for(B, Tout):
    """ragged: Tout, 1 and others"""
    v = [1 + (7 + 37 * b) % Tout for b in range(B)]
    v[0] = Tout
    if B > 1:
        v[1] = 1 if Tout > 1 else Tout
    return torch.tensor(v, dtype=torch.int32)


_CASES = {}


def case(layer, cls="randn", epi="plain"):
    """One case, fp32 tensors; cached and never modified: x (B, Cin, T), w, bias, R, yold (B, Cout, Tout), lengths, mask, SnakeBeta's vectors."""
    key = (layer, cls, epi)
    if key in _CASES:
        return _CASES[key]
    L = LAYERS[layer]
    g = torch.Generator().manual_seed(1 + sorted(LAYERS).index(layer) * 100 + CLASSES.index(cls))
    B, Cin, Cout, K, T = L["B"], L["Cin"], L["Cout"], L["K"], L["T"]
    To = out_frames(L)
    x = fill(cls, B, Cin, T, g)
    fan = Cin * (K if L["form"] != "T" else K / L["stride"])
    w = torch.randn((Cin, Cout, K) if L["form"] == "T" else (Cout, Cin, K), generator=g) / fan ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1 + 0.05
    ysc = float(frame_scales(cls, B, T).max()) or 1.0          # residuals at the scale of the conv's output
    R = torch.randn(B, Cout, To, generator=g) * ysc
    yold = torch.randn(B, Cout, To, generator=g) * ysc
    al, be = torch.randn(Cout, generator=g) * 0.3, torch.randn(Cout, generator=g) * 0.3
    lengths = lengths_for(B, To)
    mask = (torch.arange(To)[None, :] < lengths.long()[:, None]).float()[:, None, :]
    c = {"layer": layer, "cls": cls, "epi": epi, "x": x, "w": w, "bias": bias, "R": R, "yold": yold, "lengths": lengths, "mask": mask,
         "alpha_exp": torch.exp(al), "beta_inv": 1.0 / (torch.exp(be) + 0.000000001)}
    _CASES[key] = c
    return c


_REFS = {}


def references(c):
    """(fp64 y, fp64 y2, fp32 y, fp32 y2, A): computed once per case on the CPU and left unchanged"""
    key = (c["layer"], c["cls"], c["epi"])
    if key not in _REFS:
        y64, z64 = evaluate(c, torch.float64)
        y32, z32 = evaluate(c, torch.float32, chain=True)
        A, _ = evaluate(c, torch.float64, mag=True)
        _REFS[key] = (y64, z64, y32, z32, A)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------------
def frame_errors(y, ref, A):
    """(5, B, T) per frame over channels: L-inf error, RMS error, rms A, max A, max |ref|"""
    e = y.double() - ref
    return torch.stack([e.abs().amax(dim=1), e.pow(2).mean(dim=1).sqrt(), A.pow(2).mean(dim=1).sqrt(), A.amax(dim=1), ref.abs().amax(dim=1)])


def gates(err32, cp):
    """(2, B, T): the L-inf and RMS gate of every frame from the fp32 evaluation's errors; cp = c_pipe of the build"""
    basis = err32[2]
    rel = torch.where(basis > 0, err32[:2] / basis.clamp(min=1e-300), torch.zeros_like(err32[:2]))
    yard = rel.reshape(2, -1).amax(dim=1)
    return torch.stack([torch.maximum(MARGIN * yard[i] * basis, FLOOR * err32[4]) + cp * (err32[3] if i == 0 else basis) for i in range(2)])


def gate_failures(y, ref, y32, A, build, tag="", around=None):
    """Frames of y over the gate of `build`.  Returns (failures, worst error / gate over the frames: a report, 1 is the gate).
    around: a mutant reference to measure y against instead, inside the gate that `ref` defines."""
    err, err32 = frame_errors(y, ref if around is None else around, A), frame_errors(y32, ref, A)
    gate = gates(err32, c_pipe(build))
    bad = []
    if not bool(torch.isfinite(y).all()):
        bad.append((tag, "non-finite output"))
    worst = 0.0
    for i, kind in enumerate(("linf", "rms")):
        e, gt = err[i], gate[i]
        over = ~(e <= gt)
        ratio = torch.where(e > 0, e / gt.clamp(min=1e-300), torch.zeros_like(e)).nan_to_num(nan=float("inf"))
        worst = max(worst, float(ratio.max()))
        if bool(over.any()):
            j = int(ratio.argmax())
            b, t = divmod(j, e.shape[1])
            bad.append((tag, kind, f"{int(over.sum())} of {e.numel()} frames over the gate; worst at (b {b}, t {t}): error {float(e[b, t]):.3e} "
                                   f"gate {float(gt[b, t]):.3e}"))
    return bad, worst


def masked_failures(y, y2, c, tag=""):
    """Masked frames exact: 0 where the mask comes last or nothing follows mask1, R (+ Yold, in fp32) where mask1 is followed by +R;
    Y2 = y * m bit for bit."""
    E = EPIS[c["epi"]]
    bad = []
    m = c["mask"]
    dead = (m == 0).expand_as(y)
    if E.get("mask2"):
        want = torch.zeros_like(y)
    elif E.get("mask1"):
        want = torch.zeros_like(y)
        if E.get("R"):
            want = want + c["R"]
        if E.get("accum"):
            want = want + c["yold"]
        if E.get("div3"):
            want = want / 3
        if "act2" in E:
            want = lrelu(want, E["act2"])
    else:
        want = None
    if want is not None and bool(dead.any()) and not torch.equal(y[dead], want[dead]):
        bad.append((tag, f"masked frames are not exact: {int((y[dead] != want[dead]).sum())} elements differ"))
    if y2 is not None and not torch.equal(y2, y * m):
        bad.append((tag, "Y2 is not y * rowmask bit for bit"))
    return bad


def failures(y, y2, c, build, tag=""):
    """Everything an output of case c on `build` is held to."""
    y64, z64, y32, z32, A = references(c)
    bad, worst = gate_failures(y, y64, y32, A, build, tag)
    if z64 is not None:
        if y2 is None:
            bad.append((tag, "no Y2"))
        else:
            b2, w2 = gate_failures(y2, z64, z32, A, build, tag + " Y2")
            bad, worst = bad + b2, max(worst, w2)
    return bad + masked_failures(y, y2, c, tag), worst


# mutant -> (layer, epilogue) of the case that shows it, and the builds whose gate it is held against
MUTANTS = {
    "tapdrop": ("k3", "plain"), "padleak": ("k3", "plain"), "prohalo": ("k3", "pro_R"), "biasshift": ("c224", "plain"),
    "scale_late": ("c224", "euler"), "mask_late": ("k3", "m1_R"), "div3_early": ("k3", "mrf2"), "act2_slope": ("k3", "mrf2"),
    "snake_swap": ("k3", "snake"), "x_fp16": ("k3", "plain"), "x_bf16x2": ("k1", "plain"),
}
# (default: 0, 46 and 40.  x_bf16x2 is held to the fp32-pipe gate of build 0, which runs the k1 layer too: measured on the host it exceeds that
# gate 13 x, the fp16 gate 5.2 x and the bf16 gate 4.5 x on k1, and 10 / 2.9 / 2.4 x on k3 — the worst-case allowance discussed above)
MUTANT_BUILDS = {"x_fp16": (0, 46, 40), "x_bf16x2": (0,), "biasshift": (1,), "scale_late": (1,)}


# ---------------------------------------------------------------------------------------------------------------------
# what tests/test_gpu_conv.py runs: per build the layers (the first carries every epilogue and every class, the others `plain` on randn and
# mixed and the whole running sum `mrf2`).  A forced code stands only on layers that meet pick_cfg's own condition for its tile:
# Cout % 128 == 0 (0 / 40 / 46), Cout > 32 (1 / 5 / 6 / 8), Cout <= 32 (2), a small launch with a K loop of >= 8 (chunk, tap) steps or the
# dense 128 -> 128 layer (9 / 19), split_ok (Cin % 64 == 0 = Kpad, lean epilogue) on the 16-bit pipes, the transposed layers with a packed
# Cout % 64 == 0 for 41 / 47.
# ---------------------------------------------------------------------------------------------------------------------
BUILD_LAYERS = {
    0: ("k3", "k7d3", "k1", "s2", "k7_t1", "k7_t5"),
    1: ("k3", "k7d3", "k11d5", "c224", "c80", "s2", "t2", "t8", "k7_t1", "k7_t5"),
    2: ("c32", "post"),
    5: ("k3", "k11d5", "c224", "t8"),
    6: ("k3", "k7d3", "c80", "t2"),
    8: ("k3", "c224", "s2"),
    9: ("k7d3", "k3", "k11d5", "c224"),
    19: ("k3", "k7d3", "k11d5", "c224", "k7_t1", "k7_t5"),
    40: ("k3", "k7d3", "k1", "k11d5"),
    46: ("k3", "k7d3", "k1", "k11d5", "k7_t1", "k7_t5"),
    41: ("t2", "t8"),
    47: ("t2", "t8"),
    56: ("bal56",),
    60: ("bal3", "bal7"),
    66: ("bal3", "bal7"),
}
FORCED_BUILDS = (0, 1, 2, 5, 6, 8, 9, 19, 40, 41, 46, 47)
BALANCED_BUILDS = (56, 60, 66)
SIDE_EPIS = ("plain", "mrf2")
BAL_EPIS = ("plain", "nobias", "pro_R", "relu_m1", "m1_R", "R_m2", "mrf1", "mrf2", "sum3")      # lean 1 / 3, no SnakeBeta: what bal_ok admits


def epis_for(build, layer):
    """The epilogues of the main layer of a build: every combination whose flavour the build's kernel has (and, on a transposed layer,
    that needs no row mask: the hook has no column-split views)."""
    if build in BALANCED_BUILDS:
        names = BAL_EPIS
    elif build in FP32_BUILDS:
        names = tuple(EPIS)
    else:
        names = LEAN_EPIS + ("mrf0",)
    if LAYERS[layer]["form"] == "T":
        names = tuple(n for n in names if not (EPIS[n].get("mask1") or EPIS[n].get("mask2") or EPIS[n].get("y2")))
    return names


def plan(build):
    """[(layer, class, epilogue)] of a build"""
    layers = BUILD_LAYERS[build]
    out = [(layers[0], "randn", e) for e in epis_for(build, layers[0])]
    out += [(layers[0], cls, "plain") for cls in CLASSES[1:]]
    for name in layers[1:]:
        out += [(name, "randn", e) for e in SIDE_EPIS] + [(name, "mixed", "plain")]
    if build in (1, 5, 8, 9, 19):
        out.append(("c224", "randn", "euler"))            # the Euler step at Cout = 80
    if build == 19:
        out.append(("c224", "randn", "snake"))            # SnakeBeta on the general small-launch build (K padding keeps c224 off conv_sk32_kernel)
    return out


def mutant_ratio(name, build):
    """Worst (error of the mutant reference / gate of `build`) over the frames and the two kinds"""
    layer, epi = MUTANTS[name]
    c = case(layer, "randn", epi)
    y64, z64, y32, z32, A = references(c)
    ym, _ = evaluate(c, torch.float64, mut=name)
    err, err32 = frame_errors(ym, y64, A), frame_errors(y32, y64, A)
    gate = gates(err32, c_pipe(build))
    return float((err[:2] / gate.clamp(min=1e-300)).max())
