"""fp64 restatements of the U-Net's normalisation kernels, the inputs that stress them and the gates that hold the kernels to them.

Restatements (plain torch, no engine code; they run in the dtype of their inputs, so the same function is the fp64 reference and, on
fp32 inputs on the CPU, the plain fp32 evaluation every gate is derived from):

  groupnorm_mish   GroupNorm(8 groups of 32 channels over ALL T frames of an utterance, padded frames included) + Mish + mask, with the
                   three epilogues documented above GNParams in ev_kernels.h:
                     mode 0   mish(gn(x)) * m
                     mode 1   (mish(gn(x)) * m + temb[b or 0][c]) * m        (the mask twice: a padded frame is 0, not temb)
                     mode 2   mish(gn(x)) * m + R                           (R is not masked: a padded frame is R)
  layernorm        LayerNorm over the 256 channels of a row, biased variance, eps 1e-5
  chan_merge       Chan et al.'s update over per-tile {count, mean, M2} triples in ascending tile order, in fp64 from the fp32 triples
  tile_stats       the triples conv_sk32_kernel leaves: per (32-row tile of the padded utterance, group) over the tile's valid frames

Input classes.  A GroupNorm class fills one (utterance, group) slab, a LayerNorm class one row:
  randn | offset (mean 50, spread 0.05) | const (100) | zero | outlier (one 1e4 among unit-variance values) | tiny (1e-6) | huge (1e6) |
  cross (GroupNorm only: group 7's gamma is 10, so gamma * normalised + beta spans about -30 .. 30 — both sides of ev_mish's x > 20 branch
  and its negative tail.  LayerNorm has no activation behind it and one gamma for all rows: its cases carry the other seven.)
beta is randn * 0.1 + 0.3: every slab / row has an output RMS >= 1e-2 (RMS_FLOOR), asserted in tests/test_norm_reference.py.

Gates.  Per slab over its valid frames (GroupNorm) or per row (LayerNorm), for the RMS and the L-inf of (got - fp64):
    error <= max(MARGIN x worst error of the plain fp32 evaluation over the slabs / rows of the same class in the same case, relative to
                 the fp64 output RMS, times this slab's RMS;   2^-21 x this slab's fp64 L-inf)
MARGIN = 4 covers what separates the kernel's fp32 two-pass sums (per-thread partial sums, wave-shuffle trees) from torch's vectorised
fp32 two-pass sums; the floor is there because the fp32 evaluation can be exact on constant and zero slabs.  Masked frames are part of
the gate: exactly 0 in modes 0 and 1, exactly R in mode 2.  Nothing here is derived from a kernel's output."""
import torch

C = 256
GROUPS = 8
CG = C // GROUPS
EPS = 1e-5
MARGIN = 4.0
FLOOR = 2.0 ** -21
RMS_FLOOR = 1e-2
GN_P = 2                 # pad rows in front of an utterance in the estimator's level-0 geometry (rows per utterance: T + 4)
TILE = 32

GN_CLASSES = ("randn", "offset", "const", "zero", "outlier", "tiny", "huge", "cross")
LN_CLASSES = GN_CLASSES[:7]
CROSS_GROUP = 7


# ---------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------
def mish(x):
    """x * tanh(softplus(x)); softplus with torch's threshold (x above 20: x)."""
    sp = torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))
    return x * torch.tanh(sp)


def frame_mask(lengths, T, dtype):
    return (torch.arange(T)[None, :] < lengths.long()[:, None]).to(dtype)[:, None, :]


def groupnorm(x, gamma, beta, eps=EPS):
    """(B, 256, T): statistics over all T frames of each (utterance, group) slab, two passes, biased variance."""
    B, Cc, T = x.shape
    xg = x.reshape(B, GROUPS, (Cc // GROUPS) * T)
    mean = xg.mean(dim=2, keepdim=True)
    d = xg - mean
    var = (d * d).mean(dim=2, keepdim=True)
    return (d / torch.sqrt(var + eps)).reshape(B, Cc, T) * gamma[None, :, None] + beta[None, :, None]


def groupnorm_mish(x, gamma, beta, lengths, mode=0, temb=None, R=None, eps=EPS):
    """x (B, 256, T), lengths (B,), temb (1, 256) or (B, 256) (mode 1), R (B, 256, T) (mode 2); computes in x.dtype."""
    m = frame_mask(lengths, x.shape[2], x.dtype)
    y = mish(groupnorm(x, gamma, beta, eps)) * m
    if mode == 1:
        y = (y + temb.reshape(-1, x.shape[1])[:, :, None]) * m
    elif mode == 2:
        y = y + R
    return y


def layernorm(x, gamma, beta, eps=EPS):
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    return d / torch.sqrt(var + eps) * gamma + beta


def chan_merge(part):
    """part (ntiles, ..., 3) {count, mean, M2} -> (count, mean, M2) of the union, merged in ascending tile order in fp64."""
    part = part.double()
    na = torch.zeros_like(part[0, ..., 0])
    mean, m2 = na.clone(), na.clone()
    for j in range(part.shape[0]):
        nb, mb, qb = part[j, ..., 0], part[j, ..., 1], part[j, ..., 2]
        nn = na + nb
        w = torch.where(nn > 0, nb / nn.clamp(min=1.0), torch.zeros_like(nn))
        d = mb - mean
        mean = mean + d * w
        m2 = m2 + qb + d * d * na * w
        na = nn
    return na, mean, m2


def tile_stats(y, P=GN_P):
    """y (256, T), one utterance -> (ntiles, 8, 3) {count, mean, M2} per (32-row tile of the P + T + P padded rows, group) over the
    tile's frames inside [0, T), two passes in y.dtype."""
    T = y.shape[1]
    nt = (T + 2 * P + TILE - 1) // TILE
    out = torch.zeros(nt, GROUPS, 3, dtype=y.dtype)
    for j in range(nt):
        lo, hi = max(j * TILE - P, 0), min(j * TILE + TILE - P, T)
        if hi <= lo:
            continue
        v = y[:, lo:hi].reshape(GROUPS, -1)
        mean = v.mean(dim=1)
        out[j, :, 0] = v.shape[1]
        out[j, :, 1] = mean
        out[j, :, 2] = ((v - mean[:, None]) ** 2).sum(dim=1)
    return out


def tile_scales(y, P=GN_P):
    """(ntiles, 8, 2): per tile of tile_stats the {rms, linf} of its values (what an error of its mean is measured against)"""
    T = y.shape[1]
    nt = (T + 2 * P + TILE - 1) // TILE
    out = torch.zeros(nt, GROUPS, 2, dtype=y.dtype)
    for j in range(nt):
        lo, hi = max(j * TILE - P, 0), min(j * TILE + TILE - P, T)
        if hi > lo:
            v = y[:, lo:hi].reshape(GROUPS, -1)
            out[j, :, 0], out[j, :, 1] = v.pow(2).mean(dim=1).sqrt(), v.abs().amax(dim=1)
    return out


def snake_ff(x, ln_g, ln_b, w1, b1, a_exp, b_inv, w2, b2, mask):
    """x + W2 . SnakeBeta(W1 . LN(x) + b1) + b2, * mask — the feed-forward half of a transformer block (ln_mlp_kernel mode 0)."""
    h = layernorm(x, ln_g, ln_b) @ w1.T + b1
    h = h + b_inv * torch.sin(h * a_exp) ** 2
    return (x + h @ w2.T + b2) * mask[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def fill(cls, shape, g):
    """fp32 values of one input class."""
    r = torch.randn(shape, generator=g)
    if cls == "randn" or cls == "cross":
        return r
    if cls == "offset":
        return 50.0 + 0.05 * r
    if cls == "const":
        return torch.full(shape, 100.0)
    if cls == "zero":
        return torch.zeros(shape)
    if cls == "outlier":
        flat = r.reshape(-1)
        flat[int(torch.randint(0, flat.numel(), (1,), generator=g))] = 1.0e4
        return flat.reshape(shape)
    if cls == "tiny":
        return 1.0e-6 * r
    if cls == "huge":
        return 1.0e6 * r
    raise ValueError(cls)


def gn_affine(g):
    """gamma around 1 (group 7: around 10, the crossing group), beta = randn * 0.1 + 0.3."""
    gamma = torch.randn(C, generator=g) * 0.1 + 1.0
    gamma[CROSS_GROUP * CG:] = 10.0 + torch.randn(CG, generator=g)
    beta = torch.randn(C, generator=g) * 0.1 + 0.3
    return gamma, beta


def gn_lengths(B, T):
    """ragged, with T and 1 among them"""
    L = [1 + (7 + 37 * b) % T for b in range(B)]
    L[0] = T
    if B > 1:
        L[1] = 1
    return torch.tensor(L, dtype=torch.int32)


def gn_case(B, T, seed=None):
    """One GroupNorm case: slab (b, g) of groups 0..6 carries class (b + g) % 7, group 7 the crossing class.  All tensors fp32."""
    g = torch.Generator().manual_seed(1000 * B + T if seed is None else seed)
    cls = torch.zeros(B, GROUPS, dtype=torch.long)
    x = torch.empty(B, C, T)
    for b in range(B):
        for gr in range(GROUPS):
            k = GN_CLASSES.index("cross") if gr == CROSS_GROUP else (b + gr) % 7
            cls[b, gr] = k
            x[b, gr * CG:(gr + 1) * CG] = fill(GN_CLASSES[k], (CG, T), g)
    gamma, beta = gn_affine(g)
    return {"x": x, "gamma": gamma, "beta": beta, "lengths": gn_lengths(B, T), "cls": cls,
            "temb_shared": torch.randn(1, C, generator=g) * 0.5, "temb_rows": torch.randn(B, C, generator=g) * 0.5,
            "R": torch.randn(B, C, T, generator=g)}


GN_VARIANTS = ("m0", "m1s", "m1r", "m2")        # mode 0 | mode 1, shared temb | mode 1, one temb row per utterance | mode 2


def gn_args(case, variant):
    """(mode, temb, R) of a variant"""
    return {"m0": (0, None, None), "m1s": (1, case["temb_shared"], None), "m1r": (1, case["temb_rows"], None), "m2": (2, None, case["R"])}[variant]


def gn_eval(case, variant, dtype):
    mode, temb, R = gn_args(case, variant)
    cv = lambda t: None if t is None else t.to(dtype)   # noqa: E731
    return groupnorm_mish(case["x"].to(dtype), case["gamma"].to(dtype), case["beta"].to(dtype), case["lengths"], mode, cv(temb), cv(R))


# the shapes tests/test_gpu_norms.py runs: the pass width (rows per pass: 128 / 64) and the register / three-pass boundary (1024 / 768) of
# groupnorm_mish_kernel<1024> (B < 32) and <512> (B >= 32)
GN_SHAPES = [(3, T) for T in (1, 127, 128, 129, 1024, 1025)] + [(32, T) for T in (1, 63, 64, 65, 768, 769, 1030)]
APPLY_T = (4, 31, 33, 516, 2052, 2100)


def apply_case(T):
    """One utterance for the conv -> GroupNorm chain: x (1, 256, T) carries one class per 32-row tile of the padded utterance, plus a
    tile-local offset, so the tiles' means differ widely (the d * d * na * w term of the merge); w (256, 256, 3), bias, affine, temb, R."""
    g = torch.Generator().manual_seed(77000 + T)
    x = torch.empty(1, C, T)
    nt = (T + 2 * GN_P + TILE - 1) // TILE
    for j in range(nt):
        lo, hi = max(j * TILE - GN_P, 0), min(j * TILE + TILE - GN_P, T)
        if hi <= lo:
            continue
        cls = GN_CLASSES[j % 8]
        v = fill(cls, (C, hi - lo), g)
        if cls not in ("const", "zero"):
            v = v + (3.0 * ((5 * j) % 7 - 3)) * (1.0e6 if cls == "huge" else 1.0)
        x[0, :, lo:hi] = v
    w = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    bias = torch.randn(C, generator=g) * 0.1
    gamma, beta = gn_affine(g)
    return {"x": x, "w": w, "bias": bias, "gamma": gamma, "beta": beta, "lengths": torch.tensor([max(1, T - 3)], dtype=torch.int32),
            "temb_shared": torch.randn(1, C, generator=g) * 0.5, "R": torch.randn(1, C, T, generator=g),
            "cls": torch.zeros(1, GROUPS, dtype=torch.long)}


def ln_case(rows, seed=None):
    """(rows, 256) fp32: row i carries class i % 7, so every 32-row tile holds all of them at shifting positions."""
    g = torch.Generator().manual_seed(31 * rows + 5 if seed is None else seed)
    cls = torch.arange(rows) % len(LN_CLASSES)
    x = torch.empty(rows, C)
    for k, name in enumerate(LN_CLASSES):
        idx = (cls == k).nonzero().flatten()
        if name == "outlier":
            v = torch.randn(len(idx), C, generator=g)
            v[torch.arange(len(idx)), torch.randint(0, C, (len(idx),), generator=g)] = 1.0e4
        else:
            v = fill(name, (len(idx), C), g)
        x[idx] = v
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1 + 0.3
    return {"x": x, "gamma": gamma, "beta": beta, "cls": cls}


def mlp_weights(M1, seed):
    """Weights of the fused LayerNorm + linear kernels: w1 (M1, 256), b1, SnakeBeta's exp(alpha) and 1 / (exp(beta) + 1e-9) as the engine
    receives them (fp32), w2 (256, M1), b2."""
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(M1, C, generator=g) / 16.0
    b1 = torch.randn(M1, generator=g) * 0.1
    alpha, beta = torch.randn(M1, generator=g) * 0.3, torch.randn(M1, generator=g) * 0.3
    w2 = torch.randn(C, M1, generator=g) / M1 ** 0.5
    b2 = torch.randn(C, generator=g) * 0.1
    return {"w1": w1, "b1": b1, "alpha": alpha, "beta": beta, "a_exp": torch.exp(alpha), "b_inv": 1.0 / (torch.exp(beta) + 0.000000001),
            "w2": w2, "b2": b2}


def ln_rowmask(rows):
    """every 11th row masked"""
    return (torch.arange(rows) % 11 != 10).float()


def ln_eval(case, what, wts, dtype):
    """what: 'ln' | 'proj' (W1 . LN(x), no bias) | 'ff' (snake_ff, rows of ln_rowmask)"""
    x, ga, be = case["x"].to(dtype), case["gamma"].to(dtype), case["beta"].to(dtype)
    if what == "ln":
        return layernorm(x, ga, be)
    if what == "proj":
        return layernorm(x, ga, be) @ wts["w1"].to(dtype).T
    c = lambda k: wts[k].to(dtype)   # noqa: E731
    return snake_ff(x, ga, be, c("w1"), c("b1"), c("a_exp"), c("b_inv"), c("w2"), c("b2"), ln_rowmask(x.shape[0]).to(dtype))


LN_ROWS = (101, 16640)
MLP_ROWS = (70, 9000, 16640)


# ---------------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------------
def gn_slab_errors(y, ref, lengths):
    """Per (utterance, group) slab over its valid frames: (rms error, linf error, fp64 rms, fp64 linf), each (B, 8), in fp64."""
    B = ref.shape[0]
    out = torch.zeros(4, B, GROUPS, dtype=torch.float64)
    y = y.double()
    for b in range(B):
        L = int(lengths[b])
        r = ref[b, :, :L].reshape(GROUPS, -1)
        e = y[b, :, :L].reshape(GROUPS, -1) - r
        out[0, b], out[1, b] = e.pow(2).mean(dim=1).sqrt(), e.abs().amax(dim=1)
        out[2, b], out[3, b] = r.pow(2).mean(dim=1).sqrt(), r.abs().amax(dim=1)
    return out


def row_errors(y, ref):
    """Per row: (rms error, linf error, fp64 rms, fp64 linf), each (rows,)"""
    e = y.double() - ref
    return torch.stack([e.pow(2).mean(dim=1).sqrt(), e.abs().amax(dim=1), ref.pow(2).mean(dim=1).sqrt(), ref.abs().amax(dim=1)])


def class_worst(err, cls, ncls, keep=None):
    """(2, ncls): per class the worst relative (rms, linf) error — the yardstick of a case"""
    rel = err[:2] / err[2]
    out = torch.zeros(2, ncls, dtype=torch.float64)
    for k in range(ncls):
        sel = (cls == k) if keep is None else ((cls == k) & keep)
        if bool(sel.any()):
            out[:, k] = rel[:, sel].amax(dim=1)
    return out


def gate_failures(err, err32, cls, names, keep=None, tag=""):
    """Slabs / rows whose error exceeds max(MARGIN x class-worst fp32 error x rms, FLOOR x linf).  Returns (failures, {class: worst kernel
    error / gate-defining fp32 error}) — the ratio is a report, the gate is what is asserted."""
    yard = class_worst(err32, cls, len(names), keep)
    bad, ratios = [], {}
    if not bool(torch.isfinite(err[:2]).all()):
        bad.append((tag, "non-finite error"))
    for k, name in enumerate(names):
        sel = (cls == k) if keep is None else ((cls == k) & keep)
        if not bool(sel.any()):
            continue
        for i, kind in enumerate(("rms", "linf")):
            gate = torch.maximum(MARGIN * yard[i, k] * err[2][sel], FLOOR * err[3][sel])
            e = err[i][sel]
            over = ~(e <= gate)
            if bool(over.any()):
                j = int((e / gate).nan_to_num(nan=float("inf")).argmax())
                bad.append((tag, name, kind, f"{int(over.sum())} of {int(sel.sum())} over the gate; worst error {float(e[j]):.3e} gate {float(gate[j]):.3e} "
                                             f"fp32 yardstick (relative) {float(yard[i, k]):.3e}"))
            ratios[(name, kind)] = float((e / (torch.maximum(yard[i, k] * err[2][sel], FLOOR * err[3][sel] / MARGIN))).nan_to_num(nan=float("inf")).max())
    return bad, ratios


def gn_masked_failures(y, lengths, R=None, tag=""):
    """Masked frames: exactly 0 (modes 0 and 1), exactly R (mode 2)."""
    bad = []
    for b in range(y.shape[0]):
        L = int(lengths[b])
        want = torch.zeros_like(y[b, :, L:]) if R is None else R[b, :, L:].to(y.dtype)
        if not torch.equal(y[b, :, L:], want):
            bad.append((tag, f"utterance {b}: masked frames are not exactly {'0' if R is None else 'R'}"))
    return bad


def gn_failures(y, case, variant, ref64=None, y32=None, tag=""):
    """Everything a GroupNorm output is held to: every slab gated, masked frames exact.  y fp32 (a kernel's, or a mutant's)."""
    ref64 = gn_eval(case, variant, torch.float64) if ref64 is None else ref64
    y32 = gn_eval(case, variant, torch.float32) if y32 is None else y32
    L = case["lengths"]
    bad, ratios = gate_failures(gn_slab_errors(y, ref64, L), gn_slab_errors(y32, ref64, L), case["cls"], GN_CLASSES, tag=tag)
    bad += gn_masked_failures(y, L, case["R"] if variant == "m2" else None, tag)
    return bad, ratios
