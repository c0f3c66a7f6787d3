"""fp64 statement of the stage in front of the decoder: TextEncoder + DurationPredictor, the duration rounding and the hard monotonic
alignment (a plain module: the CPU and GPU text-encoder tests import it).

``encode`` restates ``TextEncoder.forward`` (text_encoder.py:378-410: embedding x sqrt(C), ConvReluNorm prenet :36-67, speaker concat,
Encoder :276-325 with RoPE MultiHeadAttention :97-246, channel LayerNorm at eps 1e-4 :15-33 and the k = 3 FFN :255-273, ``proj_m``,
DurationPredictor :70-94) at any precision and on any device.  ``token_frames`` / ``mel_lengths`` restate the duration rounding of
``MatchaTTS.synthesise`` (matcha_tts.py:121-125), ``path`` / ``expand`` restate ``generate_path`` (utils/model.py:29-41) and
``mu_y = attn^T mu_x`` (matcha_tts.py:131-135).

It is written independently of oracle/matcha_oracle.py, so that the pin of tests/test_text_encoder_reference.py (equal to the oracle
to 1e-12 in fp64) compares two statements: activations are frame-major (B, T, C), a k-tap convolution is k shifted matmuls, the heads
are sliced and multiplied one by one, RoPE rotates explicit (j, j + d/2) pairs, the path is an interval test on a prefix sum.

Precision contract:
  * in fp32, as the reference defines it and as the engine evaluates it (enc_rope_kernel): ``theta``, the angle table
    ``arange(t).float() * theta`` and its cosine / sine.  They stay fp32 whatever ``dtype`` is.
  * in ``dtype`` (fp64 for the yardstick): everything else.
  * the reference's ``masked_fill(-1e4)`` is kept, not replaced by a skip: a masked key weighs exp(-1e4 - max), which is 0 in fp32
    and fp64 alike for a row with one valid key, and a row without any (length 0, or a padded query) gets uniform attention, whose
    result every consumer masks.
  * token ids beyond a row's length never reach a valid frame; ids outside the vocabulary are clamped THERE (the reference's
    nn.Embedding raises on them wherever they are; the engine reports them inside the length only, ev_text_encoder_status).

``SLIPS`` are plausible kernel mistakes, applied here to show that the GPU gates see them.  The case list, the input builders, the
measured float32 reference errors and the gates derived from them live here, so that the CPU and GPU tests read the same numbers.
"""
import math
from collections import OrderedDict

import torch

from emojivoice_amd import weights as W

N_HEADS, N_LAYERS = 2, 6
PEAK = 3.0            # conv_q / conv_k (weights and biases) scale of the peaked-attention checkpoint: scores grow 9x

# ---------------------------------------------------------------------------------------------------------------------
# Gates, one set per checkpoint.  REF_ERR: the float32 CPU oracle (oracle/matcha_oracle.py on the fp32 state dict) against ``encode`` in
# fp64, (RMS, max) over the valid tokens of one call, absolute, worst over every case of ``cases``; for the standard checkpoint also
# over ``single_speaker_case`` and the reference-generated golden g3 vectors.  Measured on the CPU by
# tests/test_text_encoder_reference.py (test_reference_error_is_what_the_gates_were_set_from re-measures it and holds these constants
# to it).  GATE = 3 x REF_ERR: room for another equally valid fp32 summation order and for the fp16-piece arithmetic, which claims fp32
# grade (the margin of test_gpu_mel.py).  The peaked checkpoint has gates of its own because its float32 reference amplifies rounding
# ~60-fold through the six layers (a gate pooled over both checkpoints would be 7.6e-4, looser than the old 1e-4).
# ---------------------------------------------------------------------------------------------------------------------
REF_ERR = {"std": {"mu": (8.1e-7, 4.1e-6), "logw": (1.32e-6, 3.3e-6)},
           "peak": {"mu": (1.9e-5, 2.5e-4), "logw": (2.6e-5, 1.9e-4)}}
MARGIN = 3.0
GATE = {w: {k: (MARGIN * v[0], MARGIN * v[1]) for k, v in d.items()} for w, d in REF_ERR.items()}
OLD_GATE = 1e-4                                         # the absolute gate of tests/test_gpu_parity.py: GATE stays > 5x under it
# Duration flips: a token is excluded where, in fp64, exp(logw) lies within GATE["std"]["logw"][1] * exp(logw) of an integer: there a logw
# inside the gate may round the other way.  Caps (conditions on the inputs, not measurements): excluded tokens per case list, and
# utterances that hold one.
CAP_TOKENS, CAP_UTTERANCES = 0.002, 0.10
LENGTH_SCALES = (1.0, 0.8, 1.37)

SLIPS = ("rope_pos", "rope_all", "ln_eps", "masked_key", "no_ffn_mask", "emb_scale", "h_fp16")
PROBE = None          # a list: every attention appends the largest softmax weight of each valid query (heads x valid queries)


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def peaked_attention_state(salt="ev0"):
    """synthetic_matcha_state with conv_q and conv_k (weights and biases) of the six encoder layers multiplied by PEAK: the scores grow
    PEAK^2-fold, the softmaxes peak (test_text_encoder_reference.py: the median largest weight exceeds 0.5 at Tx = 151), so the
    max-subtraction and the -inf tail of the last key tile carry weight and a peaked softmax no longer averages errors away."""
    sd = OrderedDict(W.synthetic_matcha_state(salt=salt))
    for k in sd:
        if ".attn_layers." in k and (".conv_q." in k or ".conv_k." in k):
            sd[k] = sd[k] * PEAK
    return sd


def states():
    return {"std": W.synthetic_matcha_state(), "peak": peaked_attention_state()}


def encoder_state(sd, dtype=torch.float64, device=None):
    """The ``encoder.*`` entries of a Matcha state dict, prefix stripped, in ``dtype`` on ``device``."""
    return {k[len("encoder."):]: v.to(device, dtype) for k, v in sd.items() if k.startswith("encoder.")}


# ---------------------------------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------------------------------
def _conv(x, w, b):
    """'same' Conv1d on frame-major x (B, T, Cin) with w (Cout, Cin, k): one matmul per tap over the zero-padded frames."""
    k, T = w.shape[2], x.shape[1]
    xp = torch.nn.functional.pad(x, (0, 0, k // 2, k // 2))
    y = b.view(1, 1, -1)
    for j in range(k):
        y = y + xp[:, j:j + T] @ w[:, :, j].t()
    return y


def _cln(x, g, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b


def rope_table(T, d, device=None, first=0):
    """(cos, sin), each (T, d / 2) in fp32: theta = 1 / 10000^(arange(0, d, 2) / d) and the angles arange(T) * theta of
    text_encoder.py:115-134, all float32."""
    theta = 1.0 / (10000.0 ** (torch.arange(0, d, 2).float() / d))
    ang = (torch.arange(first, first + T).float()[:, None] * theta[None, :]).to(device)
    return ang.cos(), ang.sin()


def _rope(x, d, first=0):
    """x (B, T, kc): rotate the pairs (j, j + d/2), j < d/2, of the first d features by the angle of the frame; the rest passes."""
    cos, sin = rope_table(x.shape[1], d, x.device, first)
    cos, sin = cos.to(x.dtype), sin.to(x.dtype)
    a, b, rest = x[..., :d // 2], x[..., d // 2:d], x[..., d:]
    return torch.cat((a * cos - b * sin, b * cos + a * sin, rest), dim=-1)


def _mha(sd, p, x, valid, slips):
    """MultiHeadAttention (text_encoder.py:175-246) on masked frame-major x; valid (B, T) bool."""
    q, k, v = (_conv(x, sd[f"{p}.conv_{n}.weight"], sd[f"{p}.conv_{n}.bias"]) for n in "qkv")
    kc = q.shape[-1] // N_HEADS
    d = kc if "rope_all" in slips else int(kc * 0.5)
    live = valid[:, :, None] & valid[:, None, :]                       # (B, Tq, Tk): attn_mask != 0
    if "masked_key" in slips:                                          # the first padded key of every row is let in
        lens = valid.sum(1)
        extra = torch.zeros_like(valid)
        rows = torch.nonzero(lens < valid.shape[1]).flatten()
        extra[rows, lens[rows]] = True
        live = live | (valid[:, :, None] & extra[:, None, :])
    outs = []
    for h in range(N_HEADS):
        sl = slice(h * kc, (h + 1) * kc)
        qh, kh = _rope(q[..., sl], d), _rope(k[..., sl], d, first=1 if "rope_pos" in slips else 0)   # (the slip: keys one position late)
        s = qh @ kh.transpose(1, 2) / math.sqrt(kc)
        s = torch.where(live, s, torch.full_like(s, -1e4))
        w = torch.softmax(s, dim=-1)
        if PROBE is not None:
            PROBE.append(w.amax(-1)[valid].detach().cpu())
        outs.append(w @ v[..., sl])
    return _conv(torch.cat(outs, dim=-1), sd[f"{p}.conv_o.weight"], sd[f"{p}.conv_o.bias"])


def encoder(sd, ids, lengths, spk, slips=()):
    """``sd``: encoder_state.  ids (B, Tx) long, lengths (B,), spk (B, E) in the state's dtype or None.  (mu (B, 80, Tx), logw (B, 1, Tx))."""
    emb = sd["emb.weight"]
    B, T = ids.shape
    valid = torch.arange(T, device=ids.device)[None, :] < lengths.to(ids.device)[:, None]
    m = valid.unsqueeze(-1).to(emb.dtype)
    ids = torch.where(valid, ids, ids.clamp(0, emb.shape[0] - 1))
    eps = 1e-5 if "ln_eps" in slips else 1e-4
    e = emb[ids] * (1.0 if "emb_scale" in slips else math.sqrt(emb.shape[1]))
    h = e
    for i in range(3):
        h = _conv(h * m, sd[f"prenet.conv_layers.{i}.weight"], sd[f"prenet.conv_layers.{i}.bias"])
        h = torch.relu(_cln(h, sd[f"prenet.norm_layers.{i}.gamma"], sd[f"prenet.norm_layers.{i}.beta"], eps))
    h = (e + _conv(h, sd["prenet.proj.weight"], sd["prenet.proj.bias"])) * m
    if spk is not None:
        h = torch.cat((h, spk[:, None, :].expand(B, T, spk.shape[-1])), dim=-1)
    for i in range(N_LAYERS):
        h = h * m
        h = _cln(h + _mha(sd, f"encoder.attn_layers.{i}", h, valid, slips), sd[f"encoder.norm_layers_1.{i}.gamma"], sd[f"encoder.norm_layers_1.{i}.beta"], eps)
        p = f"encoder.ffn_layers.{i}"
        y = torch.relu(_conv(h if "no_ffn_mask" in slips else h * m, sd[f"{p}.conv_1.weight"], sd[f"{p}.conv_1.bias"]))
        y = _conv(y * m, sd[f"{p}.conv_2.weight"], sd[f"{p}.conv_2.bias"]) * m
        h = _cln(h + y, sd[f"encoder.norm_layers_2.{i}.gamma"], sd[f"encoder.norm_layers_2.{i}.beta"], eps)
        if i == 2 and "h_fp16" in slips:
            h = h.half().to(h.dtype)
    h = h * m
    mu = _conv(h, sd["proj_m.weight"], sd["proj_m.bias"]) * m
    d = h
    for i in (1, 2):
        d = torch.relu(_conv(d * m, sd[f"proj_w.conv_{i}.weight"], sd[f"proj_w.conv_{i}.bias"]))
        d = _cln(d, sd[f"proj_w.norm_{i}.gamma"], sd[f"proj_w.norm_{i}.beta"], eps)
    logw = _conv(d * m, sd["proj_w.proj.weight"], sd["proj_w.proj.bias"]) * m
    return mu.transpose(1, 2), logw.transpose(1, 2)


def encode(sd, ids, lengths, spk, dtype=torch.float64, device=None, slips=(), esd=None):
    """(mu_x, logw) of ev_text_encoder for a Matcha state dict: ids (B, Tx), lengths (B,), spk (B, E) fp32 speaker rows or None."""
    esd = encoder_state(sd, dtype, device) if esd is None else esd
    spk = None if spk is None else spk.to(device, dtype)
    return encoder(esd, ids.to(device).long(), lengths.to(device).long(), spk, slips)


# ---------------------------------------------------------------------------------------------------------------------
# durations and alignment
# ---------------------------------------------------------------------------------------------------------------------
def token_frames(logw, lengths):
    """ceil(exp(logw)) per token, 0 beyond the lengths (matcha_tts.py:121-122 at length_scale 1): (B, Tx), in logw's dtype."""
    logw = logw.reshape(logw.shape[0], -1)
    valid = torch.arange(logw.shape[1], device=logw.device)[None, :] < lengths.to(logw.device)[:, None]
    return torch.ceil(torch.exp(logw)) * valid.to(logw.dtype)


def near_integer(logw64, lengths, rel):
    """(B, Tx) bool: valid tokens whose fp64 exp(logw) lies within ``rel * exp(logw)`` of an integer (the exclusion band)."""
    logw64 = logw64.reshape(logw64.shape[0], -1)
    valid = torch.arange(logw64.shape[1])[None, :] < lengths[:, None]
    w = torch.exp(logw64)
    return valid & ((w - torch.round(w)).abs() <= rel * w)


def mel_lengths(frames, length_scale):
    """y_lengths of matcha_tts.py:122-123 for integer token durations ``frames`` (B, Tx): the durations times the scale and their sum
    are float32, as the reference computes them on the CPU (55 x 0.8 sits next to 44: the fp32 sum decides the truncation), so this
    is the reference's own reduction, torch.sum of a (B, 1, Tx) float32 tensor over [1, 2] on the CPU.  Returns (w_ceil (B, Tx) fp32, y_lengths (B,) long)."""
    w_ceil = frames.to("cpu", torch.float32) * length_scale
    return w_ceil, torch.clamp_min(torch.sum(w_ceil.unsqueeze(1), [1, 2]), 1).long()


def padded_frames(y_max, factor=4):
    """fix_len_compatibility (utils/model.py:14-20)."""
    return -(-int(y_max) // factor) * factor


def path(w_ceil, x_lengths, y_lengths, Tp):
    """generate_path of the masked durations: attn (B, Tx, Tp) float32.  Frame ty belongs to token i when cum[i - 1] <= ty < cum[i],
    with cum the float32 prefix sums (every prefix the exact sum rounded once: torch's CPU cumsum accumulates float32 in double, and
    a double holds these sums exactly), compared as floats with arange(Tp), as sequence_mask does; masked by both lengths."""
    w = w_ceil.to("cpu", torch.float32).reshape(w_ceil.shape[0], -1)
    B, Tx = w.shape
    cum = torch.cumsum(w.double(), 1).float()
    prev = torch.cat((torch.full((B, 1), -math.inf), cum[:, :-1]), dim=1)
    ty = torch.arange(Tp, dtype=torch.float32).view(1, 1, Tp)
    inside = (ty < cum.unsqueeze(-1)) & ~(ty < prev.unsqueeze(-1))
    xm = torch.arange(Tx)[None, :, None] < x_lengths.cpu().view(B, 1, 1)
    ym = torch.arange(Tp)[None, None, :] < y_lengths.cpu().view(B, 1, 1)
    return (inside & xm & ym).float()


def expand(attn, mu_x):
    """mu_y (B, 80, Tp) = attn^T mu_x as the gather it is: every frame has at most one token."""
    assert float(attn.sum(1).max()) <= 1.0
    src = attn.argmax(1)                                                   # (B, Tp)
    has = attn.sum(1) > 0
    mu_x = mu_x.cpu()
    g = torch.gather(mu_x, 2, src.unsqueeze(1).expand(-1, mu_x.shape[1], -1))
    return torch.where(has.unsqueeze(1), g, torch.zeros_like(g))


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the case list
# ---------------------------------------------------------------------------------------------------------------------
B_BENCH, TX_BENCH = 64, 151
EDGE_TX = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 257, 513)
BENCH_EDGE_LENGTHS = (1, 63, 64, 65, 128, 150, 151)


def bench_inputs(n_vocab=W.N_VOCAB_DEFAULT, n_spks=W.N_SPKS_EMOJI, B=B_BENCH, Tx=TX_BENCH):
    """(ids (B, Tx), speaker ids (B,)) exactly as bench.time_text_encoder draws them: seed 77, ids first, then the speakers."""
    g = torch.Generator().manual_seed(77)
    ids = torch.randint(1, n_vocab, (B, Tx), generator=g)
    return ids, torch.randint(0, n_spks, (B,), generator=g)


def bench_ragged_lengths(B=B_BENCH, Tx=TX_BENCH):
    """Odd and even lengths over the batch, with 1, 63, 64, 65, 128, 150 and 151 among them."""
    L = [2 + (53 * r) % (Tx - 2) for r in range(B)]
    for i, v in enumerate(BENCH_EDGE_LENGTHS):
        L[(9 * i + 4) % B] = v
    return torch.tensor(L, dtype=torch.long)


def random_inputs(B, Tx, seed, n_vocab=W.N_VOCAB_DEFAULT, n_spks=W.N_SPKS_EMOJI):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, n_vocab, (B, Tx), generator=g), torch.randint(0, n_spks, (B,), generator=g)


def cases():
    """[(name, ids, lengths, speaker ids)] for the emoji checkpoints (178 symbols, 109 speakers): the bench batch with full and with
    ragged lengths, every edge Tx as a ragged B = 3 batch (lengths Tx, 1, Tx // 2: row 0 alone is the B = 1 call, rows being
    independent), the long call and the batch with a zero-length row between full rows."""
    ids, spk = bench_inputs()
    out = [("bench full", ids, torch.full((B_BENCH,), TX_BENCH, dtype=torch.long), spk),
           ("bench ragged", ids, bench_ragged_lengths(), spk)]
    for Tx in EDGE_TX:
        i, s = random_inputs(3, Tx, 5000 + Tx)
        out.append((f"edge {Tx}", i, torch.tensor([Tx, 1, Tx // 2]), s))
    i, s = random_inputs(2, 1200, 1200)
    out.append(("long 2x1200", i, torch.tensor([1200, 333]), s))
    i, s = random_inputs(3, 40, 40)
    out.append(("zero-length row", i, torch.tensor([40, 0, 40]), s))
    return out


def single_speaker_case():
    """(state dict, ids, lengths): synthetic_matcha_state(178, 1) (no speaker rows, C = 192) at one mid shape."""
    ids, _ = random_inputs(4, 100, 192, n_spks=1)
    return W.synthetic_matcha_state(178, 1), ids, torch.tensor([100, 37, 64, 99])


def speaker_rows(sd, spk_ids):
    return sd["spk_emb.weight"][spk_ids].float()


def errors(got, ref, lengths):
    """(RMS, max) of got - ref over the valid tokens of one call; got, ref (B, C, Tx)."""
    valid = (torch.arange(ref.shape[-1])[None, :] < lengths.cpu()[:, None]).unsqueeze(1).expand_as(ref)
    e = (got.detach().cpu().double() - ref.cpu().double())[valid]
    if e.numel() == 0:
        return 0.0, 0.0
    return float(e.pow(2).mean().sqrt()), float(e.abs().max())
