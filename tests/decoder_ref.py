"""fp64 statement of the CFM decoder: the U-Net estimator and its Euler solver (a plain module: the CPU and GPU decoder tests import it).

``estimator`` restates ``Decoder.forward`` (decoder.py:363-443; Block1D, ResnetBlock1D :32-61; BasicTransformerBlock with SnakeBeta,
transformer.py:63-80, 243-316; diffusers' Attention as the oracle restates it) and ``solve_euler`` restates ``BASECFM.solve_euler``
(flow_matching.py:32-85), at any precision and on any device.  ``decode`` is what ``ev_cfm_decode2`` computes: the normalised ``dec``.

Precision contract:
  * in fp32, as the reference defines them (and as the engine evaluates them, run_time_mlp in ev_engine.hip): the time grid
    ``torch.linspace(0, 1, n + 1)`` with the running ``t`` / ``dt`` of solve_euler, and the sinusoidal embedding ``sinusoidal_pos_emb``.
    Both stay fp32 whatever ``dtype`` is: at t = 0.7 the fp32 and fp64 embeddings differ by 2.6e-5.
  * in ``dtype`` (fp64 for the yardstick), everything from ``time_mlp.linear_1`` on: every conv, GroupNorm, Mish, LayerNorm, attention,
    SnakeBeta and linear, and the Euler update ``x = x + dt * v`` with ``dt`` the fp32 value.

Masking follows the reference exactly (tests/test_decoder_reference.py pins each trap against a slip):
  * GroupNorm statistics run over all Tp frames, padded frames included (Block1D);
  * the attention mask is ADDED to the scores (+1 on valid keys, +0 on padded keys): padded frames stay live keys and values;
  * ``x * mask`` is applied before every conv, and the output is masked.

``SLIPS`` are plausible kernel mistakes, applied here to show that the GPU gates would see them.  The gates themselves (``GATE``,
``GATE_EST``, ``GATE_PEAKED``, ``REF_FLOOR``) live here so that the CPU and GPU tests read the same numbers.  Two slips stay below the gates:
the sinusoid in fp64 moves ``dec`` by about 3e-6 of a row's RMS and one velocity by 2.4e-5 (t = 0.9); a time grid in fp64 moves ``dec``
by about 5e-8.  The yardstick's fp32 sinusoid and grid are therefore pinned by equality with the oracle's instead.
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from emojivoice_amd import weights as W

PREFIX = "decoder.estimator."
PEAK = 4.0            # attn1.to_q and attn1.to_k scale of the peaked-attention checkpoint: score std ~16 instead of ~1

# Per-row gates, (RMS, L-inf) of the error relative to the row's fp64 RMS, set on an MI355X at 3-3.6x the worst value measured over
# every case, setting and switch of tests/test_gpu_decoder.py.  Relative, because a short row in a long padded batch is large: GroupNorm
# statistics include the padded frames, so a 1-frame row of a 516-frame batch has an RMS near 10 (its error scales with it).
GATE = (3.5e-6, 1.5e-5)      # dec, standard weights (worst measured 1.0e-6 / 4.3e-6)
GATE_EST = (7e-6, 3.5e-5)    # one estimator call, standard weights (worst measured 2.1e-6 / 1.0e-5)
GATE_PEAKED = (3.9e-4, 3.2e-3)   # dec after PEAK_STEPS Euler steps, peaked-attention weights (worst measured 1.3e-4 / 1.07e-3: 3.0x)
PEAK_STEPS = 2               # Euler steps of the peaked cases: past a few steps the peaked U-Net amplifies fp32 rounding chaotically
REF_FLOOR = 0.3              # every compared row's fp64 RMS exceeds this: no comparison is vacuous

PROBE = None                 # a list: every attention appends its mean largest softmax weight (the peaked checkpoint's test)

SLIPS = ("gn_valid_only", "keys_neg_inf", "no_mask_before_conv", "sinusoid_fp64", "grid_fp64", "qk_fp16", "score_scale")
SCORE_SLIP = 2.0**-8         # the ``score_scale`` slip: scores off by one bf16 ulp of their scale, as a mis-rounded static q / k scale


def estimator_state(sd, dtype=torch.float64, device=None):
    """The ``decoder.estimator.*`` entries of a Matcha state dict, prefix stripped, in ``dtype`` on ``device``."""
    return {k[len(PREFIX):]: v.to(device, dtype) for k, v in sd.items() if k.startswith(PREFIX)}


def peaked_attention_state(salt="ev0"):
    """synthetic_matcha_state with every ``attn1.to_q`` and ``attn1.to_k`` multiplied by 4: the scores' std grows ~16x, so the softmaxes
    peak.  This loads the static q / k / v scales of the fp16 attention (qkv_pack_scales) and keeps a peaked softmax from averaging
    errors away, as near-uniform attention of the standard weights does."""
    sd = OrderedDict(W.synthetic_matcha_state(salt=salt))
    for k in sd:
        if k.endswith("attn1.to_q.weight") or k.endswith("attn1.to_k.weight"):
            sd[k] = sd[k] * PEAK
    return sd


def sequence_mask(lengths, Tp, dtype=torch.float64, device=None):
    """(B, 1, Tp) 0/1 frame mask of utils/model.py:7-11."""
    lengths = torch.as_tensor(lengths).to(device)
    return (torch.arange(Tp, device=device).unsqueeze(0) < lengths.unsqueeze(1)).unsqueeze(1).to(dtype)


def sinusoid(t, dim, slips=()):
    """sinusoidal_pos_emb (decoder.py:14-29) of one time value, in fp32 on the CPU (fp64 under the ``sinusoid_fp64`` slip)."""
    dt = torch.float64 if "sinusoid_fp64" in slips else torch.float32
    t = torch.as_tensor(t).to(dt).reshape(1)
    half = dim // 2
    f = torch.exp(torch.arange(half).to(dt) * -(math.log(10000) / (half - 1)))
    e = 1000 * t.unsqueeze(1) * f.unsqueeze(0)
    return torch.cat((e.sin(), e.cos()), dim=-1)


def time_grid(n_steps, slips=()):
    """[(t, dt)] of solve_euler's loop (flow_matching.py:52, 70-83): fp32 scalars (fp64 under the ``grid_fp64`` slip)."""
    span = torch.linspace(0, 1, n_steps + 1, dtype=torch.float64 if "grid_fp64" in slips else torch.float32)
    t, dt = span[0], span[1] - span[0]
    out = []
    for s in range(1, n_steps + 1):
        out.append((t, dt))
        t = t + dt
        if s < n_steps:
            dt = span[s + 1] - t
    return out


def _group_norm(x, mask, w, b, slips, groups=8, eps=1e-5):
    if "gn_valid_only" not in slips:
        return F.group_norm(x, groups, w, b, eps=eps)
    B, C, T = x.shape
    xg, m = x.view(B, groups, C // groups, T), mask.view(B, 1, 1, T)
    n = m.sum(dim=(2, 3), keepdim=True) * (C // groups)
    mean = (xg * m).sum(dim=(2, 3), keepdim=True) / n
    var = ((xg - mean) ** 2 * m).sum(dim=(2, 3), keepdim=True) / n
    y = ((xg - mean) / torch.sqrt(var + eps)).view(B, C, T)
    return y * w.view(1, -1, 1) + b.view(1, -1, 1)


def _block1d(sd, p, x, mask, slips, unmasked=False):
    h = F.conv1d(x if unmasked else x * mask, sd[f"{p}.block.0.weight"], sd[f"{p}.block.0.bias"], padding=1)
    return F.mish(_group_norm(h, mask, sd[f"{p}.block.1.weight"], sd[f"{p}.block.1.bias"], slips)) * mask


def _resnet(sd, p, x, mask, temb, slips, unmasked=False):
    h = _block1d(sd, f"{p}.block1", x, mask, slips, unmasked)
    h = h + F.linear(F.mish(temb), sd[f"{p}.mlp.1.weight"], sd[f"{p}.mlp.1.bias"]).unsqueeze(-1)
    h = _block1d(sd, f"{p}.block2", h, mask, slips)
    return h + F.conv1d(x * mask, sd[f"{p}.res_conv.weight"], sd[f"{p}.res_conv.bias"])


def _attention(sd, p, x, fmask, slips, heads=2):
    """diffusers Attention with AttnProcessor2_0 as the oracle restates it: the (B, T) 0/1 mask added to the scores."""
    b, t, _ = x.shape
    q, k, v = (F.linear(x, sd[f"{p}.to_{n}.weight"]) for n in "qkv")
    if "qk_fp16" in slips:
        q, k = q.half().to(x.dtype), k.half().to(x.dtype)
    hd = q.shape[-1] // heads
    q, k, v = (y.view(b, t, heads, hd).transpose(1, 2) for y in (q, k, v))
    scale = hd**-0.5 * (1 + SCORE_SLIP) if "score_scale" in slips else hd**-0.5
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    bias = fmask.view(b, 1, 1, t)
    if "keys_neg_inf" in slips:
        bias = torch.where(bias > 0, bias, torch.full_like(bias, -math.inf))
    w = torch.softmax(s + bias, dim=-1)
    if PROBE is not None:
        PROBE.append(float(w.amax(-1).mean()))
    o = torch.matmul(w, v)
    return F.linear(o.transpose(1, 2).reshape(b, t, heads * hd), sd[f"{p}.to_out.0.weight"], sd[f"{p}.to_out.0.bias"])


def _transformer(sd, p, x, mask, slips):
    """BasicTransformerBlock (transformer.py:243-316) on (B, C, T), returned as (B, C, T)."""
    x = x.transpose(1, 2)
    dim = x.shape[-1]
    n = F.layer_norm(x, (dim,), sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"], eps=1e-5)
    x = _attention(sd, f"{p}.attn1", n, mask[:, 0], slips) + x
    n = F.layer_norm(x, (dim,), sd[f"{p}.norm3.weight"], sd[f"{p}.norm3.bias"], eps=1e-5)
    h = F.linear(n, sd[f"{p}.ff.net.0.proj.weight"], sd[f"{p}.ff.net.0.proj.bias"])
    h = h + (1.0 / (torch.exp(sd[f"{p}.ff.net.0.beta"]) + 0.000000001)) * torch.pow(torch.sin(h * torch.exp(sd[f"{p}.ff.net.0.alpha"])), 2)
    return (F.linear(h, sd[f"{p}.ff.net.2.weight"], sd[f"{p}.ff.net.2.bias"]) + x).transpose(1, 2)


def estimator(esd, x, mask, mu, t, spk, slips=()):
    """Decoder.forward (decoder.py:363-443) for channels (256, 256), one block per level, two mid blocks.  ``esd``: estimator_state;
    x, mu (B, 80, Tp), mask (B, 1, Tp) and spk (B, 64) in the state's dtype and device; ``t`` a scalar (kept fp32, see the module)."""
    in_ch = esd["time_mlp.linear_1.weight"].shape[1]
    te = sinusoid(t, in_ch, slips).to(x.device, x.dtype)
    te = F.linear(F.silu(F.linear(te, esd["time_mlp.linear_1.weight"], esd["time_mlp.linear_1.bias"])),
                  esd["time_mlp.linear_2.weight"], esd["time_mlp.linear_2.bias"])
    x = torch.cat([x, mu, spk.unsqueeze(-1).expand(-1, -1, x.shape[-1])], dim=1)
    hiddens, masks = [], [mask]
    for i in range(2):
        m = masks[-1]
        x = _resnet(esd, f"down_blocks.{i}.0", x, m, te, slips, unmasked=(i == 0 and "no_mask_before_conv" in slips))
        x = _transformer(esd, f"down_blocks.{i}.1.0", x, m, slips)
        hiddens.append(x)
        if i == 0:
            x = F.conv1d(x * m, esd["down_blocks.0.2.conv.weight"], esd["down_blocks.0.2.conv.bias"], stride=2, padding=1)
        else:
            x = F.conv1d(x * m, esd["down_blocks.1.2.weight"], esd["down_blocks.1.2.bias"], padding=1)
        masks.append(m[:, :, ::2])
    masks = masks[:-1]
    for i in range(2):
        x = _resnet(esd, f"mid_blocks.{i}.0", x, masks[-1], te, slips)
        x = _transformer(esd, f"mid_blocks.{i}.1.0", x, masks[-1], slips)
    for i in range(2):
        m = masks.pop()
        x = _resnet(esd, f"up_blocks.{i}.0", torch.cat([x, hiddens.pop()], dim=1), m, te, slips)
        x = _transformer(esd, f"up_blocks.{i}.1.0", x, m, slips)
        if i == 0:
            x = F.conv_transpose1d(x * m, esd["up_blocks.0.2.conv.weight"], esd["up_blocks.0.2.conv.bias"], stride=2, padding=1)
        else:
            x = F.conv1d(x * m, esd["up_blocks.1.2.weight"], esd["up_blocks.1.2.bias"], padding=1)
    x = _block1d(esd, "final_block", x, m, slips)
    return F.conv1d(x * m, esd["final_proj.weight"], esd["final_proj.bias"]) * mask


def solve_euler(esd, z, mu, mask, n_steps, spk, slips=()):
    """BASECFM.solve_euler (flow_matching.py:55-85): x = x + dt * v with dt the fp32 value, from x = z (already temperature-scaled)."""
    x = z
    for t, dt in time_grid(n_steps, slips):
        x = x + float(dt) * estimator(esd, x, mask, mu, t, spk, slips)
    return x


def decode(sd, mu, lengths, spk, z, n_steps, dtype=torch.float64, device=None, slips=(), esd=None):
    """``dec`` of ev_cfm_decode2 (the normalised decoder output; its padded frames keep z, the velocity being exactly 0 there) for fp32 inputs: mu, z (B, 80, Tp; z already
    temperature-scaled), lengths (B,), spk (B, 64).  Returned in ``dtype`` on ``device``."""
    esd = estimator_state(sd, dtype, device) if esd is None else esd
    Tp = mu.shape[-1]
    mask = sequence_mask(lengths, Tp, dtype, device)
    cast = lambda a: a.to(device, dtype)   # noqa: E731
    return solve_euler(esd, cast(z), cast(mu), mask, n_steps, cast(spk), slips)


def velocity(sd, x, mu, lengths, spk, t, dtype=torch.float64, device=None, esd=None):
    """One estimator call as ev_estimator makes it: the velocity at fp32 time ``t``."""
    esd = estimator_state(sd, dtype, device) if esd is None else esd
    mask = sequence_mask(lengths, mu.shape[-1], dtype, device)
    cast = lambda a: a.to(device, dtype)   # noqa: E731
    return estimator(esd, cast(x), mask, cast(mu), torch.tensor(t, dtype=torch.float32), cast(spk))
