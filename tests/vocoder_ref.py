"""fp64 statement of the HiFi-GAN generator and a windowed form of it (a plain module: the CPU and GPU vocoder tests import it).

``restate`` is a plain-torch statement of ``matcha.hifigan.models.Generator.forward`` for ResBlock1 and ResBlock2 (models.py:80-197) at
any config, precision and device, weight norm folded.  ``restate_windows`` evaluates it on frame windows of single rows: a window's
output equals the full row's on its frames once the mel it runs on reaches ``MARGIN`` frames past either side (clipped at the row's
ends, where the zero padding of every conv is the same in both).  The V1 receptive field reaches 12.4 frames left and 13.4 right
(pinned by test_vocoder_v1_reference.py), so 16 frames leave room.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from emojivoice_amd import weights as W

MARGIN = 16          # mel frames of context on either side of a window
HOP = 256            # output samples per mel frame (the product of the upsample rates)
LINEAR_POST = 0.05   # conv_post scale of the linear-regime checkpoint


def restate_body(sd, mel, h, dtype=torch.float64, device=None):
    """Generator.forward (models.py:181-192) up to the input of the last leaky_relu: the MRF mean of the last level."""
    sd = {k: v.to(device, dtype) for k, v in sd.items()}
    x = F.conv1d(mel.to(device, dtype), sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3)
    rk, rd = h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]
    nk, rb2 = len(rk), str(h["resblock"]) != "1"
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(x, sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        xs = None
        for j, (kk, ds) in enumerate(zip(rk, rd)):
            p, y = f"resblocks.{i * nk + j}", x
            if rb2:
                for m, d in enumerate(ds):
                    y = y + F.conv1d(F.leaky_relu(y, 0.1), sd[f"{p}.convs.{m}.weight"], sd[f"{p}.convs.{m}.bias"], dilation=d, padding=(kk * d - d) // 2)
            else:
                for m, d in enumerate(ds):
                    t = F.conv1d(F.leaky_relu(y, 0.1), sd[f"{p}.convs1.{m}.weight"], sd[f"{p}.convs1.{m}.bias"], dilation=d, padding=(kk * d - d) // 2)
                    t = F.conv1d(F.leaky_relu(t, 0.1), sd[f"{p}.convs2.{m}.weight"], sd[f"{p}.convs2.{m}.bias"], padding=(kk - 1) // 2)
                    y = y + t
            xs = y if xs is None else xs + y
        x = xs / nk
    return x


def restate_post(sd, x):
    """models.py:193-195: leaky_relu (slope 0.01), conv_post, tanh."""
    w, b = sd["conv_post.weight"].to(x.device, x.dtype), sd["conv_post.bias"].to(x.device, x.dtype)
    return torch.tanh(F.conv1d(F.leaky_relu(x), w, b, padding=3))


def restate(sd, mel, h, dtype=torch.float64, device=None):
    """Generator.forward (models.py:181-197) with ResBlock1 (:80-97) or ResBlock2 (:136-141), weight norm folded."""
    return restate_post(sd, restate_body(sd, mel, h, dtype, device))


def linear_regime_state(h=W.HIFIGAN_V1, salt="ev0"):
    """synthetic_hifigan_state with conv_post's weight and bias scaled by 0.05: the output tanh stays nearly linear (pre-tanh std
    ~0.08 instead of ~0.5), so an upstream error reaches the waveform unshrunk by tanh'."""
    sd = OrderedDict(W.synthetic_hifigan_state(h, salt))
    sd["conv_post.weight"] = sd["conv_post.weight"] * LINEAR_POST
    sd["conv_post.bias"] = sd["conv_post.bias"] * LINEAR_POST
    return sd


def window_span(T, t0, t1, margin=MARGIN):
    """The mel frames [a, b) a window [t0, t1) of a T-frame row runs on."""
    assert 0 <= t0 < t1 <= T, (T, t0, t1)
    return max(0, t0 - margin), min(T, t1 + margin)


def restate_windows(sds, mel, h, wins, margin=MARGIN, dtype=torch.float64, device=None):
    """fp64 output samples [HOP * t0, HOP * t1) of row r for every window (r, t0, t1) of ``wins``, under each state dict of ``sds``.

    The state dicts must differ in conv_post only (the body runs once, with sds[0]).  Windows whose mel spans have one length run as
    one batch.  Returns out[i][n]: the samples of window n under sds[i], on the CPU, in ``dtype``."""
    T = mel.shape[-1]
    spans = [window_span(T, t0, t1, margin) for _, t0, t1 in wins]
    out = [[None] * len(wins) for _ in sds]
    groups = {}
    for n, (a, b) in enumerate(spans):
        groups.setdefault(b - a, []).append(n)
    for idx in groups.values():
        seg = torch.stack([mel[wins[n][0], :, spans[n][0]:spans[n][1]] for n in idx])
        x = restate_body(sds[0], seg, h, dtype, device)
        for i, sd in enumerate(sds):
            y = restate_post(sd, x)[:, 0].cpu()
            for k, n in enumerate(idx):
                _, t0, t1 = wins[n]
                a = spans[n][0]
                out[i][n] = y[k, HOP * (t0 - a):HOP * (t1 - a)]
    return out
