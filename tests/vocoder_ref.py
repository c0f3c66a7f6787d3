"""fp64 statement of the HiFi-GAN generator and a windowed form of it (a plain module: the CPU and GPU vocoder tests import it).

``restate`` is a plain-torch statement of ``matcha.hifigan.models.Generator.forward`` for ResBlock1 and ResBlock2 (models.py:80-197) at
any config, precision and device, weight norm folded.  ``restate_windows`` evaluates it on frame windows of single rows: a window's
output equals the full row's on its frames once the mel it runs on reaches ``MARGIN`` frames past either side (clipped at the row's
ends, where the zero padding of every conv is the same in both).  The V1 receptive field reaches 12.4 frames left and 13.4 right
(pinned by test_vocoder_v1_reference.py), so 16 frames leave room.  For any other config the margin follows from the config: ``reach(h)``
bounds the field (pinned by test_vocoder_configs_reference.py), and ``restate_windows`` takes ``ceil(reach(h)) + 2`` when it is given none.

The second half holds what the per-row GPU tests share (test_gpu_vocoder_v1.py, test_gpu_vocoder_configs_fp64.py): the gates, the run /
check / sweep helpers and the window choosers.
"""
import math
import time
from collections import OrderedDict

import torch
import torch.nn.functional as F

from emojivoice_amd import weights as W

MARGIN = 16          # mel frames of context on either side of a window
HOP = 256            # output samples per mel frame (the product of the upsample rates)
LINEAR_POST = 0.05   # conv_post scale of the linear-regime checkpoint


def restate_body(sd, mel, h, dtype=torch.float64, device=None, slope=0.1):
    """Generator.forward (models.py:181-192) up to the input of the last leaky_relu: the MRF mean of the last level.  ``slope``: the
    leaky_relu slope of the body, 0.1 in the model (the yardstick's own sensitivity test states it wrongly on purpose)."""
    sd = {k: v.to(device, dtype) for k, v in sd.items()}
    x = F.conv1d(mel.to(device, dtype), sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3)
    rk, rd = h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]
    nk, rb2 = len(rk), str(h["resblock"]) != "1"
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, slope)
        x = F.conv_transpose1d(x, sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        xs = None
        for j, (kk, ds) in enumerate(zip(rk, rd)):
            p, y = f"resblocks.{i * nk + j}", x
            if rb2:
                for m, d in enumerate(ds):
                    y = y + F.conv1d(F.leaky_relu(y, slope), sd[f"{p}.convs.{m}.weight"], sd[f"{p}.convs.{m}.bias"], dilation=d, padding=(kk * d - d) // 2)
            else:
                for m, d in enumerate(ds):
                    t = F.conv1d(F.leaky_relu(y, slope), sd[f"{p}.convs1.{m}.weight"], sd[f"{p}.convs1.{m}.bias"], dilation=d, padding=(kk * d - d) // 2)
                    t = F.conv1d(F.leaky_relu(t, slope), sd[f"{p}.convs2.{m}.weight"], sd[f"{p}.convs2.{m}.bias"], padding=(kk - 1) // 2)
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


def reach(h):
    """Upper bound, in mel frames, on how far a changed mel frame moves the output on either side (the same on both: measured from the
    frame's first sample leftwards and from its last sample rightwards).

    A change confined to samples [a, b) of a level grows by p on either side under a conv of halo p, and becomes [u a - p, u b + p) with
    p = (k - u) / 2 under a transposed conv of stride u, kernel k and padding (k - u) / 2.  So, at its own level, every layer adds its halo:
    conv_pre 3 (mel frames), the upsampler into level l (k - u) / 2, the widest ResBlock of level l the sum of its convs' halos —
    ResBlock1 (k - 1) d / 2 + (k - 1) / 2 per dilation, ResBlock2 (k - 1) d / 2 — and conv_post 3.  A level's samples are 1 / (its rate
    product) of a mel frame."""
    rb2 = str(h["resblock"]) != "1"
    widest = max(sum((k - 1) * d // 2 + (0 if rb2 else (k - 1) // 2) for d in ds)
                 for k, ds in zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]))
    frames, prod = 3.0, 1
    for u, k in zip(h["upsample_rates"], h["upsample_kernel_sizes"]):
        prod *= u
        frames += ((k - u) // 2 + widest) / prod
    return frames + 3.0 / prod


def default_margin(h):
    """The context ``restate_windows`` takes when it is given none: the bound on the field, rounded up, plus two frames."""
    return math.ceil(reach(h)) + 2


def window_span(T, t0, t1, margin=MARGIN):
    """The mel frames [a, b) a window [t0, t1) of a T-frame row runs on."""
    assert 0 <= t0 < t1 <= T, (T, t0, t1)
    return max(0, t0 - margin), min(T, t1 + margin)


def restate_windows(sds, mel, h, wins, margin=None, dtype=torch.float64, device=None):
    """fp64 output samples [HOP * t0, HOP * t1) of row r for every window (r, t0, t1) of ``wins``, under each state dict of ``sds``.

    The state dicts must differ in conv_post only (the body runs once, with sds[0]).  Windows whose mel spans have one length run as
    one batch.  ``margin`` None: ``default_margin(h)``, which follows the config's receptive field (V1's callers pass ``MARGIN``).
    Returns out[i][n]: the samples of window n under sds[i], on the CPU, in ``dtype``."""
    T = mel.shape[-1]
    if margin is None:
        margin = default_margin(h)
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


# ---------------------------------------------------------------------------------------------------------------------
# what the per-row GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
SETTINGS = (16, 6, 0)
WEIGHTS = ("std", "lin")
GATE = {"std": (5e-6, 5e-5), "lin": (5e-6, 3e-5)}        # (RMS, L-inf): absolute for std, relative to the row's fp64 RMS for lin
REF_FLOOR = {"std": 0.2, "lin": 0.01}                  # the row's fp64 RMS must exceed this: the comparison is not vacuous


def run(voc, mel, setting=16, chain=True, amax=True):
    """The vocoder's output under one arithmetic setting, and how many balanced persistent launches the call made."""
    eng = voc.engine
    eng.set_arithmetic(setting)
    eng.set_chain(chain)
    eng.set_amax(amax)
    try:
        e0 = eng.sk_stats()[0]
        wav = voc(mel)
        torch.cuda.synchronize()
        e1 = eng.sk_stats()[0]
    finally:
        eng.set_arithmetic(16)
        eng.set_chain(True)
        eng.set_amax(True)
    return wav, (e1 - e0) & 0xFFFFFFFF


def fanout_planned(eng, B, T):
    """True when a (B, T) call plans the three-stream MRF fan-out: its workspace exceeds the single-stream plan's."""
    saved = eng.mrf_streams_max
    ws = eng.workspace_bytes(B, 0, T)
    eng.set_mrf_streams_max(0)
    try:
        single = eng.workspace_bytes(B, 0, T)
    finally:
        eng.set_mrf_streams_max(saved)
    assert ws >= single
    return ws > single


def row_errors(wav, wins, refs):
    """{row: (RMS, L-inf of wav - ref over the row's windows, RMS of ref, wav finite)}; ``wav`` a (B, 1, HOP T) tensor or a list of
    per-window samples in the order of ``wins``."""
    per_row = {}
    for n, ((r, t0, t1), ref) in enumerate(zip(wins, refs)):
        got = wav[n] if isinstance(wav, (list, tuple)) else wav[r, 0, HOP * t0:HOP * t1]
        per_row.setdefault(r, []).append((got, ref))
    out = {}
    for r, pairs in per_row.items():
        got = torch.cat([p[0] for p in pairs]).double().cpu()
        ref = torch.cat([p[1] for p in pairs]).double()
        e = got - ref
        out[r] = (float(e.pow(2).mean().sqrt()), float(e.abs().max()), float(ref.pow(2).mean().sqrt()), bool(torch.isfinite(got).all()))
    return out


def check(tag, weights, wav, wins, refs, bad, label="V1ERR", gate=GATE, floor=REF_FLOOR, f32=None, table=None):
    """Per row over its windows: (RMS, L-inf) of the error against the fp64 reference, gated; one table line per call.  ``f32``: the
    plain fp32 torch restatement on the same windows, whose own error against fp64 is printed beside the line (never gated);
    ``table``: a list that collects the printed lines."""
    worst = [0.0, 0.0, 0.0, 0.0, float("inf")]            # rms, linf, rms / ref, linf / ref, smallest ref RMS
    g_rms, g_linf = gate[weights]
    for r, (rms, linf, rr, finite) in row_errors(wav, wins, refs).items():
        worst = [max(worst[0], rms), max(worst[1], linf), max(worst[2], rms / rr), max(worst[3], linf / rr), min(worst[4], rr)]
        scale = 1.0 if weights == "std" else rr
        if not (rms <= g_rms * scale and linf <= g_linf * scale and rr > floor[weights] and finite):
            bad.append((tag, weights, r, rms, linf, rr))
    line = (f"{label} {tag:<34s} {weights}  rms {worst[0]:.2e}  linf {worst[1]:.2e}  rel rms {worst[2]:.2e}  rel linf {worst[3]:.2e}  "
            f"min ref rms {worst[4]:.3f}")
    if f32 is not None:
        w32 = [0.0, 0.0]
        for rms, linf, rr, _ in row_errors(f32, wins, refs).values():
            k = 1.0 if weights == "std" else rr
            w32 = [max(w32[0], rms / k), max(w32[1], linf / k)]
        line += f"  | torch fp32 {'rms' if weights == 'std' else 'rel rms'} {w32[0]:.2e}  {'linf' if weights == 'std' else 'rel linf'} {w32[1]:.2e}"
    print(line)
    if table is not None:
        table.append(line)


def sweep(tag, vocs, mel, wins, refs, bad, settings=SETTINGS, f32=None, **kw):
    """Every setting x checkpoint; returns {setting: balanced launches of the std call}."""
    epochs = {}
    for s in settings:
        for w in WEIGHTS:
            wav, ep = run(vocs[w], mel, s)
            check(f"{tag} s{s}", w, wav, wins, refs[w], bad, f32=None if f32 is None else f32[w], **kw)
            if w == "std":
                epochs[s] = ep
    return epochs


def row_windows(lengths, w=8):
    """Head, tail and one interior window per row; the interior offset steps 8 frames a row, so over 64 rows the interior windows
    cover the whole time axis and, with the rows' 524-frame stride on the flattened axis, every phase of the 128-row tiles."""
    wins = []
    for r, L in enumerate(lengths):
        t0 = w + (w * r) % max(1, L - 2 * w)
        wins += [(r, 0, min(w, L)), (r, max(0, L - w), L), (r, min(t0, L - w), min(t0, L - w) + w)]
    return wins


def gpu_refs(sds, mel, h, wins, clock, check_cpu=1, margin=None, device="cuda:0", f32=False):
    """{weights: [fp64 samples of each window]} through torch on the GPU; the first ``check_cpu`` windows are also run on the CPU and must
    agree to 1e-10.  ``f32``: also the same windows in plain fp32 torch, returned second.  ``clock``: {"gpu_ref", "cpu_ref"} seconds."""
    names = list(WEIGHTS)
    t0 = time.perf_counter()
    got = restate_windows([sds[n] for n in names], mel, h, wins, margin=margin, device=device)
    got32 = None
    if f32:
        with torch.backends.cudnn.flags(enabled=False):    # torch's own conv kernels: no solver search per shape, one arithmetic
            got32 = restate_windows([sds[n] for n in names], mel, h, wins, margin=margin, dtype=torch.float32, device=device)
    torch.cuda.synchronize()
    clock["gpu_ref"] += time.perf_counter() - t0
    if check_cpu:
        t0 = time.perf_counter()
        cpu = restate_windows([sds[n] for n in names], mel.cpu(), h, wins[:check_cpu], margin=margin)
        clock["cpu_ref"] += time.perf_counter() - t0
        for i in range(len(names)):
            for n in range(check_cpu):
                assert float((cpu[i][n] - got[i][n]).abs().max()) <= 1e-10, (names[i], wins[n])
    refs = {n: got[i] for i, n in enumerate(names)}
    return (refs, {n: got32[i] for i, n in enumerate(names)}) if f32 else refs
