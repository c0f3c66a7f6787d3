"""Yardstick, float32 restatement, test signals, case list and error measure of the denoiser tests (tests/test_denoiser_reference.py,
tests/test_gpu_denoiser.py).

``yardstick`` is the reference's call sequence (hifigan/denoiser.py:25-64: ``torch.stft`` with n_fft 1024, hop 256, the periodic Hann
window, centred with reflect padding; sqrt(re^2 + im^2); atan2; clamp(|X| - bias * strength, 0); mag * (cos, sin); ``torch.istft``) on the
CPU in the dtype asked for: float64 is the yardstick, float32 is the reference's own arithmetic.  Its mutant switches restate six ways
of getting the operation subtly wrong; the gates must catch every one of them.

``restatement_f32`` is the same operation done the way the engine does it, in float32 and without the engine: the windowed DFT bases
from float64 trigonometry rounded to float32, frames times the forward basis, the gain on [re | im], times the inverse basis, overlap-add,
division by the sum of squared windows.  Its distance from the yardstick is what a correct float32 implementation costs, and that, not
the engine's own output, sets the gates (tests/test_denoiser_reference.py).
"""

import numpy as np
import torch

import mel_ref

N_FFT, HOP, NB = 1024, 256, 513
PAD = N_FFT // 2
# Per-row gates (row_errors' three figures): 3 x (5.38e-7, 1.41e-6, 2.03e-6), the worst row of the sequential float32 restatement over
# CASES.  tests/test_denoiser_reference.py has the measured table and re-measures on every run.
GATE_RMS, GATE_MAX, GATE_MAG = 1.61e-6, 4.23e-6, 6.10e-6

# (bias kind, strength): strengths chosen so that the yardstick keeps at least a tenth of every non-silent row's RMS (asserted in
# tests/test_denoiser_reference.py), so an error divided by the input's size is also an honest share of the output's size
PAIRS = {"flat": ("rand2", 0.0005), "voc": ("decay", 0.00025), "off": ("rand2", 0.0)}
# The ladder of tests/test_gpu_denoiser.py: (B, frames, content).  B * (frames + 12) rows per conv launch: one shape per conv build the
# forward (Cin 256 -> Cout 1032) and the inverse (Cin 1032 -> Cout 256) layer reach, an odd batch and the streaming reserve length.
LADDER = [(1, 3, "mixed"), (3, 21, "loud_quiet_loud"), (64, 3, "mixed"), (64, 8, "loud_quiet_loud"), (64, 20, "mixed"),
          (64, 40, "loud_quiet_loud"), (64, 52, "mixed"), (64, 88, "loud_quiet_loud"), (64, 120, "mixed"), (64, 245, "loud_quiet_loud"),
          (7, 516, "mixed"), (1, 1200, "loud_quiet_loud")]
# every ladder shape under both pairs and at strength 0; the bench shape once
CASES = [(B, T, kind, pair) for B, T, kind in LADDER for pair in ("flat", "voc", "off")] + [(64, 516, "mixed", "voc")]
# the short cases the mutants are run on: quiet rows, where the gain removes a share of the signal that a wrong spectrum changes
MUTANT_CASES = [(1, 3, "noise1e-4", "flat"), (3, 21, "noise1e-4", "flat"), (3, 21, "noise1e-4", "voc")]


def case_id(case):
    B, T, kind, pair = case
    return f"B{B}-T{T}-{kind}-{pair}"


def bias(kind):
    """(513,) float32 bias spectrum.  rand2: uniform in [0, 2) (the existing parity test's); decay: a vocoder-like spectrum, loud at the
    low bins and falling over four decades."""
    if kind == "rand2":
        return (torch.rand(NB, generator=torch.Generator().manual_seed(513), dtype=torch.float64) * 2.0).to(torch.float32)
    if kind == "decay":
        k = torch.arange(NB, dtype=torch.float64)
        return (4.0 * torch.exp(-k / 24.0) + 0.02 + 0.01 * torch.cos(0.37 * k)).to(torch.float32)
    raise KeyError(kind)


def signal(kind, B, L, seed=0):
    """(B, L) float32.  mel_ref.signal's kinds (noise1, noise1e-2, noise1e-4, sines, chirp, mixed, silent) and
    loud_quiet_loud: noise at amplitude 1 whose rows 1, 4, 7, .. are scaled by 1e-4 (for B = 1: the one row is loud);
    loud_zero_loud:  the same with rows 1, 4, 7, .. exactly zero."""
    if kind in ("loud_quiet_loud", "loud_zero_loud"):
        y = mel_ref.signal("noise1", B, L, seed).double()
        mid = torch.arange(B) % 3 == 1
        y[mid] = y[mid] * (1e-4 if kind == "loud_quiet_loud" else 0.0)
        return y.to(torch.float32)
    return mel_ref.signal(kind, B, L, seed)


def case_inputs(case):
    """(audio (B, L) float32, bias (513,) float32, strength) of one entry of CASES / MUTANT_CASES."""
    B, T, kind, pair = case
    bk, strength = PAIRS[pair]
    return signal(kind, B, HOP * T, seed=B + T), bias(bk), strength


def _reflect_pad(x, edge_repeated=False):
    """512 samples a side: x[512] .. x[1] | x | x[L-2] .. x[L-513]  (edge_repeated, the mutant: x[511] .. x[0] | x | x[L-1] .. x[L-512])."""
    L = x.shape[-1]
    s = 0 if edge_repeated else 1
    left = x[..., s: s + PAD].flip(-1)
    right = x[..., L - PAD - s: L - s].flip(-1)
    return torch.cat([left, x, right], dim=-1)


def envelope(L, dtype=torch.float64):
    """sum over the frames f in [0, L / 256] of w^2[m - 256 f] at the samples m = 512 .. 512 + L - 1 of the padded signal: torch.istft's
    normalisation.  1.5 everywhere but in the first and last 768 samples."""
    F = L // HOP + 1
    w2 = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64).pow(2)
    env = torch.zeros(HOP * (F + 3), dtype=torch.float64)
    for f in range(F):
        env[HOP * f: HOP * f + N_FFT] += w2
    return env[PAD: PAD + L].to(dtype)


def yardstick(audio, bias, strength, dtype=torch.float64, symmetric_window=False, edge_repeated=False, flat_envelope=False,
              edges_doubled=False, bias_shift=0, gain_on_power=False):
    """(mag (B, 513, L / 256 + 1), out (B, L)) of (B, L) audio in `dtype`.  The keyword switches are the mutants."""
    x = torch.as_tensor(audio).detach().cpu().to(dtype)
    if x.dim() == 1:
        x = x[None]
    b = torch.as_tensor(bias).detach().cpu().to(dtype).reshape(-1)
    L = x.shape[-1]
    win = torch.hann_window(N_FFT, periodic=not symmetric_window, dtype=dtype)
    if edge_repeated:
        spec = torch.stft(_reflect_pad(x, True), n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=win, center=False, return_complex=True)
    else:
        spec = torch.stft(x, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=win, return_complex=True)
    sr = torch.view_as_real(spec)
    mag = torch.sqrt(sr.pow(2).sum(-1))
    # (+ 0.0: a bin that is exactly zero is read at angle 0.  torch's FFT of a silent frame returns -0.0 real parts in about half of
    # the bins, where atan2 gives pi: an accident of the library's signed zeros that only a negative strength on silence can show.
    # No other value changes.)
    ang = torch.atan2(sr[..., -1], sr[..., 0] + 0.0)
    thr = torch.roll(b, bias_shift)[None, :, None] * strength
    den = torch.sqrt(torch.clamp(mag * mag - thr, 0.0)) if gain_on_power else torch.clamp(mag - thr, 0.0)
    z = torch.complex(den * torch.cos(ang), den * torch.sin(ang))
    if edges_doubled:
        z = z.clone()
        z[:, 0] *= 2.0
        z[:, NB - 1] *= 2.0
    out = torch.istft(z, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=win)
    if flat_envelope:
        out = out * (envelope(L, dtype) / 1.5)[None, :]
    return mag, out


_BASES = {}


def bases():
    """(forward (1024, 1026), inverse (1026, 1024), w^2 (1024,)) in float32 from float64 trigonometry: columns / rows [re(513) | im(513)];
    forward w[n] e^{-2 pi i k n / N}, inverse w[n] c_k e^{+2 pi i k n / N} / N with c = 1 at DC and Nyquist (whose imaginary parts do not
    enter) and 2 elsewhere."""
    if not _BASES:
        n = np.arange(N_FFT, dtype=np.int64)
        k = np.arange(NB, dtype=np.int64)
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)
        ang = 2.0 * np.pi * ((n[:, None] * k[None, :]) % N_FFT) / N_FFT                          # (n, k)
        fwd = np.concatenate([win[:, None] * np.cos(ang), -win[:, None] * np.sin(ang)], axis=1)
        ck = np.where((k == 0) | (k == N_FFT // 2), 1.0, 2.0)
        inv_re = (win[:, None] * ck[None, :] * np.cos(ang) / N_FFT).T                            # (k, n)
        inv_im = (-win[:, None] * ck[None, :] * np.sin(ang) / N_FFT).T
        inv_im[0] = 0.0
        inv_im[NB - 1] = 0.0
        _BASES["f"] = torch.from_numpy(fwd.astype(np.float32))
        _BASES["i"] = torch.from_numpy(np.concatenate([inv_re, inv_im], axis=0).astype(np.float32))
        _BASES["w2"] = torch.from_numpy((win * win).astype(np.float32))
    return _BASES["f"], _BASES["i"], _BASES["w2"]


def _matmul_f32(a, w, sequential):
    """a (M, K) @ w (K, N) in float32; sequential: acc = fma(a[:, k], w[k], acc) for k = 0 .. K - 1, every term rounded to float32 as it
    is added (no wider accumulator, no pairwise or blocked order): the least favourable order a correct float32 kernel may take."""
    if not sequential:
        return a @ w
    out = torch.empty(a.shape[0], w.shape[1], dtype=torch.float32)
    for r0 in range(0, a.shape[0], 2048):
        cols = a[r0: r0 + 2048].t().contiguous()
        acc = torch.zeros(cols.shape[1], w.shape[1], dtype=torch.float32)
        for kk in range(w.shape[0]):
            acc.addcmul_(cols[kk][:, None], w[kk][None, :])
        out[r0: r0 + 2048] = acc
    return out


def forward_f32(audio, sequential=False):
    """[re(513) | im(513)] rows (B * (L / 256 + 1), 1026) of the float32 restatement: reflect-padded frames times the forward basis."""
    x = torch.as_tensor(audio).detach().cpu().to(torch.float32)
    if x.dim() == 1:
        x = x[None]
    frames = _reflect_pad(x).unfold(-1, N_FFT, HOP)                                  # (B, F, 1024)
    return _matmul_f32(frames.reshape(-1, N_FFT).contiguous(), bases()[0], sequential)


def restatement_f32(audio, bias, strength, sequential=False, spec=None):
    """(mag, out) the way the engine computes them, in float32 on the CPU (see the module docstring).  spec: forward_f32's result for
    this audio and order, where several strengths share it."""
    B, L = (1, len(audio)) if torch.as_tensor(audio).dim() == 1 else tuple(audio.shape)
    b = torch.as_tensor(bias).detach().cpu().to(torch.float32).reshape(-1)
    _, inv, w2 = bases()
    F = L // HOP + 1
    if spec is None:
        spec = forward_f32(audio, sequential)
    re, im = spec[:, :NB], spec[:, NB:]
    mag = torch.sqrt(re * re + im * im)
    m2 = torch.clamp(mag - b[None, :] * torch.tensor(strength, dtype=torch.float32), min=0.0)
    g = m2 / torch.where(mag > 0, mag, torch.ones_like(mag))
    re2 = torch.where(mag > 0, re * g, m2)                                         # |X| = 0: angle 0
    im2 = torch.where(mag > 0, im * g, torch.zeros_like(im))
    fr = _matmul_f32(torch.cat([re2, im2], dim=1).contiguous(), inv, sequential).reshape(B, F, 4, HOP)
    rows = torch.zeros(B, F + 3, HOP, dtype=torch.float32)
    env = torch.zeros(F + 3, HOP, dtype=torch.float32)
    for j in range(4):                                                                 # row r <- frame r - j, samples 256 j ..
        rows[:, j: j + F] += fr[:, :, j]
        env[j: j + F] += w2[HOP * j: HOP * (j + 1)][None, :]
    out = (rows / env[None]).reshape(B, -1)[:, PAD: PAD + L]
    return mag.reshape(B, F, NB).transpose(1, 2).contiguous(), out.contiguous()


def silent_frame(bias, strength):
    """The 1024-sample frame whose spectrum a silent frame takes under a negative strength: irfft(-bias * strength) (zero phase).
    A silent row has no input to measure an error against; this frame's RMS and peak stand in for the input's in row_errors, as the
    frame (window times input) whose spectrum enters the inverse does in every other case."""
    b = torch.as_tensor(bias).detach().cpu().double().reshape(-1)
    return torch.fft.irfft(torch.complex(-b * strength, torch.zeros_like(b)), n=N_FFT)


def negative_case():
    """(audio, bias, strength, denominators): loud | silent | loud rows of one frame length under a negative strength, where the
    reference adds bias * |strength| to every magnitude and a silent bin comes out as -bias * strength at angle 0.  `denominators`
    takes audio's place in row_errors: the audio, with silent_frame in the silent row."""
    audio, b, strength = signal("loud_zero_loud", 3, N_FFT, seed=3), bias("rand2"), -0.01
    den = audio.double().clone()
    den[1] = silent_frame(b, strength)
    return audio, b, strength, den


def row_errors(got, y64, audio):
    """Per row of the batch, three figures of got = (mag, out) against the yardstick y64 = (mag, out); either half of `got` may be None:
        rms: RMS of the output's error over the RMS of the row's input,
        mx:  largest output error over the row's input peak,
        mg:  largest magnitude error over the row's largest |X| (yardstick).
    The denominators come from the input: where the gain removes most of a row the output shrinks and the error does not.  A row
    whose yardstick output (magnitude) is zero everywhere is compared for equality: 0.0 if every element of `got` is zero, else inf."""
    a = torch.as_tensor(audio).detach().cpu().double()
    if a.dim() == 1:
        a = a[None]
    B = a.shape[0]
    mag64, out64 = y64
    inf = torch.full((B,), float("inf"), dtype=torch.float64)
    zero = torch.zeros(B, dtype=torch.float64)
    rms = mx = mg = None
    if got[1] is not None:
        e = torch.as_tensor(got[1]).detach().cpu().double().reshape(B, -1) - out64.double()
        in_rms, in_peak = a.pow(2).mean(1).sqrt(), a.abs().amax(1)
        exact = out64.abs().amax(1) == 0
        same = torch.where(e.abs().amax(1) == 0, zero, inf)
        rms = torch.where(exact, same, e.pow(2).mean(1).sqrt() / torch.where(exact, torch.ones_like(in_rms), in_rms))
        mx = torch.where(exact, same, e.abs().amax(1) / torch.where(exact, torch.ones_like(in_peak), in_peak))
    if got[0] is not None:
        e = torch.as_tensor(got[0]).detach().cpu().double() - mag64.double()
        top = mag64.double().amax((1, 2))
        exact = top == 0
        mg = torch.where(exact, torch.where(e.abs().amax((1, 2)) == 0, zero, inf), e.abs().amax((1, 2)) / torch.where(exact, torch.ones_like(top), top))
    return rms, mx, mg


def worst(figs):
    """Largest of each of row_errors' three figures (None stays None)."""
    return tuple(None if f is None else float(f.max()) for f in figs)
