"""Yardstick, test signals and error measure of the mel_spectrogram tests (tests/test_audio_host.py, tests/test_gpu_mel.py).

``mel_yardstick`` is the reference's call sequence (utils/audio.py:45-82: reflect pad 384, ``torch.stft(center=False)`` with the
periodic Hann window, sqrt(re^2 + im^2 + 1e-9), the filter bank, log(clamp(., 1e-5))) on the CPU in the dtype asked for: float64 is
the yardstick, float32 is the reference's own arithmetic, whose distance from the yardstick sets the gate.  Two mutants of it (the
1e-9 outside the root, a symmetric Hann window) show that the gate is not vacuous.
"""
import math

import numpy as np
import torch

CLAMP = 1e-5
SR, N_FFT, HOP, FMIN, FMAX = 22050, 1024, 256, 0, 8000


def mel_yardstick(y, basis, dtype=torch.float64, eps_inside=True, periodic=True, log=True):
    """(B, n_mels, L / 256) from y (B, L) and basis (n_mels, 513); with log=False the mel energies before clamp and log."""
    y = torch.as_tensor(y).detach().cpu().to(dtype)
    basis = torch.as_tensor(basis).detach().cpu().to(dtype)
    pad = (N_FFT - HOP) // 2
    yp = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    win = torch.hann_window(N_FFT, periodic=periodic, dtype=dtype)
    spec = torch.view_as_real(torch.stft(yp, N_FFT, hop_length=HOP, win_length=N_FFT, window=win, center=False, pad_mode="reflect",
                                         normalized=False, onesided=True, return_complex=True))
    p = spec.pow(2).sum(-1)
    mag = torch.sqrt(p + 1e-9) if eps_inside else torch.sqrt(p) + 1e-9
    e = torch.matmul(basis, mag)
    return torch.log(torch.clamp(e, min=CLAMP)) if log else e


def mel_errors(got, y, basis):
    """(max, rms, clamped share) of ``got`` against the fp64 yardstick, in log units.  Max and RMS run over the mel bins whose fp64
    energy is above the 1e-5 clamp; the bins at or below it are compared after the clamp only (they enter `clamp_max`, the fourth
    value: |got - log(1e-5)| there, which a correct result keeps at rounding level unless fp32 error lifts a bin just over the clamp)."""
    e = mel_yardstick(y, basis, log=False)
    ref = torch.log(torch.clamp(e, min=CLAMP))
    d = (torch.as_tensor(got).detach().cpu().double() - ref).abs()
    above = e > CLAMP
    da = d[above]
    mx = float(da.max()) if da.numel() else 0.0
    rms = float(da.pow(2).mean().sqrt()) if da.numel() else 0.0
    dc = d[~above]
    return mx, rms, 1.0 - float(above.double().mean()), float(dc.max()) if dc.numel() else 0.0


def _noise(B, L, amp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, generator=g, dtype=torch.float64) * amp


def signal(kind, B, L, seed=0):
    """Test signals (B, L) float32.  Every kind but `silent` keeps the fp64 yardstick's share of clamped mel bins under 10 %."""
    n = torch.arange(L, dtype=torch.float64)
    if kind.startswith("noise"):                     # noise1, noise1e-2, noise1e-4
        y = _noise(B, L, float(kind[5:]), seed)
    elif kind == "mixed":                            # rows cycle through the three amplitudes
        amps = torch.tensor([1.0, 1e-2, 1e-4], dtype=torch.float64)[torch.arange(B) % 3]
        y = _noise(B, L, 1.0, seed) * amps[:, None]
    elif kind == "sines":                            # 48 sines from bin 6 to 364, alternately on a bin and between two, over a 1e-4 noise floor
        y = _noise(B, L, 1e-4, seed)
        for i in range(48):
            k = 6.0 + 7.5 * i + (0.0 if i % 2 == 0 else 0.25)
            y = y + 0.02 * torch.sin(2 * math.pi * k * n / N_FFT + 0.7 * i)[None, :] * (1.0 + 0.1 * torch.arange(B, dtype=torch.float64))[:, None]
    elif kind == "chirp":                            # linear sweep 50 Hz -> 7.9 kHz at amplitude 0.5 over a 1e-3 noise floor
        f0, f1 = 50.0, 7900.0
        ph = 2 * math.pi * (f0 * n / SR + 0.5 * (f1 - f0) / (L / SR) * (n / SR) ** 2)
        y = 0.5 * torch.sin(ph)[None, :] * (1.0 - 0.2 * torch.arange(B, dtype=torch.float64))[:, None] + _noise(B, L, 1e-3, seed)
    elif kind == "silent":                           # noise at 0.1 with exact zeros over the middle third
        y = _noise(B, L, 0.1, seed)
        y[:, L // 3: 2 * L // 3] = 0.0
    else:
        raise KeyError(kind)
    return y.to(torch.float32)


def silent_frames(L):
    """Frames of signal('silent', ., L) whose 1024-sample window lies wholly inside the zeroed third (padded sample 256 f + j = sample 256 f + j - 384)."""
    lo, hi = L // 3, 2 * L // 3
    return [f for f in range(L // HOP) if 256 * f - 384 >= lo and 256 * f - 384 + N_FFT <= hi]


def silent_constant(basis):
    """What a frame of exact zeros gives per mel bin: log(max(sum_k w[m][k] * sqrt(1e-9), 1e-5)), in fp64 from the float32 basis."""
    e = torch.as_tensor(basis).double().sum(dim=1) * math.sqrt(1e-9)
    return torch.log(torch.clamp(e, min=CLAMP))

