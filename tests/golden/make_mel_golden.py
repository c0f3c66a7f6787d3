#!/usr/bin/env python3
"""Golden vector of the analysis side, from the REFERENCE's own ``mel_spectrogram``.

Runs ONLY where a checkout of the reference exists (it never travels to the GPU box), once, by hand — never by a test:

    python tests/golden/make_mel_golden.py <path of the reference's Matcha-TTS directory>

``matcha/utils/audio.py`` is loaded from that checkout unmodified (by file, so that the package's ``__init__`` with its training-side
imports does not run).  The one third-party package it needs that is absent offline, librosa, is pre-registered in ``sys.modules`` as
an inert stand-in whose ``filters.mel`` returns ``emojivoice_amd.audio.mel_filterbank`` — the filter bank is therefore NOT pinned to
librosa by this vector; everything after it (reflect padding, torch.stft with the periodic Hann window, the 1e-9
inside the root, the matmul, the clamp and the log) is the reference's own float32 arithmetic.

Output: tests/golden/mel_vectors.npz with the seeded 2 x 8192 signal ``y``, the call's arguments and the reference's output ``mel``.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

ARGS = dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000)


def signal():
    """Row 0: white noise under a slow envelope (standard deviation 0.02 .. 0.2); row 1: five sines on and between bins over noise of
    their amplitude (the spectral peaks stand ~13x above the noise: float32's own error stays near 1e-6 in log units, so that the fp64
    yardstick of the tests can be held to this vector at 1e-5)."""
    g = torch.Generator().manual_seed(20240607)
    n = torch.arange(8192, dtype=torch.float64)
    env = 0.11 + 0.09 * torch.sin(2 * np.pi * n / 8192 * 1.5)
    r0 = torch.randn(8192, generator=g, dtype=torch.float64) * env
    bins = torch.tensor([12.0, 40.5, 97.25, 200.0, 333.7], dtype=torch.float64)
    r1 = sum(0.01 * torch.sin(2 * np.pi * b * n / 1024 + i) for i, b in enumerate(bins))
    r1 = r1 + 0.01 * torch.randn(8192, generator=g, dtype=torch.float64)
    return torch.stack([r0, r1]).to(torch.float32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    from emojivoice_amd.audio import mel_filterbank

    def mel(*, sr, n_fft, n_mels, fmin, fmax):
        return mel_filterbank(sr, n_fft, n_mels, fmin, fmax)

    librosa = types.ModuleType("librosa")
    librosa.filters = types.ModuleType("librosa.filters")
    librosa.filters.mel = mel
    sys.modules["librosa"], sys.modules["librosa.filters"] = librosa, librosa.filters
    spec = importlib.util.spec_from_file_location("matcha_utils_audio", os.path.join(ref, "matcha", "utils", "audio.py"))
    audio = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audio)

    torch.set_num_threads(1)
    y = signal()
    with torch.inference_mode():
        out = audio.mel_spectrogram(y, ARGS["n_fft"], ARGS["num_mels"], ARGS["sampling_rate"], ARGS["hop_size"], ARGS["win_size"],
                                    ARGS["fmin"], ARGS["fmax"], center=False)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 80, 32), (out.dtype, out.shape)
    path = os.path.join(HERE, "mel_vectors.npz")
    np.savez_compressed(path, y=y.numpy(), mel=out.numpy(), **{k: np.array(v) for k, v in ARGS.items()})
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KB): mel {tuple(out.shape)} min {float(out.min()):.3f} max {float(out.max()):.3f}")


if __name__ == "__main__":
    main()
