#!/usr/bin/env python3
"""Golden vectors of HiFi-GAN generators other than V1, from the REFERENCE's own module.

Runs ONLY in the build container (needs the reference checkout, which never travels to
the GPU box).  Usage:  python tests/golden/make_vocoder_golden.py

``matcha.hifigan.models.Generator`` imports unmodified; it builds ResBlock1 or ResBlock2
from ``h.resblock`` (models.py:106-145, 160).  Per config (V2, V3 and one off-standard
ResBlock2 config) the script loads the key-seeded synthetic weights of
``emojivoice_amd.weights`` with ``load_state_dict(strict=True)`` — which pins every
parameter name and shape of ``hifigan_shapes`` — records those names and shapes, and runs
a small ragged batch: mel lengths below the padded length, the tail filled with mel_mean
(what a batched decode hands the vocoder).  Output: tests/golden/vocoder_configs.npz.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/Matcha-TTS"
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

# resblock "2" on four levels of rate 4: ResBlock2 at 64 / 32 / 16 / 8 channels, and a k = 7, d = 12 conv (halo 36) on the first level
OFFSTD = {"resblock": "2", "upsample_rates": [4, 4, 4, 4], "upsample_kernel_sizes": [8, 8, 8, 8], "upsample_initial_channel": 128,
          "resblock_kernel_sizes": [3, 5, 7], "resblock_dilation_sizes": [[1, 2], [2, 6], [3, 12]], "num_mels": 80,
          "sampling_rate": 22050, "hop_size": 256}


def main():
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    from emojivoice_amd import weights as W
    from emojivoice_amd.hifigan import v2, v3
    from matcha.hifigan.env import AttrDict
    from matcha.hifigan.models import Generator

    out = {}
    lengths = [24, 17, 9]
    g = torch.Generator().manual_seed(2024)
    for name, cfg in (("v2", v2), ("v3", v3), ("offstd", OFFSTD)):
        h = AttrDict(cfg)
        sd = W.synthetic_hifigan_state(h)
        gen = Generator(h)
        gen.remove_weight_norm()
        gen.load_state_dict(sd, strict=True)
        gen.eval()
        ref_names = list(gen.state_dict().keys())
        out[f"{name}_param_names"] = np.array(ref_names)
        out[f"{name}_param_shapes"] = np.array([list(gen.state_dict()[k].shape) + [0] * (3 - gen.state_dict()[k].dim()) for k in ref_names], np.int64)
        out[f"{name}_config"] = np.array(json.dumps({k: cfg[k] for k in OFFSTD}))
        T = max(lengths)
        mel = torch.full((len(lengths), 80, T), W.MEL_MEAN_EMOJI)
        for b, n in enumerate(lengths):
            mel[b, :, :n] = torch.randn(80, n, generator=g) * 2.0 - 5.0
        with torch.inference_mode():
            wav = gen(mel)
        out[f"{name}_mel"] = mel.numpy()
        out[f"{name}_lengths"] = np.array(lengths, np.int64)
        out[f"{name}_wav"] = wav.numpy()
        print(f"{name}: {len(ref_names)} tensors, wav {tuple(wav.shape)} rms {float(wav.pow(2).mean().sqrt()):.3f}")
    path = os.path.join(HERE, "vocoder_configs.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
