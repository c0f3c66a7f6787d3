#!/usr/bin/env python3
"""Time ev_mel_spectrogram beside ev_stft_magnitude on the same audio (HIP events, median of N calls after warm-up).

    python tools/mel_bench.py [--calls 30] [--out profiles/mel_spectrogram_bench.json]

ev_stft_magnitude is the nearest equivalent that existed before the analysis path: pad + forward DFT + magnitude, no projection.
Shapes: B = 64 and B = 1 at 132 096 samples (516 frames, the bench utterance).  None of the figures is a gate.
"""
import argparse
import functools
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_timing  # noqa: E402
from emojivoice_amd._lib import Engine  # noqa: E402
from emojivoice_amd.audio import mel_filterbank  # noqa: E402

timed = functools.partial(bench_timing.timed, warmup=5, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mel_spectrogram_bench.json"))
    args = ap.parse_args()
    eng = Engine(0)
    eng.load_mel_basis(mel_filterbank(22050, 1024, 80, 0, 8000))
    L = 132096
    eng.reserve(64, 0, 0, L // 256)
    res = {"device": torch.cuda.get_device_name(0), "samples": L, "n_mels": 80, "shapes": {}}
    g = torch.Generator().manual_seed(0)
    for B in (64, 1):
        y = (torch.randn(B, L, generator=g) * 0.1).cuda()
        mel = timed(lambda: eng.mel_spectrogram(y), args.calls)
        stft = timed(lambda: eng.stft_magnitude(y), args.calls)
        res["shapes"][f"B{B}"] = {"ev_mel_spectrogram": mel, "ev_stft_magnitude": stft, "ratio_of_medians": mel["median_ms"] / stft["median_ms"],
                                  "mel_frames_per_s": B * (L // 256) / (mel["median_ms"] * 1e-3)}
        print(f"B={B}: ev_mel_spectrogram {mel['median_ms']:.3f} ms  ev_stft_magnitude {stft['median_ms']:.3f} ms  ratio {mel['median_ms'] / stft['median_ms']:.2f}"
              f"  (host clock, back to back: {mel['host_clock_back_to_back_ms']:.3f} / {stft['host_clock_back_to_back_ms']:.3f} ms)")
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
