#!/usr/bin/env python3
"""Time ev_resample beside a device-to-device copy of the same bytes (HIP events, median of N calls after warm-up).

    python tools/resample_bench.py [--calls 30] [--out profiles/resample_bench.json]

Shapes: the bench utterance (132 096 samples at 22.05 kHz) coming from 44.1 kHz (1/2: 264 192 samples in) and from 48 kHz (147/320), and
going to 48 kHz (320/147), at B = 64 and B = 1, with scipy's default filter (audio.resample_filter).  The yardstick is HBM: the kernel
must read the input and write the output once, so a copy that moves (input + output) bytes — half of them read, half written — is the
least a memory-bound kernel could take.  FMAs per output are the taps per phase, ceil(n_taps / up).  None of the figures is a gate.
"""
import argparse
import functools
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_timing  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

timed = functools.partial(bench_timing.timed, warmup=5, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "filter": "audio.resample_filter (zeros 10, Kaiser beta 5.0)", "shapes": {}}
    g = torch.Generator().manual_seed(0)
    T = 132096
    for name, orig, new, L in (("44100_to_22050", 44100, 22050, 2 * T), ("48000_to_22050", 48000, 22050, T * 320 // 147), ("22050_to_48000", 22050, 48000, T)):
        up, down = audio.resample_ratio(orig, new)
        taps = audio.resample_filter(up, down)
        eng = Engine(0)
        eng.load_resampler(taps, up, down)
        L_out = -(-L * up // down)
        for B in (64, 1):
            x = (torch.randn(B, L, generator=g) * 0.1).cuda()
            y = torch.empty(B, L_out, device="cuda")

            def call():
                rc = eng.lib.ev_resample(eng.h, x.data_ptr(), None, B, L, y.data_ptr(), L_out, _stream_ptr())
                assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

            n_copy = (B * L + B * L_out) // 2          # floats: read once, written once = the kernel's bytes
            src, dst = torch.randn(n_copy, device="cuda"), torch.empty(n_copy, device="cuda")
            rs = timed(call, args.calls)
            cp = timed(lambda: dst.copy_(src), args.calls)
            nbytes = 4 * B * (L + L_out)
            res["shapes"][f"{name}_B{B}"] = {
                "up": up, "down": down, "n_taps": int(len(taps)), "fma_per_output": -(-len(taps) // up), "samples_in": L, "samples_out": L_out, "bytes_in_plus_out": nbytes,
                "ev_resample": rs, "copy_same_bytes": cp, "ratio_of_medians": rs["median_ms"] / cp["median_ms"],
                "resample_GB_per_s": nbytes / (rs["median_ms"] * 1e-3) / 1e9, "copy_GB_per_s": nbytes / (cp["median_ms"] * 1e-3) / 1e9}
            print(f"{name} B={B}: ev_resample {rs['median_ms']:.4f} ms  copy of the same bytes {cp['median_ms']:.4f} ms  ratio {rs['median_ms'] / cp['median_ms']:.2f}"
                  f"  ({nbytes / (rs['median_ms'] * 1e-3) / 1e9:.0f} GB/s; host clock, back to back: {rs['host_clock_back_to_back_ms']:.4f} / {cp['host_clock_back_to_back_ms']:.4f} ms)")
        eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
