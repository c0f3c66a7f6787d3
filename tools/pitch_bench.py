#!/usr/bin/env python3
"""Time ev_pitch_yin beside a device-to-device copy of the bytes it moves (HIP events, median of N calls after warm-up).

    python tools/pitch_bench.py [--calls 20] [--out profiles/pitch_bench.json]

Shapes: 6 s at 22.05 kHz (132 300 samples), B = 64 and B = 1, the defaults of audio.pitch_yin (frame 1024, hop 256, lags 36 .. 340 =
65 .. 600 Hz, threshold 0.1): 517 frames per row.  The call reads the input once from HBM (every frame stages its 1365 samples; the
overlap comes out of the caches) and writes three (B, F) outputs; the yardstick is a copy that moves as many bytes.  The kernel is NOT
expected near that copy: it is arithmetic-bound, W (tau_max + 1) = 349 184 float64 fmas per frame (each with one float64 subtraction
and one conversion), so the figure that matters is the fma rate printed beside it.  The input is a 3-harmonic tone under noise, so that
frames are voiced and the decision takes its usual path (the cost does not depend on the data otherwise).  None of the figures is a gate.
"""
import argparse
import functools
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_timing  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

W, H, TAU_MIN, TAU_MAX, THRESHOLD = 1024, 256, 36, 340, 0.1
timed = functools.partial(bench_timing.timed, warmup=5, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pitch_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "frame_length": W, "hop_length": H, "tau_min": TAU_MIN, "tau_max": TAU_MAX, "threshold": THRESHOLD,
           "shapes": {}}
    g = torch.Generator().manual_seed(0)
    sr, L = 22050, 6 * 22050
    F = -(-L // H)
    eng = Engine(0)
    for B in (64, 1):
        t = torch.arange(L, dtype=torch.float64) / sr
        f0 = 90.0 + 4.0 * torch.arange(B, dtype=torch.float64)[:, None]                       # 90 .. 342 Hz, one per row
        x = sum(a * torch.sin(2 * math.pi * f0 * k * t) for k, a in ((1, 0.3), (2, 0.15), (3, 0.075)))
        x = (x + 0.01 * torch.randn(B, L, generator=g, dtype=torch.float64)).float().cuda()
        lag = torch.empty(B, F, dtype=torch.int32, device="cuda")
        period, cmnd = torch.empty(B, F, device="cuda"), torch.empty(B, F, device="cuda")

        def track():
            rc = eng.lib.ev_pitch_yin(eng.h, x.data_ptr(), None, B, L, W, H, TAU_MIN, TAU_MAX, THRESHOLD, lag.data_ptr(), period.data_ptr(), cmnd.data_ptr(),
                                      _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        track()
        torch.cuda.synchronize()
        voiced = int((lag > 0).sum())
        nbytes = 4 * (B * L + 3 * B * F)                                # read x once, write the three outputs
        n_copy = max(nbytes // 8, 1)                                    # floats: read once, written once = the same bytes
        src, dst = torch.randn(n_copy, device="cuda"), torch.empty(n_copy, device="cuda")
        tp = timed(track, args.calls)
        cp = timed(lambda: dst.copy_(src), args.calls)
        fmas = B * F * W * (TAU_MAX + 1)
        res["shapes"][f"B{B}_L{L}"] = {
            "frames": B * F, "voiced_frames": voiced, "bytes_moved": nbytes, "float64_fmas": fmas, "ev_pitch_yin": tp, "copy_same_bytes": cp,
            "ratio_of_medians": tp["median_ms"] / cp["median_ms"], "fma_T_per_s": fmas / (tp["median_ms"] * 1e-3) / 1e12,
            "audio_seconds_per_second": B * L / sr / (tp["median_ms"] * 1e-3)}
        print(f"B={B} L={L}: ev_pitch_yin {tp['median_ms']:.4f} ms  copy of the same bytes {cp['median_ms']:.4f} ms  ratio {tp['median_ms'] / cp['median_ms']:.1f}  "
              f"({fmas / (tp['median_ms'] * 1e-3) / 1e12:.2f} T float64 fma/s; {B * F} frames, {voiced} voiced; "
              f"host clock, back to back: {tp['host_clock_back_to_back_ms']:.4f} / {cp['host_clock_back_to_back_ms']:.4f} ms)")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
