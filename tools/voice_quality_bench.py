#!/usr/bin/env python3
"""Time ev_voice_quality at (n_fft, hop, win) = (1024, 256, 1024) on 64 x 6 s and 1 x 6 s of 22050 Hz audio (HIP events, median of N calls
after warm-up), beside three yardsticks on the same rows:
  * a device-to-device copy of the input (the least a call could cost: it reads every sample once);
  * one ev_stft_dist call at (1024, 256, 1024): its first matrix product is the one ev_voice_quality runs, for two signals instead of one
    and without the second product, so it is what the second product's cost should be judged by;
  * the numpy restatement of the definition (tests/voice_quality_ref.py) on 16 CPU threads.

    python tools/voice_quality_bench.py [--calls 30] [--cpu_calls 2] [--out profiles/voice_quality_bench.json]

The call is arithmetic: per row and frame W NB float64 fmas for each of the two planes of the first product and NBp NQ for the second.  The
achieved rate counts those USEFUL fmas (2 flops each) over the whole call's event time.  The guides give no float64 roof for the matrix
cores and none has been measured here, so no share of peak is stated and no figure is a gate.
"""
import argparse
import functools
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench_timing  # noqa: E402
import voice_quality_ref as R  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, SECONDS, CPU_THREADS = 22050, 6, 16
NFFT, HOP, WIN = 1024, 256, 1024
FLOOR = 1e-7
timed = functools.partial(bench_timing.timed, warmup=3, host_clock=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--cpu_calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voice_quality_bench.json"))
    args = ap.parse_args()
    torch.set_num_threads(CPU_THREADS)
    L = SECONDS * SR
    t = audio.voice_quality_tables(SR, NFFT)
    geom = R.Geometry(NFFT, HOP, WIN, t["q_fit"], t["q_min"], t["q_max"], tuple(map(tuple, t["bands"].tolist())), SR)
    NB, NQ, NF = NFFT // 2 + 1, t["q_max"] - t["q_fit"] + 1, -(-L // HOP)
    NBp = (NB + 3) // 4 * 4
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "seconds": SECONDS, "samples": L, "n_fft": NFFT, "hop": HOP, "win": WIN,
           "quefrencies": [t["q_fit"], t["q_min"], t["q_max"]], "power_floor": FLOOR, "cpu_threads": CPU_THREADS,
           "float64_matrix_roof": "not stated by the guides, not measured", "shapes": {}}
    vq, sd = Engine(0), Engine(0)
    vq.load_voice_quality(audio.stft_dist_window(WIN), audio.stoi_twiddle(NFFT), HOP, NFFT, t["bands"], t["slope_w"], t["q_fit"], t["q_min"], t["q_max"],
                          t["fit_w"], t["q_mean"])
    sd.load_stft_dist(audio.stft_dist_window(WIN), audio.stoi_twiddle(NFFT), HOP, NFFT)
    g = torch.Generator().manual_seed(0)
    for B in (64, 1):
        x_h = 0.1 * torch.randn(B, L, generator=g)
        x = x_h.cuda()
        y = (x_h + 0.01 * torch.randn(B, L, generator=g)).cuda()
        frame = torch.empty(B, NF, 8, dtype=torch.float64, device="cuda")
        peak = torch.empty(B, NF, dtype=torch.int32, device="cuda")
        sums = torch.empty(B, 4, dtype=torch.float64, device="cuda")
        counts = torch.empty(B, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(x)

        def call_vq():
            rc = vq.lib.ev_voice_quality(vq.h, x.data_ptr(), None, B, L, FLOOR, frame.data_ptr(), peak.data_ptr(), None, _stream_ptr())
            assert rc == 0, vq.lib.ev_last_error(vq.h).decode()

        def call_sd():
            rc = sd.lib.ev_stft_dist(sd.h, x.data_ptr(), y.data_ptr(), None, B, L, FLOOR, None, sums.data_ptr(), counts.data_ptr(), _stream_ptr())
            assert rc == 0, sd.lib.ev_last_error(sd.h).decode()

        ts, tsd, tcp = timed(call_vq, args.calls), timed(call_sd, args.calls), timed(lambda: dst.copy_(x), args.calls)
        cpu_ms = []
        for _ in range(args.cpu_calls + 1):                               # (the first is the warm-up)
            t0 = time.perf_counter()
            rf, rp, _, _ = R.batch(x_h.numpy(), None, geom, floor=FLOOR)
            cpu_ms.append((time.perf_counter() - t0) * 1e3)
        cpu = statistics.median(cpu_ms[1:])
        df, dp = frame.cpu().numpy(), peak.cpu().numpy()
        same = dp == rp                                                   # (white noise: near-ties of the cepstral peak may fall either way)
        diff = R.err(df[same], rf[same])
        fma1, fma2 = B * NF * WIN * NB * 2, B * NF * NBp * NQ
        shape = {"rows": B, "frames_per_row": NF, "bins": NB, "quefrencies": NQ, "workgroups": B * -(-NF // 16),
                 "useful_fmas_first_product": fma1, "useful_fmas_second_product": fma2, "ev_voice_quality": ts,
                 "useful_float64_tflops": 2.0 * (fma1 + fma2) / (ts["median_ms"] * 1e-3) / 1e12,
                 "device_to_device_copy_of_the_input": tcp, "ev_stft_dist_same_resolution_two_signals": tsd,
                 "voice_quality_over_stft_dist": ts["median_ms"] / tsd["median_ms"], "voice_quality_over_copy": ts["median_ms"] / tcp["median_ms"],
                 "numpy_restatement_cpu_ms": cpu, "cpu_over_device": cpu / ts["median_ms"],
                 "frames_with_equal_peak": int(same.sum()), "frames": int(same.size), "worst_error_device_against_cpu_on_those": diff,
                 "audio_seconds_per_second": B * SECONDS / (ts["median_ms"] * 1e-3)}
        res["shapes"][f"B{B}_{SECONDS}s"] = shape
        print(f"B={B} {NFFT}/{HOP}/{WIN}: ev_voice_quality {ts['median_ms']:.3f} ms (min {ts['min_ms']:.3f}, max {ts['max_ms']:.3f})  ev_stft_dist "
              f"{tsd['median_ms']:.3f} ms  copy {tcp['median_ms']:.4f} ms  numpy on {CPU_THREADS} threads {cpu:.1f} ms ({cpu / ts['median_ms']:.0f} x)  "
              f"{shape['useful_float64_tflops']:.2f} useful float64 TFLOP/s  {shape['workgroups']} workgroups  device against CPU {diff:.2e} on "
              f"{int(same.sum())} of {same.size} frames with the same q*")
        del x, y, dst
    vq.close()
    sd.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
