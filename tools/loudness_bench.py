#!/usr/bin/env python3
"""Time ev_loudness beside a device-to-device copy of the bytes it reads (HIP events, median of N calls after warm-up).

    python tools/loudness_bench.py [--calls 20] [--out profiles/loudness_bench.json]

Shapes at 22.05 kHz (S = 2205, the coefficients of audio.k_weighting(22050)): 64 x 6 s and 1 x 6 s (132 300 samples a row: 130 chunks of the
filter) and 1 x 600 s (13 230 000 samples: 12 920 chunks).  The call reads the input twice (once per filter pass; the second read of a short
row comes out of the caches) and writes a few doubles per chunk; the yardstick is a copy that moves the input's bytes once.  The kernel is
NOT expected near that copy at these sizes: it is LATENCY-bound — a lane walks its 1024-sample chunk as one chain of float64 fmas, twice,
and even 64 x 6 s gives only 192 waves to 1024 SIMDs.  What the figures show is whether the time-parallel scheme works: one row of 600 s
holds 100 x the samples of one row of 6 s, and a kernel that walked a row as one chain would take 100 x as long.  The script prints that ratio.
The input is Gaussian noise at -20 dBFS (the cost does not depend on the data).  None of the figures is a gate.
"""
import argparse
import functools
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_timing  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, S, CHUNK = 22050, 2205, 1024
timed = functools.partial(bench_timing.timed, warmup=5, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loudness_bench.json"))
    args = ap.parse_args()
    coef = np.ascontiguousarray(audio.k_weighting(SR))
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "sub_len": S, "chunk": CHUNK, "shapes": {}}
    g = torch.Generator().manual_seed(0)
    eng = Engine(0)
    for B, seconds in ((64, 6), (1, 6), (1, 600)):
        L = seconds * SR
        NS = L // S
        x = (0.1 * torch.randn(B, L, generator=g)).cuda()
        sub = torch.empty(B, NS, dtype=torch.float64, device="cuda")
        block = torch.empty(B, max(NS - 3, 0), dtype=torch.float64, device="cuda")
        gated = torch.empty(B, 2, dtype=torch.float64, device="cuda")
        counts = torch.empty(B, 3, dtype=torch.int32, device="cuda")

        def measure():
            rc = eng.lib.ev_loudness(eng.h, x.data_ptr(), None, B, L, S, coef.ctypes.data, audio.ABSOLUTE_GATE, sub.data_ptr(), block.data_ptr(),
                                     gated.data_ptr(), counts.data_ptr(), _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        measure()
        torch.cuda.synchronize()
        lufs = audio.lufs(gated[:, 0]).cpu()
        nbytes = 4 * B * L
        src, dst = torch.randn(B * L, device="cuda"), torch.empty(B * L, device="cuda")
        tl = timed(measure, args.calls)
        cp = timed(lambda: dst.copy_(src), args.calls)
        res["shapes"][f"B{B}_{seconds}s"] = {
            "samples": B * L, "chunks_per_row": -(-(NS * S) // CHUNK), "input_bytes": nbytes, "integrated_lufs_row0": float(lufs[0]),
            "blocks_row0": int(counts[0, 0]), "ev_loudness": tl, "copy_of_the_input": cp, "ratio_of_medians": tl["median_ms"] / cp["median_ms"],
            "audio_seconds_per_second": B * seconds / (tl["median_ms"] * 1e-3)}
        print(f"B={B} {seconds} s: ev_loudness {tl['median_ms']:.4f} ms  copy of the input {cp['median_ms']:.4f} ms  ratio {tl['median_ms'] / cp['median_ms']:.1f}  "
              f"({B * seconds / (tl['median_ms'] * 1e-3):.0f} s of audio per second; row 0: {float(lufs[0]):.2f} LUFS over {int(counts[0, 0])} blocks; "
              f"host clock, back to back: {tl['host_clock_back_to_back_ms']:.4f} / {cp['host_clock_back_to_back_ms']:.4f} ms)")
        del x, src, dst
    t6, t600 = res["shapes"]["B1_6s"]["ev_loudness"]["median_ms"], res["shapes"]["B1_600s"]["ev_loudness"]["median_ms"]
    res["one_row_600s_over_one_row_6s"] = t600 / t6
    print(f"1 x 600 s takes {t600 / t6:.1f} x the time of 1 x 6 s for 100 x the samples (a row walked as one chain would take 100 x)")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
