#!/usr/bin/env python3
"""Time ev_dtw with and without a path (HIP events, median of N calls after warm-up).

    python tools/dtw_bench.py [--calls 30] [--out profiles/dtw_bench.json]

Shapes (B, C, Tx, Ty): (64, 13, 516, 560) — a batch of 6 s utterances against their 6.5 s renderings, 13 mel-cepstral coefficients, what
--evaluate_pairs runs; (1, 13, 516, 560) — one pair; (64, 80, 1032, 1100) — 12 s, the whole mel as the feature, two matrix rows per
thread and the decision bits in the handle's arena.  Every row is full length; y is x at sorted random indices plus noise.  The work is
Tx + Ty - 1 dependent anti-diagonals per row, one barrier each, whatever B is (one workgroup per row): the figure that matters is the
time per anti-diagonal printed beside the call's.  With a path, thread 0's backtrack over the decision bits follows (K dependent reads).
None of the figures is a gate.
"""
import argparse
import functools
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_timing  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SHAPES = [(64, 13, 516, 560), (1, 13, 516, 560), (64, 80, 1032, 1100)]
timed = functools.partial(bench_timing.timed, warmup=5, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dtw_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "metric": "euclidean", "shapes": {}}
    g = torch.Generator().manual_seed(0)
    eng = Engine(0)
    for (B, C, Tx, Ty) in SHAPES:
        x = torch.randn(B, C, Tx, generator=g)
        idx = torch.sort(torch.randint(0, Tx, (B, Ty), generator=g), dim=1).values
        y = torch.gather(x, 2, idx[:, None, :].expand(B, C, Ty)) + 0.3 * torch.randn(B, C, Ty, generator=g)
        x, y = x.cuda(), y.cuda()
        cost = torch.empty(B, dtype=torch.float64, device="cuda")
        steps = torch.empty(B, dtype=torch.int32, device="cuda")
        path = torch.empty(B, Tx + Ty - 1, 2, dtype=torch.int32, device="cuda")

        def call(with_path):
            rc = eng.lib.ev_dtw(eng.h, x.data_ptr(), y.data_ptr(), None, None, B, C, Tx, Ty, 0, cost.data_ptr(), steps.data_ptr(),
                                path.data_ptr() if with_path else None, _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        call(True)
        torch.cuda.synchronize()
        k_mean = float(steps.float().mean())
        tp = timed(lambda: call(True), args.calls)
        tn = timed(lambda: call(False), args.calls)
        diags = Tx + Ty - 1
        res["shapes"][f"B{B}_C{C}_Tx{Tx}_Ty{Ty}"] = {
            "anti_diagonals": diags, "cells_per_row": Tx * Ty, "mean_path_steps": k_mean, "with_path": tp, "without_path": tn,
            "us_per_anti_diagonal_with_path": tp["median_ms"] * 1e3 / diags, "us_per_anti_diagonal_without_path": tn["median_ms"] * 1e3 / diags,
            "cells_G_per_s_without_path": B * Tx * Ty / (tn["median_ms"] * 1e-3) / 1e9}
        print(f"B={B} C={C} {Tx}x{Ty}: with a path {tp['median_ms']:.4f} ms ({tp['median_ms'] * 1e3 / diags:.3f} us per anti-diagonal), without "
              f"{tn['median_ms']:.4f} ms ({tn['median_ms'] * 1e3 / diags:.3f} us per anti-diagonal); mean path {k_mean:.0f} steps; "
              f"host clock, back to back: {tp['host_clock_back_to_back_ms']:.4f} / {tn['host_clock_back_to_back_ms']:.4f} ms")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
