#!/usr/bin/env python3
"""Time the monotonic alignment search three ways on the same inputs (HIP events, median of N calls after warm-up).

    python tools/mas_bench.py [--calls 30] [--out profiles/mas_bench.json]

  (a) ev_mas_align with attn, durations and mu_y, without d_logp      (what MatchaTTS.forward calls)
  (b) ev_mas_align, durations only                                    (what a durations script needs)
  (c) ev_log_prior then ev_maximum_path with path and durations       (the two-call route: the (B, Tx, Ty) scores go through memory)
Shapes (B, Tx, Ty): (64, 120, 516), (64, 300, 1032), (1, 200, 860); ragged lengths, y = mu_x expanded + noise.  For context the bytes
the fused route avoids are printed: the fp32 score matrix written and read again on the device, and the device -> host -> device
round trip of that matrix and of the int32 path the reference makes.  None of the figures is a gate.
"""
import argparse
import functools
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench_timing  # noqa: E402
import mas_ref as R  # noqa: E402
from emojivoice_amd._lib import Engine  # noqa: E402

SHAPES = [(64, 120, 516), (64, 300, 1032), (1, 200, 860)]
timed = functools.partial(bench_timing.timed, warmup=5, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mas_bench.json"))
    args = ap.parse_args()
    eng = Engine(0)
    res = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for (B, Tx, Ty) in SHAPES:
        mu_x, y, xl, yl = R.mel_pairs("aligned", B, Tx, Ty, seed=B + Tx)
        mu_x, y, xl, yl = mu_x.cuda(), y.cuda(), xl.cuda().int(), yl.cuda().int()
        a = timed(lambda: eng.mas_align(mu_x, y, xl, yl), args.calls)
        b = timed(lambda: eng.mas_align(mu_x, y, xl, yl, want_attn=False, want_mu_y=False), args.calls)
        c = timed(lambda: eng.maximum_path(eng.log_prior(mu_x, y), xl, yl), args.calls)
        r1, r2 = eng.mas_align(mu_x, y, xl, yl), eng.maximum_path(eng.log_prior(mu_x, y), xl, yl)
        same = bool(torch.equal(r1["attn"], r2[0]) and torch.equal(r1["dur"], r2[1]))
        matrix = B * Tx * Ty * 4
        res["shapes"][f"B{B}_Tx{Tx}_Ty{Ty}"] = {"fused_attn_dur_mu_y": a, "fused_durations_only": b, "log_prior_then_maximum_path": c,
                                                 "routes_agree_bit_for_bit": same, "score_matrix_bytes": matrix,
                                                 "device_bytes_avoided": 2 * matrix, "reference_host_round_trip_bytes": 2 * matrix}
        print(f"(B, Tx, Ty) = {(B, Tx, Ty)}: (a) fused {a['median_ms']:.3f} ms  (b) durations only {b['median_ms']:.3f} ms  (c) two calls {c['median_ms']:.3f} ms"
              f"  [min {a['min_ms']:.3f} / {b['min_ms']:.3f} / {c['min_ms']:.3f}]  same result: {same}\n"
              f"    the fused route avoids {2 * matrix / 1e6:.1f} MB of device traffic (scores written and read again); the reference moves "
              f"{2 * matrix / 1e6:.1f} MB over the host link (scores down, int32 path up) and searches one row after another on one core")
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
