#!/usr/bin/env python3
"""Time the no-grad validation pass both ways on the same seeded (text, mel) pairs (HIP events, median of N calls after warm-up).

    python tools/cfm_loss_bench.py [--calls 30] [--out profiles/cfm_loss_bench.json]

  (a) MatchaTTS.forward(batched=True)    one ev_cfm_loss call: one time per utterance inside the U-Net, y_t and u never stored
  (b) MatchaTTS.forward(batched=False)   the row-by-row path: B batch-1 ev_estimator passes between torch ops (the baseline)
Shapes: B = 16 and B = 64 at Tx = 120, Ty = 516; ragged lengths, y = mu_x expanded + noise, t and z fixed.  Both include the text
encoder and the alignment search, which are the same calls in both.  The host clock around back-to-back calls is printed beside the
event times.  No ratio is promised; none of the figures is a gate.

Measured: not measured (no GPU run of this tool has been recorded yet).
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
from emojivoice_amd.matcha_tts import synthetic  # noqa: E402

SHAPES = [(16, 120, 516), (64, 120, 516)]
timed = functools.partial(bench_timing.timed, warmup=3, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cfm_loss_bench.json"))
    args = ap.parse_args()
    model = synthetic()
    dev = model.device
    res = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for (B, Tx, Ty) in SHAPES:
        ids, xl, spks, yl, t, z = R.forward_texts(B, Tx, Ty, seed=B + Tx)
        ids, xl, spks, yl, t, z = ids.to(dev), xl.to(dev), spks.to(dev), yl.to(dev), t.to(dev), z.to(dev)
        spk = model._sd["spk_emb.weight"][spks]
        mu_x, _, _ = model.encode(ids, xl, spk)
        _, y, _, _ = R.mel_pairs("aligned", B, Tx, Ty, B + Tx + 2, mu_x=mu_x.cpu(), x_lengths=xl.cpu(), y_lengths=yl.cpu())
        y = y.to(dev)
        a = timed(lambda: model.forward(ids, xl, y, yl, spks, t=t, z=z, batched=True), args.calls)
        b = timed(lambda: model.forward(ids, xl, y, yl, spks, t=t, z=z, batched=False), args.calls)
        ra, rb = model.forward(ids, xl, y, yl, spks, t=t, z=z, batched=True), model.forward(ids, xl, y, yl, spks, t=t, z=z, batched=False)
        rel = [abs(float(p) - float(q)) / abs(float(q)) for p, q in zip(ra[:3], rb[:3])]
        res["shapes"][f"B{B}_Tx{Tx}_Ty{Ty}"] = {"forward_batched": a, "forward_row_by_row": b, "ratio_of_medians": b["median_ms"] / a["median_ms"],
                                                 "losses_batched": [float(v) for v in ra[:3]], "losses_row_by_row": [float(v) for v in rb[:3]],
                                                 "relative_difference_dur_prior_diff": rel, "same_alignment": bool(torch.equal(ra[3], rb[3]))}
        print(f"(B, Tx, Ty) = {(B, Tx, Ty)}: (a) batched {a['median_ms']:.2f} ms  (b) row by row {b['median_ms']:.2f} ms  [min {a['min_ms']:.2f} / {b['min_ms']:.2f}]"
              f"  (host clock, back to back: {a['host_clock_back_to_back_ms']:.2f} / {b['host_clock_back_to_back_ms']:.2f} ms)\n"
              f"    losses differ by a relative {rel[0]:.1e} / {rel[1]:.1e} / {rel[2]:.1e} (dur / prior / diff); same alignment: {torch.equal(ra[3], rb[3])}")
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
