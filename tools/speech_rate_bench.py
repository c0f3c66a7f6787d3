#!/usr/bin/env python3
"""Time ev_speech_rate on 64 x 6 s (517 frames) and 1 x 190 s (NF = 16384, the frame limit) of 22.05 kHz audio at the default geometry (W = 1412, hop 256),
with and without d_power / d_mark, beside ``torch_speech_rate``: a batched float64 torch restatement on the device (unfolded frames, a sort for
the rank, cummax / cummin for the runs, a doubling scan for the segmented minimum).  The variants take turns, round by round, under HIP events
(bench_timing.rounds_of): medians with min / max.

    python tools/speech_rate_bench.py [--rounds 10] [--inner 2] [--out profiles/speech_rate_bench.json]

Nothing here is a gate and no ratio is promised: the figures are what was seen.  Every shape is compared with the torch form (marks and counts
equal, worst power error) and the small one with the numpy restatement (tests/speech_rate_ref.py).
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench_timing  # noqa: E402
import speech_rate_ref as R  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine  # noqa: E402

SR, HOP = 22050, 256
SHAPES = ((64, 517 * HOP), (1, 16384 * HOP))                             # (rows, samples): 64 x 6.0 s (517 frames); 1 x 190.2 s, NF = 16384
PAR = dict(R.PAR, min_pause=26, min_sound=9)                            # 0.3 s and 0.1 s at hop 256


def make(B, L):
    """B rows of bursts at hop 256 (about 2 s of speech between silences of 0.46 s), tiled to the length."""
    rows = []
    for b in range(B):
        y = R.bursts(HOP, groups=(4, 3, 4), seed=200 + b, lead=20, trail=20, sr=float(SR))[0]
        rows.append(np.tile(y, -(-L // len(y)))[:L])
    return np.stack(rows)


def shift(t, o, fill):
    """t[..., f + o] at f, ``fill`` past the end."""
    return torch.cat([t[..., o:], torch.full_like(t[..., :o], fill)], -1)


def torch_speech_rate(x, win, par):
    """ev_speech_rate's outputs for full rows by batched torch ops; x (B, L) float32 on the device with L a multiple of the hop.  torch sums in
    its own order, so the power agrees to rounding only."""
    B, L = x.shape
    W, NF = win.shape[0], L // HOP
    sil, dipr = R.ratios(par)
    lo = W // 2 - HOP // 2
    S = torch.nn.functional.pad(x.to(torch.float64), (lo, W)).unfold(1, W, HOP)[:, :NF]
    sw = win.sum()
    m = (S * win).sum(-1) / sw
    P = (win * (S - m[..., None]) ** 2).sum(-1) / sw
    k = int(np.floor(par["rank_fraction"] * float(NF - 1)))
    ref = torch.sort(P, dim=1, descending=True).values[:, k]
    thr = ref * sil
    raw = (P > thr[:, None]) & (P > par["power_floor"])
    idx = torch.arange(NF, device=x.device).expand(B, NF)

    def nearest(flag):                                                   # the nearest frame with the flag at or before / at or behind every frame
        before = torch.cummax(torch.where(flag, idx, torch.full_like(idx, -1)), 1).values
        behind = torch.flip(torch.cummin(torch.flip(torch.where(flag, idx, torch.full_like(idx, NF)), [1]), 1).values, [1])
        return before, behind
    p, q = nearest(raw)
    a = raw | ((p >= 0) & (q < NF) & (q - p - 1 < par["min_pause"]))
    p, q = nearest(~a)
    snd = a & ~(q - p - 1 < par["min_sound"])
    cand = torch.zeros_like(snd)
    mid = P[:, 1:-1]
    cand[:, 1:-1] = (mid > P[:, :-2]) & (mid >= P[:, 2:]) & (mid > thr[:, None]) & snd[:, 1:-1]
    v = shift(P, 1, float("inf"))                                        # element f: frame f + 1; a segment ends in front of a candidate
    h = shift(cand, 2, True) | (idx + 1 >= NF - 1)
    o = 1
    while o < NF:
        v = torch.where(h, v, torch.minimum(v, shift(v, o, float("inf"))))
        h = h | shift(h, o, True)
        o *= 2
    nuc = cand & (v * dipr <= P)
    p, q = nearest(snd)
    inner = ~snd & (p >= 0) & (q < NF)
    ends = inner & shift(snd, 1, False)
    plen = torch.where(ends, idx - p, torch.zeros_like(idx))           # (the run's length, at its last frame)
    count = torch.stack([torch.full((B,), NF, device=x.device), snd.sum(1), ends.sum(1), inner.sum(1), cand.sum(1), nuc.sum(1),
                         (~snd & (p < 0)).sum(1), (~snd & (q >= NF) & (p >= 0)).sum(1)], 1).to(torch.int32)
    n, S1, S2 = ends.sum(1).double(), plen.sum(1).double(), (plen * plen).sum(1).double()
    one = torch.ones_like(n)
    stat = torch.stack([ref, thr, torch.where(n > 0, S1 / torch.maximum(n, one), 0 * n),
                        torch.where(n > 0, torch.sqrt(n * S2 - S1 * S1) / torch.maximum(n, one), 0 * n)], 1)
    mark = (snd * 1 + raw * 2 + cand * 4 + nuc * 8).to(torch.uint8)
    return P, mark, stat, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "speech_rate_bench.json"))
    args = ap.parse_args()
    W, H = audio.speech_rate_geometry(SR, HOP)
    win = audio.intensity_window(W)
    wd = torch.from_numpy(win).cuda()
    eng = Engine(0)
    eng.load_speech_rate(win, H)
    sil, dipr = R.ratios(PAR)
    a = (PAR["power_floor"], PAR["rank_fraction"], sil, dipr, PAR["min_pause"], PAR["min_sound"])
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "window": W, "hop": H, "parameters": PAR,
           "timing": "HIP events, the variants alternating round by round (median over rounds, min / max beside it)", "shapes": {}}
    for B, L in SHAPES:
        x = torch.from_numpy(make(B, L)).cuda()
        variants = {"ev_speech_rate": lambda: eng.speech_rate(x, None, None, *a),
                    "ev_speech_rate_counts_only": lambda: eng.speech_rate(x, None, None, *a, want_power=False, want_mark=False),
                    "copy_of_the_input": lambda: x.clone(), "torch_restatement": lambda: torch_speech_rate(x, wd, PAR)}
        ev = {k: bench_timing.stats(ms, args.inner) for k, ms in bench_timing.rounds_of(variants, args.rounds, args.inner, warmup=2).items()}
        n0 = eng.alloc_count()
        power, mark, stat, count = eng.speech_rate(x, None, None, *a)
        lean = eng.speech_rate(x, None, None, *a, want_power=False, want_mark=False)
        tp, tm, ts, tc = torch_speech_rate(x, wd, PAR)
        torch.cuda.synchronize()
        k_ms = ev["ev_speech_rate"]["median_ms"]
        shape = {"rows": B, "samples_per_row": L, "seconds_per_row": L / SR, "frames_per_row": L // H, "events": ev,
                 "samples_per_us": B * L / (k_ms * 1e3), "input_gb_per_s": B * L * 4 / (k_ms * 1e6),
                 "torch_over_ev_speech_rate": ev["torch_restatement"]["median_ms"] / k_ms, "allocations_in_a_repeated_call": eng.alloc_count() - n0,
                 "counts_only_equal": bool(torch.equal(lean[2], stat) and torch.equal(lean[3], count)),
                 "marks_equal_to_torch": bool(torch.equal(tm, mark)), "counts_equal_to_torch": bool(torch.equal(tc, count)),
                 "worst_power_error_against_torch": R.rel_err(power.cpu().numpy(), tp.cpu().numpy()),
                 "worst_stat_error_against_torch": R.rel_err(stat.cpu().numpy(), ts.cpu().numpy()), "count_row_0": count[0].tolist()}
        if L <= 517 * HOP:
            ref = R.speech_rate(x[:4].cpu().numpy(), None, win, H, PAR)
            shape["first_rows_against_numpy"] = {"marks_equal": bool(np.array_equal(ref["mark"], mark[:4].cpu().numpy())),
                                                 "counts_equal": bool(np.array_equal(ref["count"], count[:4].cpu().numpy())),
                                                 "power_bit_equal": bool(np.array_equal(ref["power"], power[:4].cpu().numpy())),
                                                 "least_margin": float(ref["margin"].min())}
        res["shapes"][f"{B}x{L / SR:.0f}s"] = shape
        print(f"{B} x {L / SR:.1f} s: ev_speech_rate {k_ms:.3f} ms ({ev['ev_speech_rate']['min_ms']:.3f} .. {ev['ev_speech_rate']['max_ms']:.3f}), counts only "
              f"{ev['ev_speech_rate_counts_only']['median_ms']:.3f} ms, copy {ev['copy_of_the_input']['median_ms']:.3f} ms, torch restatement "
              f"{ev['torch_restatement']['median_ms']:.2f} ms;  {shape['samples_per_us']:.1f} samples per us;  marks / counts equal to torch "
              f"{shape['marks_equal_to_torch']} / {shape['counts_equal_to_torch']}, power {shape['worst_power_error_against_torch']:.1e}  "
              f"{shape.get('first_rows_against_numpy', '')}")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
