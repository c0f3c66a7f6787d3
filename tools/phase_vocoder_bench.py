#!/usr/bin/env python3
"""Time ev_phase_vocoder on 64 x 6 s and 1 x 6 s of 22.05 kHz audio at nfft 1024 (hop 256), at rates 0.8 and 1.25, beside
  * ev_stft_dist at (1024, 256, 1024) on the same rows: two forward DFTs of this size, the natural yardstick for one forward DFT plus
    16 / 13 / rate inverse ones (a workgroup of pv_synthesis_kernel computes 16 frames for the 13 hop segments it owns);
  * ``torch_stretch``: a batched float64 torch restatement on the device (torch.stft, the propagation vectorised over bins and frames, the phase
    by a cumulative sum, torch.istft);
  * a device-to-device copy of the input.
The variants take turns, round by round, under HIP events (bench_timing.rounds_of): medians with min / max.

    python tools/phase_vocoder_bench.py [--rounds 10] [--inner 2] [--out profiles/phase_vocoder_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/phase_vocoder_bench.py --trace_pass     # a run of its own
    python tools/phase_vocoder_bench.py --kernel_trace DIR [--out ...]                                          # adds "launches" to the JSON

The three launches of a call cannot be told apart by events around the call, so their split comes from a kernel trace taken in a run of its own
(--trace_pass issues one warm-up and five calls per shape and rate, nothing else on the phase vocoder's kernels); --kernel_trace reads the
trace (no GPU needed) and stores the median of each kernel per shape and rate over the five calls behind the warm-up.  Nothing here is a gate and no ratio is promised: the figures are what
was seen.  Every shape is compared with the torch form (worst |y - y_torch| over the peak).
"""
import argparse
import collections
import csv
import glob
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench_timing  # noqa: E402

SR, SECONDS, NFFT = 22050, 6, 1024
HOP, NB = NFFT // 4, NFFT // 2 + 1
L = SECONDS * SR
SHAPES, RATES = (64, 1), (0.8, 1.25)
KERNELS = ("pv_analysis_kernel", "pv_propagate_kernel", "pv_synthesis_kernel")
TRACE_CALLS = 5


def make(B):
    import phase_vocoder_ref as R
    return torch.from_numpy(np.stack([R.speech_like(L, 400 + b) for b in range(B)]))


def torch_stretch(x, rate):
    """The definition for full rows by batched float64 torch ops on the device."""
    w = torch.hann_window(NFFT, periodic=True, dtype=torch.float64, device=x.device)
    D = torch.stft(x.to(torch.float64), NFFT, hop_length=HOP, window=w, center=True, pad_mode="constant", return_complex=True)   # (B, NB, nf)
    nf = D.shape[-1]
    n_out = int(math.ceil(nf / rate))
    D = torch.nn.functional.pad(D, (0, 2))
    mag, ang = D.abs(), D.angle()
    s = torch.arange(n_out, dtype=torch.float64) * rate
    i = torch.floor(s).to(torch.int64)
    a = (s - torch.floor(s)).to(x.device)
    i = i.to(x.device)
    m = (1.0 - a) * mag[..., i] + a * mag[..., i + 1]
    omega = (2.0 * math.pi * HOP * torch.arange(NB, dtype=torch.float64, device=x.device) / NFFT)[None, :, None]
    d = ang[..., i + 1] - ang[..., i] - omega
    d = d - 2.0 * math.pi * torch.round(d / (2.0 * math.pi))
    phi = torch.cumsum(torch.cat([ang[..., :1], (omega + d)[..., :-1]], dim=-1), dim=-1)
    Y = torch.polar(m, phi)
    return torch.istft(Y, NFFT, hop_length=HOP, window=w, center=True, length=int(round(x.shape[1] / rate))).to(torch.float32)


def trace_dispatches(folder):
    """{(kernel, workgroups along x, along y): microseconds of every dispatch, in dispatch order} of the phase vocoder's kernels in a rocprofv3
    kernel trace."""
    kt = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    assert kt, f"no kernel trace under {folder}"
    us = collections.defaultdict(list)
    for r in sorted(csv.DictReader(open(kt[0])), key=lambda r: int(r["Dispatch_Id"])):
        name = r["Kernel_Name"].split("(")[0]
        if name in KERNELS:
            wg = int(r["Workgroup_Size_X"]) if "Workgroup_Size_X" in r else 1
            us[(name, int(r["Grid_Size_X"]) // max(wg, 1), int(r["Grid_Size_Y"]))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return us


def launch_grids(B, rate):
    NF = 1 + L // HOP
    NO = int(math.ceil(NF / rate))
    return {"pv_analysis_kernel": ((NF + 15) // 16, B), "pv_propagate_kernel": ((NB + 63) // 64, B), "pv_synthesis_kernel": ((NO + 15) // 13, B)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--trace_pass", action="store_true")
    ap.add_argument("--kernel_trace", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "phase_vocoder_bench.json"))
    args = ap.parse_args()
    if args.kernel_trace:
        us = trace_dispatches(args.kernel_trace)
        res = json.load(open(args.out))
        for B in SHAPES:
            for ri, rate in enumerate(RATES):
                split = {}
                for k, (gx, gy) in launch_grids(B, rate).items():
                    # the analysis and propagation grids do not depend on the rate: the rates then share a key and took turns in the order of RATES,
                    # 1 + TRACE_CALLS dispatches each; the first of each is the warm-up and is left out
                    same = [r for r in RATES if launch_grids(B, r)[k] == (gx, gy)]
                    v = us.get((k, gx, gy), [])
                    n = 1 + TRACE_CALLS
                    mine = v[same.index(rate) * n: (same.index(rate) + 1) * n][1:] if len(v) == n * len(same) else []
                    split[k] = {"median_us": statistics.median(mine), "dispatches": len(mine), "workgroups": gx * gy} if mine else None
                    print(f"B={B} rate {rate}: {k} {gx} x {gy} workgroups: " + (f"{statistics.median(mine):.1f} us (median of {len(mine)})" if mine else "not in the trace"))
                res["shapes"][f"B{B}_{SECONDS}s"]["rates"][str(rate)]["launches"] = split
        bench_timing.write_json(args.out, res)
        return
    from emojivoice_amd import audio
    from emojivoice_amd._lib import Engine

    eng, dist = Engine(0), Engine(0)
    eng.load_phase_vocoder(audio.phase_vocoder_window(NFFT), audio.stoi_twiddle(NFFT), NFFT)
    dist.load_stft_dist(audio.stft_dist_window(NFFT), audio.stoi_twiddle(NFFT), HOP, NFFT)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "seconds": SECONDS, "samples": L, "nfft": NFFT, "hop": HOP, "shapes": {}}
    for B in SHAPES:
        x = make(B).cuda()
        shape = {"rows": B, "rates": {}}
        for rate in RATES:
            if args.trace_pass:
                for _ in range(1 + TRACE_CALLS):
                    eng.phase_vocoder(x, None, rate)
                torch.cuda.synchronize()
                continue
            y, out_len, _, _ = eng.phase_vocoder(x, None, rate)
            yt = torch_stretch(x, rate)
            diff = float((y - yt).abs().max() / yt.abs().max())
            n0 = eng.alloc_count()
            buf = torch.empty_like(x)
            variants = {"ev_phase_vocoder": lambda: eng.phase_vocoder(x, None, rate), "ev_stft_dist": lambda: dist.stft_dist(x, x, None, audio.MSTFT_POWER_FLOOR),
                        "torch_restatement": lambda: torch_stretch(x, rate), "copy": lambda: buf.copy_(x)}
            ev = {k: bench_timing.stats(v, args.inner) for k, v in bench_timing.rounds_of(variants, args.rounds, args.inner).items()}
            k_ms = ev["ev_phase_vocoder"]["median_ms"]
            NF = 1 + L // HOP
            NO = int(math.ceil(NF / rate))
            fwd, inv = B * NF * NFFT * NB * 2, B * ((NO + 15) // 13) * 16 * NFFT * NB * 2
            shape["rates"][str(rate)] = {
                "frames_in": NF, "frames_out": NO, "samples_out": int(out_len[0]), "events": ev, "fmas_forward": fwd, "fmas_inverse_as_launched": inv,
                "float64_tflops_as_launched": 2.0 * (fwd + inv) / (k_ms * 1e-3) / 1e12, "scratch_bytes": audio.phase_vocoder_scratch_bytes(B, L, rate, NFFT),
                "stft_dist_over_ev_phase_vocoder": ev["ev_stft_dist"]["median_ms"] / k_ms, "torch_over_ev_phase_vocoder": ev["torch_restatement"]["median_ms"] / k_ms,
                "audio_seconds_per_second": B * SECONDS / (k_ms * 1e-3), "allocations_in_the_repeated_calls": eng.alloc_count() - n0,
                "worst_difference_against_torch_over_peak": diff}
            print(f"{B} x {SECONDS} s at rate {rate}: ev_phase_vocoder {k_ms:.3f} ms ({ev['ev_phase_vocoder']['min_ms']:.3f} .. {ev['ev_phase_vocoder']['max_ms']:.3f}), "
                  f"ev_stft_dist {ev['ev_stft_dist']['median_ms']:.3f} ms, torch {ev['torch_restatement']['median_ms']:.3f} ms, copy {ev['copy']['median_ms']:.4f} ms; "
                  f"{2.0 * (fwd + inv) / (k_ms * 1e-3) / 1e12:.2f} float64 TFLOP/s as launched; against torch {diff:.2e} of the peak")
        res["shapes"][f"B{B}_{SECONDS}s"] = shape
        del x
    eng.close()
    dist.close()
    if not args.trace_pass:
        bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
