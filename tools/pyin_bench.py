#!/usr/bin/env python3
"""Time ev_pyin_observe, ev_pyin_decode and audio.pitch_pyin beside ev_pitch_yin on the same input (HIP events, median of N calls after warm-up).

    python tools/pyin_bench.py [--calls 20] [--out profiles/pyin_bench.json]

Shapes: 6 s at 22.05 kHz (132 300 samples), B = 64 and B = 1, the defaults of audio.pitch_pyin (frame 1024, hop 256, lags 36 .. 340,
100 thresholds under Beta(2, 18), 385 bins of a tenth of a semitone, R = 25): 517 frames per row.  The input is tools/pitch_bench.py's: a
3-harmonic tone per row under noise.  observe does ev_pitch_yin's W (tau_max + 1) float64 fmas per frame and then two sweeps of n_thr
ballots per 64 troughs; decode is one workgroup per row, 2 n_bins states x 2 (2 R + 1) add-compares per frame behind one barrier, then
F dependent byte loads of one lane: it is latency-bound and does not shrink with the batch.  audio.pitch_pyin adds the host tables, the
torch allocations and the conversion of the states into Hz.  None of the figures is a gate.
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
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine  # noqa: E402

SR, W, H, FMIN, FMAX = 22050, 1024, 256, 65.0, 600.0
timed = functools.partial(bench_timing.timed, warmup=5, host_clock=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pyin_bench.json"))
    args = ap.parse_args()
    tau_min, tau_max = audio.pitch_lag_range(SR, FMIN, FMAX)
    bpo, n_bins = audio.pyin_bins(FMIN, FMAX, 0.1)
    R = audio.pyin_transition_radius(SR, H, bpo)
    w = audio.pyin_threshold_prior()
    tables = audio.pyin_transition(n_bins, R, 0.01)
    res = {"device": torch.cuda.get_device_name(0), "frame_length": W, "hop_length": H, "tau_min": tau_min, "tau_max": tau_max, "n_thresholds": 100,
           "n_bins": n_bins, "R": R, "shapes": {}}
    g = torch.Generator().manual_seed(0)
    L = 6 * SR
    F = -(-L // H)
    eng = Engine(0)
    for B in (64, 1):
        t = torch.arange(L, dtype=torch.float64) / SR
        f0 = 90.0 + 4.0 * torch.arange(B, dtype=torch.float64)[:, None]                       # 90 .. 342 Hz, one per row
        x = sum(a * torch.sin(2 * math.pi * f0 * k * t) for k, a in ((1, 0.3), (2, 0.15), (3, 0.075)))
        x = (x + 0.01 * torch.randn(B, L, generator=g, dtype=torch.float64)).float().cuda()
        obs = torch.empty(B, F, n_bins, dtype=torch.float64, device="cuda")
        pv = torch.empty(B, F, dtype=torch.float64, device="cuda")
        back = torch.empty(B, F, 2 * n_bins, dtype=torch.uint8, device="cuda")
        observe = lambda: eng.pyin_observe(x, None, W, H, tau_min, tau_max, SR, FMIN, bpo, n_bins, w, 2.0, 0.01, out=(obs, pv))
        decode = lambda: eng.pyin_decode(obs, pv, None, L, H, R, *tables, back=back)
        observe()
        state, _ = decode()
        torch.cuda.synchronize()
        voiced = int(((state >= 0) & (state < n_bins)).sum())
        t_yin = timed(lambda: eng.pitch_yin(x, None, W, H, tau_min, tau_max, 0.1), args.calls)
        t_obs = timed(observe, args.calls)
        t_dec = timed(decode, args.calls)
        t_all = timed(lambda: audio.pitch_pyin(x, SR), args.calls)
        yin = t_yin["median_ms"]
        res["shapes"][f"B{B}_L{L}"] = {
            "frames": B * F, "voiced_frames": voiced, "obs_bytes": obs.numel() * 8, "back_bytes": back.numel(), "ev_pitch_yin": t_yin,
            "ev_pyin_observe": t_obs, "ev_pyin_decode": t_dec, "audio_pitch_pyin": t_all,
            "observe_over_yin": t_obs["median_ms"] / yin, "decode_over_yin": t_dec["median_ms"] / yin, "pitch_pyin_over_yin": t_all["median_ms"] / yin,
            "decode_over_observe": t_dec["median_ms"] / t_obs["median_ms"],
            "audio_seconds_per_second": B * L / SR / (t_all["median_ms"] * 1e-3)}
        print(f"B={B} L={L}: ev_pitch_yin {yin:.4f} ms  observe {t_obs['median_ms']:.4f} ms ({t_obs['median_ms'] / yin:.2f} x)  "
              f"decode {t_dec['median_ms']:.4f} ms ({t_dec['median_ms'] / yin:.2f} x)  audio.pitch_pyin {t_all['median_ms']:.4f} ms "
              f"({t_all['median_ms'] / yin:.2f} x)  ({B * F} frames, {voiced} voiced)")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
