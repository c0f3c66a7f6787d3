#!/usr/bin/env python3
"""Time ev_perturbation at audio.perturbation's default geometry (22050 Hz, hop 256, corr_length 1024, n_cycles 3, at ev_pitch_yin's own lags) on
64 x 6 s and 1 x 6 s of audio (HIP events, median of N calls after warm-up), beside three yardsticks on the same rows and frames:
  * a device-to-device copy of the input (the least a call could cost: it reads every sample once);
  * the ev_pitch_yin call (1024, 256, lags 36 .. 340) that supplies the lags;
  * one ev_formants call at (W 1024, H 256, order 13): the same one-wavefront-per-frame shape with far more arithmetic per frame.

    python tools/perturbation_bench.py [--calls 30] [--out profiles/perturbation_bench.json]

The call is latency-bound, not arithmetic: per voiced frame one search over a period and up to 2 n_cycles searches over a quarter of it, each a
strided read and a 6-step reduction that the next search depends on, then 7 sums over corr_length samples.  Nothing here is a gate: the figures
are what was seen.  The B = 1 row is also compared with the numpy restatement (tests/perturbation_ref.py): marks and counts equal, worst error.
"""
import argparse
import functools
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench_timing  # noqa: E402
import perturbation_ref as R  # noqa: E402
import stoi_ref  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, SECONDS = 22050, 6
W, H, NC, PF, AF = 1024, 256, 3, 1.3, 1.6
TAU_MIN, TAU_MAX = 36, 340
FM_ORDER = 13
FLOOR = audio.PERTURBATION_POWER_FLOOR
timed = functools.partial(bench_timing.timed, warmup=3, host_clock=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "perturbation_bench.json"))
    args = ap.parse_args()
    L = SECONDS * SR
    F = -(-L // H)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "seconds": SECONDS, "samples": L, "hop_length": H, "corr_length": W,
           "n_cycles": NC, "period_factor": PF, "amplitude_factor": AF, "power_floor": FLOOR, "lags": [TAU_MIN, TAU_MAX],
           "formants_geometry": [W, H, FM_ORDER], "shapes": {}}
    eng, fe = Engine(0), Engine(0)
    fe.load_formants(audio.formant_window(W), H, FM_ORDER, float(np.exp(-2.0 * np.pi * 50.0 / SR)), float(SR), 50.0, 4)
    for B in (64, 1):
        x_h = np.stack([stoi_ref.speech_like(L, seed=1 + b, fs=SR, f0=100.0 + 7.0 * (b % 16)) for b in range(B)])
        x = torch.from_numpy(x_h).cuda()
        lag = torch.empty(B, F, dtype=torch.int32, device="cuda")
        frame = torch.empty(B, F, 8, dtype=torch.float64, device="cuda")
        count = torch.empty(B, F, 4, dtype=torch.int32, device="cuda")
        marks = torch.empty(B, F, 2 * NC + 1, dtype=torch.int32, device="cuda")
        lpc = torch.empty(B, F, FM_ORDER + 2, dtype=torch.float64, device="cuda")
        fm = torch.empty(B, F, 4, 2, dtype=torch.float64, device="cuda")
        fct = torch.empty(B, F, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(x)

        def call_yin():
            rc = eng.lib.ev_pitch_yin(eng.h, x.data_ptr(), None, B, L, W, H, TAU_MIN, TAU_MAX, 0.1, lag.data_ptr(), None, None, _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        def call_pt():
            rc = eng.lib.ev_perturbation(eng.h, x.data_ptr(), None, B, L, H, lag.data_ptr(), NC, W, PF, AF, FLOOR, frame.data_ptr(), count.data_ptr(),
                                         marks.data_ptr(), _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        def call_fm():
            rc = fe.lib.ev_formants(fe.h, x.data_ptr(), None, B, L, audio.FORMANT_POWER_FLOOR, lpc.data_ptr(), fm.data_ptr(), fct.data_ptr(), _stream_ptr())
            assert rc == 0, fe.lib.ev_last_error(fe.h).decode()

        ty = timed(call_yin, args.calls)
        tp, tf, tcp = timed(call_pt, args.calls), timed(call_fm, args.calls), timed(lambda: dst.copy_(x), args.calls)
        lg, ct = lag.cpu().numpy(), count.cpu().numpy()
        voiced = int((lg > 0).sum())
        shape = {"rows": B, "frames_per_row": F, "wavefronts": B * F, "workgroups": B * -(-F // 4), "ev_perturbation": tp, "ev_pitch_yin_same_frames": ty,
                 "ev_formants_same_frames": tf, "device_to_device_copy_of_the_input": tcp, "perturbation_over_formants": tp["median_ms"] / tf["median_ms"],
                 "perturbation_over_pitch_yin": tp["median_ms"] / ty["median_ms"], "perturbation_over_copy": tp["median_ms"] / tcp["median_ms"],
                 "voiced_frames": voiced, "frames": int(lg.size), "frames_with_all_periods": int((ct[..., 0] == 2 * NC).sum()),
                 "periods_found": int(ct[..., 0].sum()), "audio_seconds_per_second": B * SECONDS / (tp["median_ms"] * 1e-3)}
        if B == 1:
            ref = R.batch(x_h, None, lg, R.geo(H, W, NC, PF, AF, FLOOR))
            shape["marks_equal_to_the_restatement"] = bool(np.array_equal(marks.cpu().numpy(), ref["marks"]))
            shape["counts_equal_to_the_restatement"] = bool(np.array_equal(ct, ref["count"]))
            shape["worst_error_d_frame"] = R.err(frame.cpu().numpy(), ref["frame"])
        res["shapes"][f"B{B}_{SECONDS}s"] = shape
        print(f"B={B} {SR} Hz hop {H} corr {W} n_cycles {NC}: ev_perturbation {tp['median_ms']:.3f} ms (min {tp['min_ms']:.3f}, max {tp['max_ms']:.3f})  "
              f"ev_pitch_yin {ty['median_ms']:.3f} ms  ev_formants {tf['median_ms']:.3f} ms  copy {tcp['median_ms']:.4f} ms  {shape['workgroups']} workgroups  "
              f"{voiced} of {lg.size} frames voiced, {shape['frames_with_all_periods']} with all {2 * NC} periods"
              + (f"  against the restatement: marks equal {shape['marks_equal_to_the_restatement']}, counts equal "
                 f"{shape['counts_equal_to_the_restatement']}, d_frame {shape['worst_error_d_frame']:.2e}" if B == 1 else ""))
        del x, dst
    eng.close()
    fe.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
