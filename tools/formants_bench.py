#!/usr/bin/env python3
"""Time ev_formants at audio.formants' default geometry (11025 Hz, W 512, H 128, order 13, four formants) on 64 x 6 s and 1 x 6 s of audio (HIP
events, median of N calls after warm-up), beside three yardsticks on the same rows:
  * a device-to-device copy of the input (the least a call could cost: it reads every sample once);
  * one ev_voice_quality call at (1024, 128, 1024) on the same rows: the same number of frames, two float64 matrix products per frame against
    two short recursions;
  * the numpy restatement of the definition (tests/formants_ref.py) on 16 CPU threads.

    python tools/formants_bench.py [--calls 30] [--cpu_calls 1] [--out profiles/formants_bench.json]

The call is latency-bound, not arithmetic: per frame `order` lattice steps of 2 W fmas with two wave reductions each, then per iteration of the
root finder `order` Horner steps and `order` complex reciprocals per root.  "rough_float64_flops" is that rough count, 6 W p for the lattice and
30 p^2 per iteration at an assumed 12 iterations (the restatement's mean is recorded beside it); no figure is a gate.
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
import formants_ref as R  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, SECONDS, CPU_THREADS = 11025, 6, 16
W, H, ORDER, NFORM, F_LO = 512, 128, 13, 4, 50.0
VQ_NFFT = 1024
FLOOR = audio.FORMANT_POWER_FLOOR
timed = functools.partial(bench_timing.timed, warmup=3, host_clock=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--cpu_calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "formants_bench.json"))
    args = ap.parse_args()
    torch.set_num_threads(CPU_THREADS)
    L = SECONDS * SR
    NF = -(-L // H)
    pre = float(np.exp(-2.0 * np.pi * 50.0 / SR))
    geom = R.geometry(float(SR), W, H, ORDER, NFORM, F_LO, pre)
    t = audio.voice_quality_tables(SR, VQ_NFFT)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "seconds": SECONDS, "samples": L, "W": W, "H": H, "order": ORDER,
           "n_formants": NFORM, "f_lo": F_LO, "pre_emphasis": pre, "power_floor": FLOOR, "cpu_threads": CPU_THREADS,
           "voice_quality_geometry": [VQ_NFFT, H, VQ_NFFT], "shapes": {}}
    fe, vq = Engine(0), Engine(0)
    fe.load_formants(audio.formant_window(W), H, ORDER, pre, float(SR), F_LO, NFORM)
    vq.load_voice_quality(audio.stft_dist_window(VQ_NFFT), audio.stoi_twiddle(VQ_NFFT), H, VQ_NFFT, t["bands"], t["slope_w"], t["q_fit"], t["q_min"],
                          t["q_max"], t["fit_w"], t["q_mean"])
    for B in (64, 1):
        x_h = np.stack([R.speech_like(L, seed=1 + b, fs=SR) for b in range(B)])
        x = torch.from_numpy(x_h).cuda()
        lpc = torch.empty(B, NF, ORDER + 2, dtype=torch.float64, device="cuda")
        fm = torch.empty(B, NF, NFORM, 2, dtype=torch.float64, device="cuda")
        ct = torch.empty(B, NF, dtype=torch.int32, device="cuda")
        frame = torch.empty(B, NF, 8, dtype=torch.float64, device="cuda")
        peak = torch.empty(B, NF, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(x)

        def call_fm():
            rc = fe.lib.ev_formants(fe.h, x.data_ptr(), None, B, L, FLOOR, lpc.data_ptr(), fm.data_ptr(), ct.data_ptr(), _stream_ptr())
            assert rc == 0, fe.lib.ev_last_error(fe.h).decode()

        def call_vq():
            rc = vq.lib.ev_voice_quality(vq.h, x.data_ptr(), None, B, L, 1e-7, frame.data_ptr(), peak.data_ptr(), None, _stream_ptr())
            assert rc == 0, vq.lib.ev_last_error(vq.h).decode()

        tf, tv, tcp = timed(call_fm, args.calls), timed(call_vq, args.calls), timed(lambda: dst.copy_(x), args.calls)
        cpu_ms = []
        for _ in range(args.cpu_calls + 1):                               # (the first is the warm-up)
            t0 = time.perf_counter()
            rl, rf, rc_, it, _ = R.batch(x_h, None, geom, floor=FLOOR)
            cpu_ms.append((time.perf_counter() - t0) * 1e3)
        cpu = statistics.median(cpu_ms[1:])
        dl, df, dc = lpc.cpu().numpy(), fm.cpu().numpy(), ct.cpu().numpy()
        same = dc == rc_
        e_l, e_f = R.err(dl, rl), R.err(df[same], rf[same])
        iters = float(it[it > 0].mean())
        flops = B * NF * (6.0 * W * ORDER + 12.0 * 30.0 * ORDER * ORDER)
        shape = {"rows": B, "frames_per_row": NF, "wavefronts": B * NF, "workgroups": B * -(-NF // 4), "ev_formants": tf,
                 "device_to_device_copy_of_the_input": tcp, "ev_voice_quality_same_frames": tv,
                 "formants_over_voice_quality": tf["median_ms"] / tv["median_ms"], "formants_over_copy": tf["median_ms"] / tcp["median_ms"],
                 "rough_float64_flops": flops, "rough_float64_gflops_per_s": flops / (tf["median_ms"] * 1e-3) / 1e9,
                 "numpy_restatement_cpu_ms": cpu, "cpu_over_device": cpu / tf["median_ms"], "restatement_mean_iterations": iters,
                 "restatement_max_iterations": int(it.max()), "frames_with_equal_count": int(same.sum()), "frames": int(same.size),
                 "unconverged_frames_device": int((dc < 0).sum()), "worst_error_d_lpc": e_l, "worst_error_d_formant_on_equal_counts": e_f,
                 "audio_seconds_per_second": B * SECONDS / (tf["median_ms"] * 1e-3)}
        res["shapes"][f"B{B}_{SECONDS}s"] = shape
        print(f"B={B} {SR} Hz {W}/{H}/order {ORDER}: ev_formants {tf['median_ms']:.3f} ms (min {tf['min_ms']:.3f}, max {tf['max_ms']:.3f})  ev_voice_quality "
              f"{tv['median_ms']:.3f} ms  copy {tcp['median_ms']:.4f} ms  numpy on {CPU_THREADS} threads {cpu:.1f} ms ({cpu / tf['median_ms']:.0f} x)  "
              f"{shape['workgroups']} workgroups  device against CPU: d_lpc {e_l:.2e}, d_formant {e_f:.2e} on {int(same.sum())} of {same.size} frames with "
              f"the same count; {shape['unconverged_frames_device']} unconverged; restatement iterations mean {iters:.1f} max {int(it.max())}")
        del x, dst
    fe.close()
    vq.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
