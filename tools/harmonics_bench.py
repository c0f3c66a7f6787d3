#!/usr/bin/env python3
"""Time ev_harmonics at (n_fft, hop, win) = (1024, 256, 1024), n_harm 48, on 64 x 6 s and 1 x 6 s of 22050 Hz audio, with and without the
formant terms, beside four yardsticks on the same rows and frames:
  * ev_voice_quality at the same resolution: its first matrix product is the one ev_harmonics runs, and it runs a second one that ev_harmonics
    does not, so it is the figure to compare with;
  * ev_stft_dist at the same resolution (the same product for two signals);
  * a device-to-device copy of the input (the least a call could cost: it reads every sample once);
  * the numpy restatement of the definition (tests/harmonics_ref.py) on 16 CPU threads.

    python tools/harmonics_bench.py [--rounds 15] [--inner 4] [--out profiles/harmonics_bench.json]

Method: HIP events around ``inner`` back-to-back calls, after a warm-up of every variant at the shape; the variants ALTERNATE inside every round,
so what the machine does meanwhile lands on all of them alike; per variant the median, the least and the greatest per-call time over the rounds
and the spread (max - min) / median.  No time is a gate.  The rows are harmonic tones of 100 .. 250 Hz (4.6 .. 11.6 bins between harmonics) on a
noise floor, at their true periods, so the combs are as long as a voice's.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import harmonics_ref as R  # noqa: E402
from bench_timing import rounds_of, stats, write_json  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, SECONDS, CPU_THREADS = 22050, 6, 16
NFFT, HOP, WIN, NHARM = 1024, 256, 1024, 48
FLOOR = 1e-7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "harmonics_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    torch.set_num_threads(CPU_THREADS)
    L = SECONDS * SR
    NB, NF = NFFT // 2 + 1, -(-L // HOP)
    geom = R.Geometry(NFFT, HOP, WIN, SR, NHARM)
    t = audio.voice_quality_tables(SR, NFFT)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "seconds": SECONDS, "samples": L, "n_fft": NFFT, "hop": HOP, "win": WIN,
           "n_harm": NHARM, "power_floor": FLOOR, "cpu_threads": CPU_THREADS, "method": "HIP events around calls_per_round back-to-back calls; the "
           "variants alternate inside every round; spread = (max - min) / median over the rounds", "shapes": {}}
    hm, vq, sd = Engine(0), Engine(0), Engine(0)
    win, tw = audio.stft_dist_window(WIN), audio.stoi_twiddle(NFFT)
    hm.load_harmonics(win, tw, HOP, NFFT, SR, NHARM)
    vq.load_voice_quality(win, tw, HOP, NFFT, t["bands"], t["slope_w"], t["q_fit"], t["q_min"], t["q_max"], t["fit_w"], t["q_mean"])
    sd.load_stft_dist(win, tw, HOP, NFFT)
    rng = np.random.default_rng(0)
    for B in (64, 1):
        f0 = rng.uniform(100.0, 250.0, B)
        x_h = np.stack([R.tone_row(L, SR / f0[b], SR, seed=b, noise=1e-3) for b in range(B)])
        per_h = np.repeat((SR / f0).astype(np.float32)[:, None], NF, axis=1)
        fm_h = np.zeros((B, NF, 4, 2))
        fm_h[..., 0] = np.array([600.0, 1400.0, 2600.0, 3600.0]) + rng.uniform(-80.0, 80.0, (B, NF, 4))
        fm_h[..., 1] = 120.0
        fc_h = np.full((B, NF), 4, np.int32)
        x, per, fm, fc = (torch.from_numpy(a).cuda() for a in (x_h, per_h, fm_h, fc_h))
        y = x + 0.01 * torch.randn_like(x)
        frame = torch.empty(B, NF, 8, dtype=torch.float64, device="cuda")
        count = torch.empty(B, NF, 2, dtype=torch.int32, device="cuda")
        harm = torch.empty(B, NF, NHARM, 2, dtype=torch.float64, device="cuda")
        vframe = torch.empty(B, NF, 8, dtype=torch.float64, device="cuda")
        peak = torch.empty(B, NF, dtype=torch.int32, device="cuda")
        sums = torch.empty(B, 4, dtype=torch.float64, device="cuda")
        counts = torch.empty(B, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(x)

        def call_hm(with_formants=True, with_harm=True):
            rc = hm.lib.ev_harmonics(hm.h, x.data_ptr(), None, B, L, per.data_ptr(), fm.data_ptr() if with_formants else None,
                                     fc.data_ptr() if with_formants else None, 4 if with_formants else 0, FLOOR, frame.data_ptr(), count.data_ptr(),
                                     harm.data_ptr() if with_harm else None, _stream_ptr())
            assert rc == 0, hm.lib.ev_last_error(hm.h).decode()

        def call_vq():
            rc = vq.lib.ev_voice_quality(vq.h, x.data_ptr(), None, B, L, FLOOR, vframe.data_ptr(), peak.data_ptr(), None, _stream_ptr())
            assert rc == 0, vq.lib.ev_last_error(vq.h).decode()

        def call_sd():
            rc = sd.lib.ev_stft_dist(sd.h, x.data_ptr(), y.data_ptr(), None, B, L, FLOOR, None, sums.data_ptr(), counts.data_ptr(), _stream_ptr())
            assert rc == 0, sd.lib.ev_last_error(sd.h).decode()

        variants = {"ev_harmonics": call_hm, "ev_harmonics_without_formants": lambda: call_hm(False),
                    "ev_harmonics_without_d_harm": lambda: call_hm(True, False), "ev_voice_quality": call_vq,
                    "ev_stft_dist_same_resolution_two_signals": call_sd, "device_to_device_copy_of_the_input": lambda: dst.copy_(x)}
        ms = {k: stats(v, args.inner) for k, v in rounds_of(variants, args.rounds, args.inner).items()}
        call_hm()
        torch.cuda.synchronize()
        R.batch(x_h[:1], None, per_h[:1], geom, fm_h[:1], fc_h[:1], floor=FLOOR)     # (warm-up: the tables and the BLAS threads)
        t0 = time.perf_counter()
        ref = R.batch(x_h, None, per_h, geom, fm_h, fc_h, floor=FLOOR)
        cpu = (time.perf_counter() - t0) * 1e3
        df, dc, dh = frame.cpu().numpy(), count.cpu().numpy(), harm.cpu().numpy()
        same = (dc == ref["count"]).all(axis=-1)
        diff = max(R.err(df[same], ref["frame"][same]), R.err(dh[same], ref["harm"][same]))
        h, v = ms["ev_harmonics"], ms["ev_voice_quality"]
        fma1 = B * NF * WIN * NB * 2
        shape = {"rows": B, "frames_per_row": NF, "bins": NB, "workgroups": B * -(-NF // 16), "useful_fmas_matrix_product": fma1,
                 "harmonics_searched": int(ref["count"][..., 0].sum()), **ms,
                 "useful_float64_tflops": 2.0 * fma1 / (h["median_ms"] * 1e-3) / 1e12,
                 "harmonics_over_voice_quality": h["median_ms"] / v["median_ms"],
                 "harmonics_over_copy": h["median_ms"] / ms["device_to_device_copy_of_the_input"]["median_ms"],
                 "numpy_restatement_cpu_ms": cpu, "cpu_over_device": cpu / h["median_ms"],
                 "frames_with_equal_counts": int(same.sum()), "frames": int(same.size), "worst_error_device_against_cpu_on_those": diff,
                 "audio_seconds_per_second": B * SECONDS / (h["median_ms"] * 1e-3)}
        res["shapes"][f"B{B}_{SECONDS}s"] = shape
        print(f"B={B} {NFFT}/{HOP}/{WIN} n_harm {NHARM}: " + "  ".join(f"{k} {s['median_ms']:.4f} ms (min {s['min_ms']:.4f}, max {s['max_ms']:.4f}, spread "
              f"{100 * s['spread']:.1f} %)" for k, s in ms.items()) + f"  numpy on {CPU_THREADS} threads {cpu:.1f} ms ({cpu / h['median_ms']:.0f} x)  "
              f"{shape['useful_float64_tflops']:.2f} useful float64 TFLOP/s  device against CPU {diff:.2e} on {int(same.sum())} of {same.size} frames "
              f"with equal counts")
        del x, y, dst
    for e in (hm, vq, sd):
        e.close()
    write_json(args.out, res)


if __name__ == "__main__":
    main()
