#!/usr/bin/env python3
"""Time ev_auditory at (n_fft, hop, win) = (1024, 256, 1024) with 26 mel bands and 4 cepstra on 64 x 6 s and 1 x 6 s of 22050 Hz audio, with and
without d_bands, beside four yardsticks on the same rows and frames:
  * ev_harmonics and ev_voice_quality at the same resolution: their first matrix product is the one ev_auditory runs (ev_auditory runs it on
    tiles of 15 new frames instead of 16: 16 / 15 of the work), ev_voice_quality's second one is far larger than ev_auditory's;
  * a batched torch restatement of the definition on the device (float64: unfold, two matmuls with the windowed basis, one with the mel table);
  * a device-to-device copy of the input (the least a call could cost: it reads every sample once).

    python tools/auditory_bench.py [--rounds 30] [--inner 2] [--out profiles/auditory_bench.json]

Method: HIP events around ``inner`` back-to-back calls, after a warm-up of every variant at the shape; the variants ALTERNATE inside every round,
so what the machine does meanwhile lands on all of them alike; per variant the median, the least and the greatest per-call time over the rounds
and the spread (max - min) / median.  No time is a gate and no counter is read.  The rows are harmonic tones of 100 .. 250 Hz on a noise floor.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import auditory_ref as R  # noqa: E402
import harmonics_ref as HR  # noqa: E402
from bench_timing import rounds_of, stats, write_json  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, SECONDS = 22050, 6
NFFT, HOP, WIN, NMEL, NCEPS, NHARM = 1024, 256, 1024, 26, 4, 48
FLOOR = 1e-7


def torch_restatement(x, c, s, mel, eq, dct, compress, NF):
    """The definition in batched float64 torch ops on the device (silent frames are not zeroed: the rows have none)."""
    pad = torch.nn.functional.pad(x.to(torch.float64), (WIN // 2 - HOP // 2, WIN))
    fm = pad.unfold(1, WIN, HOP)[:, :NF]
    re, sm = fm @ c, fm @ s
    raw = sm * sm + re * re
    ef = (raw @ mel).clamp(min=FLOOR)
    loud = ((eq * ef) ** compress).sum(dim=-1)
    mfcc = torch.log(ef) @ dct
    mag = torch.sqrt(raw)
    d = mag[:, 1:] - mag[:, :-1]
    flux = torch.cat([torch.zeros_like(loud[:, :1]), torch.sqrt((d * d).mean(dim=-1))], dim=1)
    power = raw.sum(dim=-1)
    return torch.stack([loud, flux, power, torch.log(power.clamp(min=FLOOR))], dim=-1), mfcc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "auditory_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    L = SECONDS * SR
    NB, NF = NFFT // 2 + 1, -(-L // HOP)
    NBp = (NB + 3) // 4 * 4
    t = audio.auditory_tables(SR, NFFT, NMEL, n_ceps=NCEPS)
    vt = audio.voice_quality_tables(SR, NFFT)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "seconds": SECONDS, "samples": L, "n_fft": NFFT, "hop": HOP, "win": WIN,
           "n_mels": NMEL, "n_ceps": NCEPS, "power_floor": FLOOR, "method": "HIP events around calls_per_round back-to-back calls; the variants "
           "alternate inside every round; spread = (max - min) / median over the rounds; no counter was read", "shapes": {}}
    au, hm, vq = Engine(0), Engine(0), Engine(0)
    win, tw = audio.stft_dist_window(WIN), audio.stoi_twiddle(NFFT)
    au.load_auditory(win, tw, HOP, NFFT, t["mel_w"], t["eq"], t["dct"], t["k_lo"], t["k_hi"], t["compress"])
    hm.load_harmonics(win, tw, HOP, NFFT, SR, NHARM)
    vq.load_voice_quality(win, tw, HOP, NFFT, vt["bands"], vt["slope_w"], vt["q_fit"], vt["q_min"], vt["q_max"], vt["fit_w"], vt["q_mean"])
    c, s = (torch.from_numpy(a).cuda() for a in R.basis(NFFT, WIN, win, tw))
    mel, eq, dct = (torch.from_numpy(np.ascontiguousarray(t[k])).cuda() for k in ("mel_w", "eq", "dct"))
    rng = np.random.default_rng(0)
    for B in (64, 1):
        f0 = rng.uniform(100.0, 250.0, B)
        x_h = np.stack([HR.tone_row(L, SR / f0[b], SR, seed=b, noise=1e-3) for b in range(B)])
        per_h = np.repeat((SR / f0).astype(np.float32)[:, None], NF, axis=1)
        x, per = torch.from_numpy(x_h).cuda(), torch.from_numpy(per_h).cuda()
        frame = torch.empty(B, NF, 4, dtype=torch.float64, device="cuda")
        mfcc = torch.empty(B, NF, NCEPS, dtype=torch.float64, device="cuda")
        flags = torch.empty(B, NF, dtype=torch.int32, device="cuda")
        bands = torch.empty(B, NF, NMEL, dtype=torch.float64, device="cuda")
        hframe = torch.empty(B, NF, 8, dtype=torch.float64, device="cuda")
        hcount = torch.empty(B, NF, 2, dtype=torch.int32, device="cuda")
        vframe = torch.empty(B, NF, 8, dtype=torch.float64, device="cuda")
        peak = torch.empty(B, NF, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(x)

        def call_au(with_bands=False):
            rc = au.lib.ev_auditory(au.h, x.data_ptr(), None, B, L, FLOOR, frame.data_ptr(), mfcc.data_ptr(), flags.data_ptr(),
                                    bands.data_ptr() if with_bands else None, _stream_ptr())
            assert rc == 0, au.lib.ev_last_error(au.h).decode()

        def call_hm():
            rc = hm.lib.ev_harmonics(hm.h, x.data_ptr(), None, B, L, per.data_ptr(), None, None, 0, FLOOR, hframe.data_ptr(), hcount.data_ptr(), None,
                                     _stream_ptr())
            assert rc == 0, hm.lib.ev_last_error(hm.h).decode()

        def call_vq():
            rc = vq.lib.ev_voice_quality(vq.h, x.data_ptr(), None, B, L, FLOOR, vframe.data_ptr(), peak.data_ptr(), None, _stream_ptr())
            assert rc == 0, vq.lib.ev_last_error(vq.h).decode()

        variants = {"ev_auditory": call_au, "ev_auditory_with_d_bands": lambda: call_au(True), "ev_harmonics_without_formants_and_d_harm": call_hm,
                    "ev_voice_quality": call_vq, "torch_restatement_on_the_device": lambda: torch_restatement(x, c, s, mel, eq, dct, t["compress"], NF),
                    "device_to_device_copy_of_the_input": lambda: dst.copy_(x)}
        ms = {k: stats(v, args.inner) for k, v in rounds_of(variants, args.rounds, args.inner).items()}
        call_au()
        torch.cuda.synchronize()
        tf, tm = torch_restatement(x, c, s, mel, eq, dct, t["compress"], NF)
        live = ((flags & 1) != 0).cpu().numpy()
        diff = max(R.err(frame.cpu().numpy()[live], tf.cpu().numpy()[live]), R.err(mfcc.cpu().numpy()[live], tm.cpu().numpy()[live]))
        a, h, v = ms["ev_auditory"], ms["ev_harmonics_without_formants_and_d_harm"], ms["ev_voice_quality"]
        tiles = B * -(-NF // 15)
        fma1, fma2 = tiles * 16 * WIN * NB * 2, tiles * 16 * NBp * 32
        shape = {"rows": B, "frames_per_row": NF, "bins": NB, "workgroups": tiles, "workgroups_of_the_16_frame_kernels": B * -(-NF // 16),
                 "fmas_first_product_with_the_carried_row": fma1, "fmas_second_product_padded_to_32_bands": fma2, **ms,
                 "float64_tflops_of_both_products": 2.0 * (fma1 + fma2) / (a["median_ms"] * 1e-3) / 1e12,
                 "auditory_over_harmonics": a["median_ms"] / h["median_ms"], "auditory_over_voice_quality": a["median_ms"] / v["median_ms"],
                 "auditory_over_copy": a["median_ms"] / ms["device_to_device_copy_of_the_input"]["median_ms"],
                 "torch_restatement_over_auditory": ms["torch_restatement_on_the_device"]["median_ms"] / a["median_ms"],
                 "live_frames": int(live.sum()), "frames": int(live.size), "worst_error_device_against_the_torch_restatement_on_live_frames": diff,
                 "audio_seconds_per_second": B * SECONDS / (a["median_ms"] * 1e-3)}
        res["shapes"][f"B{B}_{SECONDS}s"] = shape
        print(f"B={B} {NFFT}/{HOP}/{WIN} {NMEL} bands: " + "  ".join(f"{k} {q['median_ms']:.4f} ms (min {q['min_ms']:.4f}, max {q['max_ms']:.4f}, spread "
              f"{100 * q['spread']:.1f} %)" for k, q in ms.items()) + f"  auditory / harmonics {shape['auditory_over_harmonics']:.3f} (16 / 15 = 1.067)  "
              f"{shape['float64_tflops_of_both_products']:.2f} float64 TFLOP/s  device against torch {diff:.2e} on {int(live.sum())} of {live.size} frames")
        del x, dst
    for e in (au, hm, vq):
        e.close()
    write_json(args.out, res)


if __name__ == "__main__":
    main()
