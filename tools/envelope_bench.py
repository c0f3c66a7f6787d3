#!/usr/bin/env python3
"""Time ev_envelope on 64 x 6 s and 1 x 6 s (517 frames) of 22.05 kHz audio at nfft 1024, hop 256, order 24, alpha 0.455, with and without
d_env, beside ev_voice_quality on the same rows (the neighbour with the same grid and one GEMM less) and beside ``torch_envelope``: a batched
float64 torch restatement on the device (unfolded frames under per-frame windows, rfft, gathers for the DC correction, the smoothing as WORLD's
difference of cumulative sums, irfft / rfft for the lifter, a matmul for the warp).  The variants take turns, round by round, under HIP events
(bench_timing.rounds_of): medians with min / max.

    python tools/envelope_bench.py [--rounds 10] [--inner 2] [--out profiles/envelope_bench.json]

Nothing here is a gate and no ratio is promised: the figures are what was seen.  Every shape is compared with the torch form (classes equal, worst
absolute error of Le and mcep: the cumulative-sum smoothing cancels, so it stands further off than the gate of the tests) and the first rows of
the small one with the numpy restatement (tests/envelope_ref.py).
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench_timing  # noqa: E402
import envelope_ref as R  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine  # noqa: E402

SR, HOP, NFFT, ORDER, ALPHA = 22050, 256, 1024, 24, 0.455
SHAPES = ((64, 517 * HOP), (1, 517 * HOP))                               # (rows, samples): 6.0 s, 517 frames


def make(B, L):
    """B rows of harmonic sums (100 .. 220 Hz) with noise 60 dB down and their periods per frame: a fifth of the frames unvoiced (period 0)."""
    rng = np.random.default_rng(300)
    NF = L // HOP
    x, p = np.empty((B, L), np.float32), np.empty((B, NF), np.float32)
    for b in range(B):
        T = SR / rng.uniform(100.0, 220.0)
        x[b] = R.harmonic_row(L, T, seed=301 + b)
        p[b] = np.where(rng.uniform(size=NF) < 0.2, 0.0, T * rng.uniform(0.97, 1.03, size=NF))
    return x, p


def torch_envelope(x, period, A, T_def, q1=R.Q1, floor=R.FLOOR):
    """ev_envelope's outputs for full rows by batched torch ops; x (B, L) float32 on the device with L a multiple of the hop."""
    B, L = x.shape
    NF, NB, hn = L // HOP, NFFT // 2 + 1, NFFT // 2
    p = period.to(torch.float64)
    ok = (p > 0) & (p >= 2.0) & (p <= R.t_max(NFFT))
    T = torch.where(ok, p, torch.full_like(p, T_def))[..., None]
    j = torch.arange(-hn, hn, device=x.device, dtype=torch.float64)
    S = torch.nn.functional.pad(x.to(torch.float64), (hn - HOP // 2, NFFT)).unfold(1, NFFT, HOP)[:, :NF]
    half = torch.floor(1.5 * T + 0.5)
    w = torch.where(j.abs() <= half, 0.5 * torch.cos(math.pi * j / (1.5 * T)) + 0.5, torch.zeros_like(T))
    xw = S * w
    s = (xw - w * (xw.sum(-1, keepdim=True) / w.sum(-1, keepdim=True))) / torch.sqrt((w * w).sum(-1, keepdim=True))
    X = torch.fft.rfft(s, dim=-1)
    P = X.real * X.real + X.imag * X.imag
    k = torch.arange(NB, device=x.device, dtype=torch.float64)
    rn = NFFT / T
    u = rn - k
    i0 = torch.floor(u)
    fu = u - i0
    g0 = i0.clamp(0, NB - 1).long()
    Pc = torch.where(k <= torch.floor(rn), P + (torch.gather(P, 2, g0) * (1.0 - fu) + torch.gather(P, 2, (g0 + 1).clamp(max=NB - 1)) * fu), P)
    pad = NFFT // 6 + 3
    i = torch.arange(-pad, hn + pad + 1, device=x.device)
    i = torch.where(i < 0, -i, i)
    ext = Pc[..., torch.where(i > hn, NFFT - i, i)]
    cum = torch.cat([torch.zeros_like(ext[..., :1]), torch.cumsum(ext, -1)], -1)
    wd = (2.0 * NFFT) / (3.0 * T)

    def integral(t):
        pos = t + (pad + 0.5)
        c = torch.floor(pos)
        return torch.gather(cum, 2, c.long()) + (pos - c) * torch.gather(ext, 2, c.long())

    Lg = torch.log(torch.clamp((integral(k + 0.5 * wd) - integral(k - 0.5 * wd)) / wd, min=floor))
    c = torch.fft.irfft(Lg.to(torch.complex128), n=NFFT, dim=-1)[..., :NB]
    q = k / T
    sinc = torch.where(k == 0, torch.ones_like(q), torch.sin(math.pi * q) / (math.pi * q).clamp_min(1e-300))
    cl = c * sinc * ((1.0 - 2.0 * q1) + (2.0 * q1) * torch.cos(2.0 * math.pi * q))
    Le = torch.fft.rfft(torch.cat([cl, cl[..., 1:-1].flip(-1)], -1), dim=-1).real
    c1 = torch.cat([0.5 * cl[..., :1], cl[..., 1:]], -1)
    live = (P > floor).any(-1, keepdim=True)
    cls = torch.where(live[..., 0], (~ok).to(torch.int32), torch.full_like(ok, 2, dtype=torch.int32))
    return torch.where(live, Le, torch.zeros_like(Le)), torch.where(live, c1 @ A.T, torch.zeros_like(c1[..., :A.shape[0]])), cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "envelope_bench.json"))
    args = ap.parse_args()
    A = audio.freq_warp_matrix(NFFT // 2 + 1, ORDER, ALPHA)
    Ad = torch.from_numpy(A).cuda()
    T_def = SR / 500.0
    eng = Engine(0)
    eng.load_envelope(audio.stoi_twiddle(NFFT), HOP, NFFT, SR, A)
    vq = audio._voice_quality_engine(torch.device("cuda:0"), SR, NFFT, HOP, 65.0, 600.0)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "n_fft": NFFT, "hop": HOP, "order": ORDER, "alpha": ALPHA,
           "timing": "HIP events, the variants alternating round by round (median over rounds, min / max beside it)", "shapes": {}}
    for B, L in SHAPES:
        xh, ph = make(B, L)
        x, p = torch.from_numpy(xh).cuda(), torch.from_numpy(ph).cuda()
        variants = {"ev_envelope": lambda: eng.envelope(x, None, p, R.FLOOR), "ev_envelope_with_d_env": lambda: eng.envelope(x, None, p, R.FLOOR, True),
                    "ev_voice_quality": lambda: vq.voice_quality(x, None, 1e-7), "copy_of_the_input": lambda: x.clone(),
                    "torch_restatement": lambda: torch_envelope(x, p, Ad, T_def)}
        ev = {k: bench_timing.stats(ms, args.inner) for k, ms in bench_timing.rounds_of(variants, args.rounds, args.inner, warmup=2).items()}
        n0 = eng.alloc_count()
        env, mcep, cls = eng.envelope(x, None, p, R.FLOOR, True)
        lean = eng.envelope(x, None, p, R.FLOOR)
        te, tm, tc = torch_envelope(x, p, Ad, T_def)
        torch.cuda.synchronize()
        k_ms = ev["ev_envelope"]["median_ms"]
        mean_k = float((2.0 * torch.floor(1.5 * torch.where(p > 0, p, torch.full_like(p, T_def)).double() + 0.5) + 1.0).mean())
        shape = {"rows": B, "samples_per_row": L, "seconds_per_row": L / SR, "frames_per_row": L // HOP, "events": ev,
                 "frames_per_us": B * (L // HOP) / (k_ms * 1e3), "mean_window_samples": mean_k,
                 "voice_quality_over_ev_envelope": ev["ev_voice_quality"]["median_ms"] / k_ms,
                 "torch_over_ev_envelope": ev["torch_restatement"]["median_ms"] / k_ms, "allocations_in_a_repeated_call": eng.alloc_count() - n0,
                 "mcep_equal_without_d_env": bool(torch.equal(lean[1], mcep) and torch.equal(lean[2], cls)),
                 "classes_equal_to_torch": bool(torch.equal(tc, cls[..., 0])),
                 "worst_env_error_against_torch": float((env - te).abs().max()), "worst_mcep_error_against_torch": float((mcep - tm).abs().max())}
        ref = R.envelope(xh[:1, :40 * HOP], None, ph[:1, :40], HOP, NFFT, A, T_def)
        shape["first_40_frames_against_numpy"] = {"classes_equal": bool(np.array_equal(ref["class"][0, :39], cls[0, :39].cpu().numpy())),
                                                  "worst_env_error": float(np.abs(ref["env"][0, :38] - env[0, :38].cpu().numpy()).max()),
                                                  "worst_mcep_error": float(np.abs(ref["mcep"][0, :38] - mcep[0, :38].cpu().numpy()).max())}
        res["shapes"][f"{B}x{L / SR:.0f}s"] = shape
        print(f"{B} x {L / SR:.1f} s: ev_envelope {k_ms:.3f} ms ({ev['ev_envelope']['min_ms']:.3f} .. {ev['ev_envelope']['max_ms']:.3f}), with d_env "
              f"{ev['ev_envelope_with_d_env']['median_ms']:.3f} ms, ev_voice_quality {ev['ev_voice_quality']['median_ms']:.3f} ms, copy "
              f"{ev['copy_of_the_input']['median_ms']:.3f} ms, torch restatement {ev['torch_restatement']['median_ms']:.2f} ms;  "
              f"{shape['frames_per_us']:.3f} frames per us;  mean window {mean_k:.0f} samples;  against torch: classes {shape['classes_equal_to_torch']}, Le "
              f"{shape['worst_env_error_against_torch']:.1e}, mcep {shape['worst_mcep_error_against_torch']:.1e};  {shape['first_40_frames_against_numpy']}")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
