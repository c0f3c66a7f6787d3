#!/usr/bin/env python3
"""Time ev_srmr on 64 x 6 s, 1 x 6 s and 1 x 600 s of 16 kHz audio at the default tables (23 channels, 8 bands, H = 1024), beside
  (a) ev_loudness on the same rows (K-weighting designed for 16 kHz, 100 ms sub-blocks): the neighbour whose chunk / carry / rerun pattern this
      one applies twice, as a scale;
  (b) ``torch_srmr``: a batched torch restatement on the device with the same structure (every chunk of every row at once, H sequential steps per
      pass, the carries chunk by chunk): some hundred thousand small torch launches.
The three take turns, round by round, under HIP events (bench_timing.rounds_of): medians with min / max.

    python tools/srmr_bench.py [--rounds 5] [--inner 1] [--out profiles/srmr_bench.json]

Nothing here is a gate and no ratio is promised: the figures are what was seen.  Every shape is compared with (b): counts equal, worst error.
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
import srmr_ref as R  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine  # noqa: E402

SR = 16000
SHAPES = ((64, 6), (1, 6), (1, 600))                                     # (rows, seconds)


def make(B, seconds):
    """B rows of a gated harmonic source with noise: 6 s of it, tiled to the length."""
    base = np.stack([R.voice(6 * SR, SR, seed=100 + b, f0=90.0 + 3.0 * b) for b in range(B)])
    return np.tile(base, (1, seconds // 6))


def torch_srmr(x, T):
    """ev_srmr's d_mean, d_srmr and d_counts for full rows by batched torch ops; x (B, L) float32 on the device, T the tables as float64 device
    tensors.  torch rounds a product before it adds, so it agrees to rounding only."""
    B, L = x.shape
    H, N, K = T["hop"], T["chan"].shape[0], T["mod"].shape[0]
    nf = (L - 4 * H) // H + 1
    nc = nf + 3
    X = x[:, :nc * H].to(torch.float64).reshape(B, nc, H)
    ar, ai, g = T["chan"][:, 0], T["chan"][:, 1], T["chan"][:, 2]
    m, win = T["mod"], T["window"]
    z = lambda *s: torch.zeros((B, nc) + s, dtype=torch.float64, device=x.device)

    def run(r, i, s1, s2, bands, pieces):
        r, i = list(r.unbind(-1)), list(i.unbind(-1))
        acc = [z(N, K) for _ in range(4)] if pieces else None
        for t in range(H):
            vr, vi = X[:, :, t, None], None
            for s in range(4):
                nr = vr + (ar * r[s] - ai * i[s])
                ni = ar * i[s] + ai * r[s]
                if vi is not None:
                    ni = vi + ni
                r[s], i[s] = nr, ni
                vr, vi = nr, ni
            if bands:
                e = (g * torch.sqrt(r[3] * r[3] + i[3] * i[3]))[..., None]
                y = m[:, 0] * e + s1
                s1 = (m[:, 1] * e + s2) - m[:, 3] * y
                s2 = m[:, 2] * e - m[:, 4] * y
                if pieces:
                    for q in range(4):
                        v = win[q * H + t] * y
                        acc[q] = acc[q] + v * v
        return torch.stack(r, -1), torch.stack(i, -1), s1, s2, acc

    zr, zi, _, _, _ = run(z(N, 4), z(N, 4), None, None, False, False)
    Mr, Mi, Mb = T["Mr"], T["Mi"], T["Mb"]
    cr, ci = torch.zeros_like(zr), torch.zeros_like(zi)
    sr_, si_ = torch.zeros_like(zr[:, 0]), torch.zeros_like(zi[:, 0])
    for c in range(nc):
        cr[:, c], ci[:, c] = sr_, si_
        sr_, si_ = (zr[:, c] + (torch.einsum("nrk,bnk->bnr", Mr, sr_) - torch.einsum("nrk,bnk->bnr", Mi, si_)),
                    zi[:, c] + (torch.einsum("nrk,bnk->bnr", Mr, si_) + torch.einsum("nrk,bnk->bnr", Mi, sr_)))
    _, _, z1, z2, _ = run(cr, ci, z(N, K), z(N, K), True, False)
    b1, b2 = torch.zeros_like(z1), torch.zeros_like(z2)
    s1, s2 = torch.zeros_like(z1[:, 0]), torch.zeros_like(z2[:, 0])
    for c in range(nc):
        b1[:, c], b2[:, c] = s1, s2
        s1, s2 = (z1[:, c] + Mb[:, 0, 0] * s1) + Mb[:, 0, 1] * s2, (z2[:, c] + Mb[:, 1, 0] * s1) + Mb[:, 1, 1] * s2
    p = run(cr, ci, b1, b2, True, True)[4]
    E = (p[0][:, 0:nf] + p[1][:, 1:nf + 1]) + (p[2][:, 2:nf + 2] + p[3][:, 3:nf + 3])
    mean = E.sum(1) / nf
    ch = mean.sum(-1)
    cum = torch.cumsum(ch / ch.sum(-1, keepdim=True), -1)
    j90 = (cum > R.SHARE).to(torch.int32).argmax(-1)
    bw = T["erb"][j90]
    ks = (T["cutoff"][None, :] < bw[:, None]).sum(-1).clamp(min=min(5, K), max=K)
    hi = (torch.arange(K, device=x.device)[None, :] >= 4) & (torch.arange(K, device=x.device)[None, :] < ks[:, None])
    ratio = mean[:, :, :4].sum((1, 2)) / (mean * hi[:, None, :]).sum((1, 2))
    return mean, torch.stack([ratio, bw], 1), torch.stack([torch.full_like(j90, nf), j90, ks.to(torch.int32)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "srmr_bench.json"))
    args = ap.parse_args()
    tab = audio.srmr_tables()
    Mr, Mi, Mb = R.transitions(tab)
    T = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(tab, Mr=Mr, Mi=Mi, Mb=Mb).items() if isinstance(v, np.ndarray)}
    T["hop"] = tab["hop"]
    eng = Engine(0)
    eng.load_srmr(tab["chan"], tab["mod"], tab["window"], tab["erb"], tab["cutoff"], tab["hop"])
    kw = audio.k_weighting(SR)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "channels": 23, "bands": 8, "hop": tab["hop"],
           "timing": "HIP events, the three variants alternating round by round (median over rounds, min / max beside it)", "shapes": {}}
    for B, seconds in SHAPES:
        x = torch.from_numpy(make(B, seconds)).cuda()
        variants = {"ev_srmr": lambda: eng.srmr(x, None), "ev_loudness": lambda: eng.loudness(x, None, SR // 10, kw, audio.ABSOLUTE_GATE, False, False),
                    "torch_restatement": lambda: torch_srmr(x, T)}
        n0 = None
        ev = {}
        for k, ms in bench_timing.rounds_of(variants, args.rounds, args.inner, warmup=1).items():
            ev[k] = bench_timing.stats(ms, args.inner)
        n0 = eng.alloc_count()
        _, mean, out, counts = eng.srmr(x, None)
        tm, to, tc = torch_srmr(x, T)
        torch.cuda.synchronize()
        k_ms = ev["ev_srmr"]["median_ms"]
        samples = B * seconds * SR
        shape = {"rows": B, "seconds": seconds, "samples": samples, "chunks_per_row": int(counts[0, 0]) + 3, "events": ev,
                 "samples_per_us": samples / (k_ms * 1e3), "ev_srmr_over_ev_loudness": k_ms / ev["ev_loudness"]["median_ms"],
                 "torch_over_ev_srmr": ev["torch_restatement"]["median_ms"] / k_ms, "allocations_in_a_repeated_call": eng.alloc_count() - n0,
                 "counts_equal_to_torch": bool(torch.equal(tc, counts)), "worst_mean_error_against_torch": R.rel_err(mean.cpu().numpy(), tm.cpu().numpy()),
                 "worst_srmr_error_against_torch": R.rel_err(out.cpu().numpy(), to.cpu().numpy()), "srmr": out[:, 0].tolist()[:4]}
        res["shapes"][f"{B}x{seconds}s"] = shape
        print(f"{B} x {seconds} s: ev_srmr {k_ms:.3f} ms ({ev['ev_srmr']['min_ms']:.3f} .. {ev['ev_srmr']['max_ms']:.3f}), ev_loudness "
              f"{ev['ev_loudness']['median_ms']:.3f} ms, torch restatement {ev['torch_restatement']['median_ms']:.1f} ms;  {shape['samples_per_us']:.1f} samples "
              f"per us;  counts equal to torch {shape['counts_equal_to_torch']}, mean {shape['worst_mean_error_against_torch']:.1e}, srmr "
              f"{shape['worst_srmr_error_against_torch']:.1e}")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
