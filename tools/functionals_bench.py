#!/usr/bin/env python3
"""Time ev_functionals at 64 x 20 contours x 516 frames (64 utterances of 6 s at hop 256 and 22.05 kHz, the contours of a full voice report), at
1 x 20 x 516 and at 1 x 1 x 4096, with the percentiles 0.2 / 0.5 / 0.8, beside two ways of getting such numbers without it, on the same data:
  (a) audio.prosody_statistics on the K = 1 pitch contour (contour 0 as f0, its mask as the voicing): how the f0 percentiles were obtained
      before this call existed, a Python loop over the rows with a boolean gather and a torch.quantile each, every iteration waiting for the
      device.  It gives three percentiles of ONE contour and nothing else;
  (b) ``torch_functionals``: a batched torch restatement of the full set on the device (masked means, a sort behind +inf for min / max and the
      percentiles, cummax for the starts of parts and runs), some forty torch launches.
All three are timed by the wall clock around a synchronised call (median of N after warm-up), since (a) waits on the host; HIP events around the
ev_functionals launch give the kernel alone.

    python tools/functionals_bench.py [--calls 30] [--out profiles/functionals_bench.json]

Nothing here is a gate: the figures are what was seen.  Every shape is also compared with (b), and the smallest with the numpy restatement
(tests/functionals_ref.py): counts equal, worst error.
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
import functionals_ref as R  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

Q = (0.2, 0.5, 0.8)
SHAPES = ((64, 20, 516), (1, 20, 516), (1, 1, 4096))


def wall(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


events = functools.partial(bench_timing.timed, warmup=3, host_clock=False)


def _masked_mean_sd(x, m):
    n = m.sum(dim=-1)
    d = n.clamp(min=1).to(torch.float64)
    mean = torch.where(m, x, torch.zeros_like(x)).sum(dim=-1) / d
    var = torch.where(m, (x - mean[..., None]) ** 2, torch.zeros_like(x)).sum(dim=-1) / d
    return torch.where(n > 0, mean, torch.zeros_like(mean)), torch.where(n > 0, var.sqrt(), torch.zeros_like(mean)), n


def _stretch_stats(flag, inside):
    """(count, mean, sd) of the lengths of the maximal stretches of ``flag`` among the frames ``inside`` (B, K, F)."""
    F = flag.shape[-1]
    f = torch.arange(F, device=flag.device)
    flag = flag & inside
    prev = torch.nn.functional.pad(flag[..., :-1], (1, 0))
    nxt = torch.nn.functional.pad(flag[..., 1:], (0, 1))
    start = torch.cummax(torch.where(flag & ~prev, f, torch.full_like(f, -1)), dim=-1).values
    end = flag & ~nxt
    length = torch.where(end, f - start + 1, torch.zeros_like(start)).to(torch.float64)
    mean, sd, n = _masked_mean_sd(length, end)
    return n, mean, sd


def torch_functionals(v, mask, lengths, q):
    """ev_functionals' outputs (stat (B, K, 12 + NQ), count (B, K, 8)) by batched torch ops on the device; v (B, K, F) float64, mask (B, K, F)
    bool, lengths (B,) int64.  Sums are torch's, so the statistics agree to rounding only."""
    B, K, F = v.shape
    f = torch.arange(F, device=v.device)
    inside = (f[None, :] < lengths[:, None])[:, None, :].expand(B, K, F)
    on = mask & inside
    fin = torch.isfinite(v)
    valid, dropped = on & fin, on & ~fin
    x = torch.where(valid, v, torch.zeros_like(v))
    mean, sd, k = _masked_mean_sd(x, valid)
    s = torch.where(valid, v, torch.full_like(v, float("inf"))).sort(dim=-1).values
    km1 = (k - 1).clamp(min=0)
    qs = torch.tensor(q, dtype=torch.float64, device=v.device)
    p = qs[None, None, :] * km1[..., None].to(torch.float64)
    j = p.floor().to(torch.int64)
    t = p - j.to(torch.float64)
    sj, sh = s.gather(-1, j), s.gather(-1, torch.minimum(j + 1, km1[..., None]))
    has = (k > 0)[..., None]
    pct = torch.where(has, sj + t * (sh - sj), torch.zeros_like(sj))
    mn = torch.where(k > 0, s[..., 0], torch.zeros_like(mean))
    mx = torch.where(k > 0, s.gather(-1, km1[..., None])[..., 0], torch.zeros_like(mean))
    # pairs (f, f + 1): adjacent when both frames are valid
    adj = valid[..., :-1] & valid[..., 1:]
    dv = x[..., 1:] - x[..., :-1]
    cls = torch.where(adj, torch.sign(dv), torch.zeros_like(dv)).to(torch.int64)
    cp, cn = torch.nn.functional.pad(cls[..., :-1], (1, 0)), torch.nn.functional.pad(cls[..., 1:], (0, 1))
    fp = f[:-1]
    start = torch.cummax(torch.where((cls != 0) & (cp != cls), fp, torch.full_like(fp, -1)), dim=-1).values.clamp(min=0)
    slope = (x[..., 1:] - x.gather(-1, start)) / (fp + 1 - start).to(torch.float64)
    out = [mean, sd, mn, mx]
    counts = [k, dropped.sum(dim=-1)]
    for sign in (1, -1):
        m, d, n = _masked_mean_sd(slope, (cls == sign) & (cn != sign))
        out += [m, d]
        counts.append(n)
    peak = adj[..., :-1] & adj[..., 1:] & (dv[..., :-1] > 0) & (dv[..., 1:] <= 0)
    counts.append(peak.sum(dim=-1))
    nr, rm, rs = _stretch_stats(valid, inside)
    ng, gm, gs = _stretch_stats(~valid, inside)
    out += [rm, rs, gm, gs]
    counts += [nr, ng, adj.sum(dim=-1)]
    return torch.cat([torch.stack(out, dim=-1), pct], dim=-1), torch.stack(counts, dim=-1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "functionals_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "percentiles": list(Q), "timing": "wall clock around a synchronised call, median; kernel_ms: HIP events",
           "shapes": {}}
    eng = Engine(0)
    qa = np.asarray(Q, dtype=np.float64)
    for B, K, F in SHAPES:
        g = np.random.default_rng(B * 1000 + F)
        v_h = 100.0 + np.cumsum(g.standard_normal((B, K, F)), axis=-1)
        m_h = np.stack([[R.make_mask("runs", F, g) for _ in range(K)] for _ in range(B)])
        v, m8 = torch.from_numpy(v_h).cuda(), torch.from_numpy(m_h).cuda()
        mb = m8 != 0
        lens = torch.full((B,), F, dtype=torch.int64, device="cuda")
        stat = torch.empty(B, K, 12 + len(Q), dtype=torch.float64, device="cuda")
        count = torch.empty(B, K, 8, dtype=torch.int32, device="cuda")
        f0, voiced = v[:, 0].float().contiguous(), mb[:, 0].contiguous()

        def call_ev():
            rc = eng.lib.ev_functionals(eng.h, v.data_ptr(), m8.data_ptr(), None, B, K, F, qa.ctypes.data, len(Q), stat.data_ptr(), count.data_ptr(),
                                        _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        tk, tw = events(call_ev, args.calls), wall(call_ev, args.calls)
        ta = wall(lambda: audio.prosody_statistics(f0, voiced), args.calls)
        tb = wall(lambda: torch_functionals(v, mb, lens, Q), args.calls)
        ts, tc = torch_functionals(v, mb, lens, Q)
        shape = {"rows": B, "contours_per_row": K, "frames": F, "workgroups": B * K, "lds_bytes": 512 + 12 * max(256, 1 << (F - 1).bit_length()),
                 "ev_functionals": {"wall": tw, "kernel": tk},
                 "a_prosody_statistics_k1_pitch_contour_only": ta, "b_batched_torch_restatement_full_set": tb,
                 "a_over_ev_functionals": ta["median_ms"] / tw["median_ms"], "b_over_ev_functionals": tb["median_ms"] / tw["median_ms"],
                 "counts_equal_to_b": bool(torch.equal(tc, count)), "worst_error_against_b": R.err(stat.cpu().numpy(), ts.cpu().numpy()),
                 "valid_frames": int(count[..., 0].sum()), "parts": int(count[..., 2:4].sum())}
        if B * K <= 20:
            ref = R.batch(v_h, m_h, None, Q)
            shape["counts_equal_to_the_restatement"] = bool(np.array_equal(count.cpu().numpy(), ref["count"]))
            shape["worst_error_against_the_restatement"] = R.err(stat.cpu().numpy(), ref["stat"])
        res["shapes"][f"{B}x{K}x{F}"] = shape
        print(f"{B} x {K} x {F}: ev_functionals {tw['median_ms']:.3f} ms wall (kernel {tk['median_ms']:.3f} ms by HIP events)  (a) prosody_statistics, "
              f"contour 0 only {ta['median_ms']:.3f} ms  (b) batched torch, full set {tb['median_ms']:.3f} ms  counts equal to (b) {shape['counts_equal_to_b']}, "
              f"worst error against (b) {shape['worst_error_against_b']:.2e}"
              + (f"  against the restatement: counts equal {shape['counts_equal_to_the_restatement']}, "
                 f"{shape['worst_error_against_the_restatement']:.2e}" if B * K <= 20 else ""))
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
