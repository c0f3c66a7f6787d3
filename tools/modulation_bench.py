#!/usr/bin/env python3
"""Time ev_modulation at ev_functionals' shapes, 64 x 20 contours x 516 frames (64 utterances of 6 s at hop 256 and 22.05 kHz), 1 x 20 x 516 and
1 x 1 x 4096, on the default grid (1 .. 16 Hz by 0.125 Hz: 121 frequencies, min_run 18, min_cycles 2, the tremor and the rhythm band), beside
  (a) ev_functionals on the same stack (percentiles 0.2 / 0.5 / 0.8): the neighbour of the family, as a scale;
  (b) ``torch_modulation``: a batched torch restatement of the spectrum and the weights on the device (cummax and scatter_add for the runs, a
      (B, K, F, NM) phase tensor for the transform; no peaks), some sixty torch launches;
  (c) the numpy restatement (tests/modulation_ref.py) over the contours on 16 worker processes, which are started and finished BEFORE this
      process touches the GPU.
The three device variants take turns, round by round, under HIP events (bench_timing.rounds_of); each is also timed by the wall clock around a
synchronised call (median of N after warm-up).

    python tools/modulation_bench.py [--rounds 10] [--inner 3] [--calls 20] [--out profiles/modulation_bench.json]

Nothing here is a gate: the figures are what was seen.  Every shape is compared with (b), and the two small ones with the numpy restatement:
weights and counts equal, worst error.
"""
import argparse
import multiprocessing
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
import modulation_ref as R  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

Q = (0.2, 0.5, 0.8)
SHAPES = ((64, 20, 516), (1, 20, 516), (1, 1, 4096))
KW = R.AUDIO_KW


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


def make(B, K, F):
    g = np.random.default_rng(B * 1000 + F)
    t = np.arange(F) / R.AUDIO_RATE
    v = 40.0 + np.cumsum(0.05 * g.standard_normal((B, K, F)), axis=-1) + 0.4 * np.sin(2 * np.pi * (g.uniform(3.0, 9.0, (B, K, 1)) * t + g.uniform(size=(B, K, 1))))
    m = np.stack([[R.make_mask("runs", F, g, KW["min_run"]) for _ in range(K)] for _ in range(B)])
    return v, m


def _one(args):
    v, m = args
    out = R.contour(v, m, len(v), **KW)
    return out["spec"], out["weight"], out["count"]


def torch_modulation(v, mask, nu, min_run, min_cycles):
    """ev_modulation's d_spec and d_weight by batched torch ops on the device; v (B, K, F) float64, mask (B, K, F) bool, nu (NM,) float64.  Sums
    are torch's, so the spectrum agrees to rounding only."""
    B, K, F = v.shape
    NM = nu.shape[0]
    f = torch.arange(F, device=v.device)
    valid = mask & torch.isfinite(v)
    first = valid & ~torch.nn.functional.pad(valid[..., :-1], (1, 0))
    start = torch.cummax(torch.where(first, f, torch.full_like(f, -1)), dim=-1).values.clamp(min=0)
    rid = (torch.cumsum(first, dim=-1) - 1).clamp(min=0)
    NR = (F + 1) // 2

    def per_run(x):
        return torch.zeros(B, K, NR, dtype=torch.float64, device=v.device).scatter_add_(-1, rid, x)

    lr = per_run(valid.to(torch.float64))
    l = lr.gather(-1, rid)
    an = valid & (l >= min_run)
    t = (f - start).to(torch.float64)
    tc = t - (l - 1.0) / 2.0
    x = torch.where(an, v, torch.zeros_like(v))
    m = per_run(x) / lr.clamp(min=1.0)
    b = per_run(tc * x) / ((lr * (lr * lr - 1.0)).clamp(min=1.0) / 12.0)
    r = torch.where(an, (x - m.gather(-1, rid)) - b.gather(-1, rid) * tc, torch.zeros_like(v))
    w = torch.where(an, 0.5 - 0.5 * torch.cos(torch.pi * (2.0 * t + 1.0) / l.clamp(min=1.0)), torch.zeros_like(v))
    sw = per_run(w)
    xw = (w * r)[..., None]
    ph = nu * t[..., None]
    ang = 2.0 * torch.pi * (ph - ph.floor())
    idx = rid[..., None].expand(B, K, F, NM)
    xr = torch.zeros(B, K, NR, NM, dtype=torch.float64, device=v.device).scatter_add_(2, idx, xw * torch.cos(ang))
    xi = torch.zeros(B, K, NR, NM, dtype=torch.float64, device=v.device).scatter_add_(2, idx, xw * torch.sin(ang))
    P = 2.0 * (xr * xr + xi * xi) / (sw * sw).clamp(min=1e-300)[..., None]
    res = ((lr >= min_run)[..., None] & (nu * lr[..., None] >= min_cycles)).to(torch.float64) * lr[..., None]
    W = res.sum(dim=2)
    return (res * P).sum(dim=2) / W.clamp(min=1.0), W.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "modulation_bench.json"))
    args = ap.parse_args()
    data = {s: make(*s) for s in SHAPES}
    # ---- (c) first: the workers are gone before the GPU is opened
    numpy_ms, numpy_out = {}, {}
    with multiprocessing.get_context("fork").Pool(16) as pool:
        for (B, K, F), (v, m) in data.items():
            jobs = [(v[b, k], m[b, k]) for b in range(B) for k in range(K)]
            pool.map(_one, jobs[:16])                                     # (warm-up)
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                out = pool.map(_one, jobs, chunksize=max(len(jobs) // 64, 1))
                ms.append(1e3 * (time.perf_counter() - t0))
            numpy_ms[(B, K, F)] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": 3, "processes": 16}
            numpy_out[(B, K, F)] = out
    res = {"device": torch.cuda.get_device_name(0), "grid": {k: KW[k] for k in ("nu0", "dnu", "NM", "min_run", "min_cycles")}, "bands": [list(b) for b in KW["bands"]],
           "timing": "HIP events, the three device variants alternating round by round (median over rounds); wall: the host clock around a synchronised "
                     "call, median; numpy: the host clock around a map over 16 processes, median of 3", "shapes": {}}
    eng = Engine(0)
    qa = np.asarray(Q, dtype=np.float64)
    ba = np.ascontiguousarray(np.asarray(KW["bands"], dtype=np.int32))
    NM, NB = KW["NM"], len(KW["bands"])
    nu = torch.from_numpy(R.grid(KW["nu0"], KW["dnu"], NM)).cuda()
    for (B, K, F), (v_h, m_h) in data.items():
        v, m8 = torch.from_numpy(v_h).cuda(), torch.from_numpy(m_h).cuda()
        mb = m8 != 0
        spec = torch.empty(B, K, NM, dtype=torch.float64, device="cuda")
        weight = torch.empty(B, K, NM, dtype=torch.int32, device="cuda")
        peak = torch.empty(B, K, NB, 4, dtype=torch.float64, device="cuda")
        stat = torch.empty(B, K, 2, dtype=torch.float64, device="cuda")
        count = torch.empty(B, K, 4 + NB, dtype=torch.int32, device="cuda")
        fstat = torch.empty(B, K, 12 + len(Q), dtype=torch.float64, device="cuda")
        fcount = torch.empty(B, K, 8, dtype=torch.int32, device="cuda")

        def call_mod():
            rc = eng.lib.ev_modulation(eng.h, v.data_ptr(), m8.data_ptr(), None, B, K, F, KW["nu0"], KW["dnu"], NM, KW["min_run"], KW["min_cycles"],
                                       ba.ctypes.data, NB, spec.data_ptr(), weight.data_ptr(), peak.data_ptr(), stat.data_ptr(), count.data_ptr(), _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        def call_func():
            rc = eng.lib.ev_functionals(eng.h, v.data_ptr(), m8.data_ptr(), None, B, K, F, qa.ctypes.data, len(Q), fstat.data_ptr(), fcount.data_ptr(),
                                        _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        call_torch = lambda: torch_modulation(v, mb, nu, KW["min_run"], KW["min_cycles"])
        variants = {"ev_modulation": call_mod, "ev_functionals": call_func, "torch_restatement": call_torch}
        ev = {k: bench_timing.stats(ms, args.inner) for k, ms in bench_timing.rounds_of(variants, args.rounds, args.inner).items()}
        wl = {k: wall(fn, args.calls) for k, fn in variants.items()}
        call_mod()
        ts, tw = call_torch()
        torch.cuda.synchronize()
        pairs = int(weight.to(torch.int64).sum())                        # (frame, frequency) pairs transformed: one cospi and one sinpi each
        k_ms = ev["ev_modulation"]["median_ms"]
        shape = {"rows": B, "contours_per_row": K, "frames": F, "workgroups": B * K,
                 "lds_bytes": (F + (F & 1) + max(2, ((F + 1) // 4 + 1) // 2 * 2) + 128) * 8 + (max(2, ((F + 1) // 4 + 1) // 2 * 2) + 128 + 24) * 4,
                 "events": ev, "wall": wl, "numpy_restatement_16_processes": numpy_ms[(B, K, F)],
                 "ev_functionals_over_ev_modulation": ev["ev_functionals"]["median_ms"] / k_ms,
                 "torch_over_ev_modulation": ev["torch_restatement"]["median_ms"] / k_ms,
                 "numpy_over_ev_modulation_wall": numpy_ms[(B, K, F)]["median_ms"] / wl["ev_modulation"]["median_ms"],
                 "analysed_runs": int(count[..., 2].sum()), "analysed_frames": int(count[..., 3].sum()), "transformed_pairs": pairs,
                 "cospi_sinpi_pairs_per_ns": pairs / (k_ms * 1e6),
                 "weights_equal_to_torch": bool(torch.equal(tw, weight)), "worst_spectrum_error_against_torch": R.err(spec.cpu().numpy(), ts.cpu().numpy())}
        ref = numpy_out[(B, K, F)]
        shape["weights_and_counts_equal_to_the_restatement"] = bool(
            np.array_equal(weight.cpu().numpy().reshape(-1, NM), np.stack([o[1] for o in ref]))
            and np.array_equal(count.cpu().numpy().reshape(-1, 4 + NB), np.stack([o[2] for o in ref])))
        shape["worst_spectrum_error_against_the_restatement"] = R.err(spec.cpu().numpy().reshape(-1, NM), np.stack([o[0] for o in ref]))
        res["shapes"][f"{B}x{K}x{F}"] = shape
        print(f"{B} x {K} x {F}: ev_modulation {k_ms:.3f} ms by HIP events ({wl['ev_modulation']['median_ms']:.3f} ms wall), ev_functionals "
              f"{ev['ev_functionals']['median_ms']:.3f} ms, torch restatement {ev['torch_restatement']['median_ms']:.3f} ms "
              f"({wl['torch_restatement']['median_ms']:.3f} ms wall), numpy on 16 processes {numpy_ms[(B, K, F)]['median_ms']:.1f} ms;  "
              f"{pairs} cospi / sinpi pairs, {shape['cospi_sinpi_pairs_per_ns']:.2f} per ns;  weights equal to torch {shape['weights_equal_to_torch']}, spectrum "
              f"{shape['worst_spectrum_error_against_torch']:.1e};  against the restatement: weights and counts equal "
              f"{shape['weights_and_counts_equal_to_the_restatement']}, spectrum {shape['worst_spectrum_error_against_the_restatement']:.1e}")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
