"""What the tools/*_bench.py share: the two timing methods and the tail that writes the profile.  Every tool keeps its own defaults (warm-up,
the host-clock leg), shapes, JSON keys and printed line; its docstring states which method it uses.  No time is a gate.
"""
import json
import os
import statistics
import time

import torch


def timed(fn, calls, warmup, host_clock):
    """HIP events around each of ``calls`` calls after ``warmup`` calls -> median, least and greatest ms; with ``host_clock`` also the host's
    clock around ``calls`` back-to-back calls that end in a synchronise, as a cross-check."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    res = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}
    if host_clock:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        res["host_clock_back_to_back_ms"] = (time.perf_counter() - t0) * 1e3 / calls
    return res


def rounds_of(variants, rounds, inner, warmup=3):
    """{name: per-call ms of every round}: every variant warmed up, then ``rounds`` rounds in which the variants take turns."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return ms


def stats(v, inner):
    med = statistics.median(v)
    return {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / med, "rounds": len(v), "calls_per_round": inner}


def write_json(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {path}")
