#!/usr/bin/env python3
"""Vocoder-only throughput of the HiFi-GAN V1 / V2 / V3 generators (synthetic weights), one JSON line.

    python tools/vocoder_configs_bench.py [--iters 10] [--warmup 3]

Per config: ms per call and audio-s/s at batch 64 x 516 mel frames (bench.py's config-2 shape) and batch 1 x 516 (a streaming
utterance).  For V3 also the one-launch ResBlock2 (resblock2_h16_kernel) switched off (ev_dbg_set_chain), and a sweep of its gate
(EV_RB2_MINKEEP = eighths of a tile a block must store to take the fused form; 8 = never), each in a fresh process since the gate is
read once.  Accuracy: every config against the fp64 restatement of tests/test_vocoder_configs.py on two rows of 64 frames.
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from emojivoice_amd import weights as W  # noqa: E402
from emojivoice_amd.hifigan import AttrDict, Generator, v1, v2, v3  # noqa: E402

CONFIGS = {"v1": v1, "v2": v2, "v3": v3}
SHAPES = ((64, 516), (1, 516))


def vocoder(h):
    g = Generator(AttrDict(h)).to("cuda:0")
    g.load_state_dict(W.synthetic_hifigan_state(h))
    g.remove_weight_norm()
    return g


def time_ms(g, B, T, iters, warmup):
    mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(B + T)) * 2.0 - 5.0).cuda()
    for _ in range(warmup):
        g(mel)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g(mel)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def record(ms, B, T):
    return {"ms": round(ms, 3), "audio_s_per_s": round(B * T * 256 / 22050 / (ms / 1e3), 1)}


def measure(names, iters, warmup, chain_off=False):
    out = {}
    for name in names:
        g = vocoder(CONFIGS[name])
        g._sync_engine()
        if chain_off:
            g.engine.set_chain(False)
        for B, T in SHAPES:
            out[f"{name}_b{B}"] = record(time_ms(g, B, T, iters, warmup), B, T)
        g.engine.close()
        del g
        torch.cuda.empty_cache()
    return out


def accuracy():
    spec = importlib.util.spec_from_file_location("tvc", os.path.join(REPO, "tests", "test_vocoder_configs.py"))
    tvc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tvc)
    out = {}
    mel = torch.randn(2, 80, 64, generator=torch.Generator().manual_seed(64)) * 2.0 - 5.0
    for name, h in CONFIGS.items():
        g = vocoder(h)
        e = g(mel.cuda()).cpu().double() - tvc.restate(W.synthetic_hifigan_state(h), mel, h)
        out[name] = {"wav_rms_err": float(e.pow(2).mean().sqrt()), "wav_linf_err": float(e.abs().max())}
        g.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=str, default="", help="internal: measure these configs only and print their records")
    a = ap.parse_args()
    if a.only:
        print(json.dumps(measure(a.only.split(","), a.iters, a.warmup)))
        return
    res = {"shape": {"mel_frames": 516, "batches": [B for B, _ in SHAPES]}, "arithmetic": 16}
    res["configs"] = measure(list(CONFIGS), a.iters, a.warmup)
    res["v3_resblock2_unfused"] = measure(["v3"], a.iters, a.warmup, chain_off=True)
    sweep = {}
    for keep8 in (2, 4, 6, 8):
        env = dict(os.environ, EV_RB2_MINKEEP=str(keep8))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "v3", "--iters", str(a.iters), "--warmup", str(a.warmup)],
                           env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sweep[str(keep8)] = {"error": r.returncode}
            break
        sweep[str(keep8)] = json.loads(r.stdout.strip().splitlines()[-1])
    res["v3_rb2_gate_sweep"] = sweep
    res["accuracy_vs_fp64_restatement"] = accuracy()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
