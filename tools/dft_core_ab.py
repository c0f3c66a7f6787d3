#!/usr/bin/env python3
"""A/B of ev_stft_dist and ev_voice_quality between two builds of the library (profiles/dft_core_ab.json).

    EV_LIB_PATH=<library> python tools/dft_core_ab.py >> runs.log        one run: a fresh process per library, alternate the two, parent first
    python tools/dft_core_ab.py --aggregate runs.log --parent <name of the parent's library file> --out profiles/dft_core_ab.json

A run times what tools/stft_dist_bench.py and tools/voice_quality_bench.py time, with their inputs, shapes (64 x 6 s and 1 x 6 s at 22050 Hz), timing
loops and call counts (10 and 30), without their CPU references, and prints one `RESULT {json}` line: the median ms per call, and checksums of the
outputs.  The aggregate is, per number, the median of each library's medians, the parent's max - min as the margin, and whether the other library
lies within it.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def run():
    import torch

    import stft_dist_bench as SB
    import voice_quality_bench as VB
    from emojivoice_amd import audio
    from emojivoice_amd._lib import LIB_PATH, Engine, _stream_ptr

    res = {"lib": os.path.basename(LIB_PATH)}
    L = SB.SECONDS * SB.SR
    g = torch.Generator().manual_seed(0)
    engines = {}
    for nfft, hop, win in audio.MSTFT_RESOLUTIONS:
        engines[(nfft, hop, win)] = e = Engine(0)
        e.load_stft_dist(audio.stft_dist_window(win), audio.stoi_twiddle(nfft), hop, nfft)
    t = audio.voice_quality_tables(VB.SR, VB.NFFT)
    vq = Engine(0)
    vq.load_voice_quality(audio.stft_dist_window(VB.WIN), audio.stoi_twiddle(VB.NFFT), VB.HOP, VB.NFFT, t["bands"], t["slope_w"], t["q_fit"], t["q_min"],
                          t["q_max"], t["fit_w"], t["q_mean"])
    NF = -(-L // VB.HOP)
    for B in (64, 1):
        x_h = 0.1 * torch.randn(B, L, generator=g)
        x, y = x_h.cuda(), (x_h + 0.01 * torch.randn(B, L, generator=g)).cuda()
        sums = torch.empty(B, 4, dtype=torch.float64, device="cuda")
        counts = torch.empty(B, dtype=torch.int32, device="cuda")
        for (nfft, hop, win), e in engines.items():
            def call_sd():
                rc = e.lib.ev_stft_dist(e.h, x.data_ptr(), y.data_ptr(), None, B, L, audio.MSTFT_POWER_FLOOR, None, sums.data_ptr(), counts.data_ptr(),
                                        _stream_ptr())
                assert rc == 0, e.lib.ev_last_error(e.h).decode()
            res[f"ev_stft_dist_{nfft}_{hop}_{win}_B{B}"] = SB.timed(call_sd, 10)["median_ms"]
        frame = torch.empty(B, NF, 8, dtype=torch.float64, device="cuda")
        peak = torch.empty(B, NF, dtype=torch.int32, device="cuda")

        def call_vq():
            rc = vq.lib.ev_voice_quality(vq.h, x.data_ptr(), None, B, L, VB.FLOOR, frame.data_ptr(), peak.data_ptr(), None, _stream_ptr())
            assert rc == 0, vq.lib.ev_last_error(vq.h).decode()
        res[f"ev_voice_quality_B{B}"] = VB.timed(call_vq, 30)["median_ms"]
        res[f"checksum_B{B}"] = [float(sums.sum()), float(frame.sum()), int(peak.sum())]
    print("RESULT " + json.dumps(res))


def aggregate(log, parent, out):
    runs = {True: [], False: []}
    with open(log) as f:
        for line in f:
            if line.startswith("RESULT "):
                r = json.loads(line[7:])
                runs[r["lib"] == parent].append(r)
    rows = {}
    for k in [k for k in runs[True][0] if k.startswith("ev_")]:
        p, n = [r[k] for r in runs[True]], [r[k] for r in runs[False]]
        mp, mn, margin = statistics.median(p), statistics.median(n), max(p) - min(p)
        rows[k] = {"parent_runs": p, "new_runs": n, "parent": mp, "parent_spread": margin, "new": mn, "new_minus_parent": mn - mp,
                   "within": abs(mn - mp) <= margin}
        print(f"{k:36s} parent {mp:8.4f} spread {margin:7.4f} new {mn:8.4f} diff {mn - mp:+8.4f} within {rows[k]['within']}")
    same = all(r[c] == runs[True][0][c] for r in runs[True] + runs[False] for c in ("checksum_B64", "checksum_B1"))
    print("checksums equal", same)
    with open(out, "w") as f:
        json.dump({"rows": rows, "checksums_equal_in_every_run": same}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--aggregate", metavar="LOG")
    ap.add_argument("--parent", default="libparent.so")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dft_core_ab.json"))
    a = ap.parse_args()
    if a.aggregate:
        aggregate(a.aggregate, a.parent, a.out)
    else:
        sys.path.insert(0, REPO)
        run()
