#!/usr/bin/env python3
"""Time ev_trim_bounds + ev_trim_apply beside a device-to-device copy of the same bytes (HIP events, median of N calls after warm-up).

    python tools/trim_bench.py [--calls 30] [--out profiles/trim_bench.json]

Shapes: a 12 s take at 22.05 kHz (264 600 samples) with two seconds of room noise at either end, B = 64 and B = 1, librosa's defaults
(frame 2048, hop 512, top_db 60), levelled to 0.95.  The two calls read the input twice (once for the block sums, once to gather) and
write the trimmed rows once; the yardstick is a copy that moves as many bytes (2 x input + output, half of them read, half written).
The bounds never leave the device between the calls.  None of the figures is a gate.
"""
import argparse
import functools
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_timing  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

timed = functools.partial(bench_timing.timed, warmup=5, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trim_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "frame_length": 2048, "hop_length": 512, "top_db": 60.0, "target_peak": 0.95, "shapes": {}}
    g = torch.Generator().manual_seed(0)
    sr, L = 22050, 12 * 22050
    eng = Engine(0)
    for B in (64, 1):
        x = torch.randn(B, L, generator=g) * 1e-5                       # room noise at -80 dB ...
        x[:, 2 * sr: L - 2 * sr] = torch.randn(B, L - 4 * sr, generator=g) * 0.1     # ... around eight seconds of signal
        x = x.cuda()
        bounds = torch.empty(B, 2, dtype=torch.int32, device="cuda")
        peak = torch.empty(B, device="cuda")
        y = torch.empty(B, L, device="cuda")
        out_len = torch.empty(B, dtype=torch.int32, device="cuda")

        def find():
            rc = eng.lib.ev_trim_bounds(eng.h, x.data_ptr(), None, B, L, 2048, 512, 60.0, bounds.data_ptr(), peak.data_ptr(), _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        def gather():
            rc = eng.lib.ev_trim_apply(eng.h, x.data_ptr(), bounds.data_ptr(), peak.data_ptr(), 0.95, B, L, y.data_ptr(), L, out_len.data_ptr(), _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        def both():
            find()
            gather()

        both()
        kept = int(out_len.sum())
        nbytes = 4 * (2 * B * L + B * L)                                # read x twice, write every output row (zeros included)
        n_copy = nbytes // 8                                            # floats: read once, written once = the same bytes
        src, dst = torch.randn(n_copy, device="cuda"), torch.empty(n_copy, device="cuda")
        tb, ta, tt = timed(find, args.calls), timed(gather, args.calls), timed(both, args.calls)
        cp = timed(lambda: dst.copy_(src), args.calls)
        res["shapes"][f"B{B}_L{L}"] = {
            "samples_in": B * L, "samples_kept": kept, "bytes_moved": nbytes, "ev_trim_bounds": tb, "ev_trim_apply": ta, "both": tt, "copy_same_bytes": cp,
            "ratio_of_medians": tt["median_ms"] / cp["median_ms"], "trim_GB_per_s": nbytes / (tt["median_ms"] * 1e-3) / 1e9,
            "copy_GB_per_s": nbytes / (cp["median_ms"] * 1e-3) / 1e9}
        print(f"B={B} L={L}: bounds {tb['median_ms']:.4f} ms  apply {ta['median_ms']:.4f} ms  both {tt['median_ms']:.4f} ms  copy of the same bytes "
              f"{cp['median_ms']:.4f} ms  ratio {tt['median_ms'] / cp['median_ms']:.2f}  ({nbytes / (tt['median_ms'] * 1e-3) / 1e9:.0f} GB/s; kept {kept} of {B * L} samples; "
              f"host clock, back to back: {tt['host_clock_back_to_back_ms']:.4f} / {cp['host_clock_back_to_back_ms']:.4f} ms)")
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
