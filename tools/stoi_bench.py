#!/usr/bin/env python3
"""Time ev_stoi beside a device-to-device copy of the bytes it reads (HIP events, median of N calls after warm-up).

    python tools/stoi_bench.py [--calls 20] [--out profiles/stoi_bench.json]

Shapes at 10 kHz, the standard geometry (256 / 128 / 512, 15 one-third octave bands, segments of 30 frames): 64 x 6 s and 1 x 6 s (60 000
samples a row: 467 frames).  The call reads both signals (twice where frames overlap; the re-reads come out of the caches) and writes the
segment scores, two doubles per 128 samples; the yardstick is a copy that moves the two inputs' bytes once.  The kernel is NOT expected near
that copy: it is arithmetic — about 256 x 212 x 2 float64 fmas per frame and signal for the DFT of the bins the bands cover, 6.5 G fmas at
64 x 6 s — and at one row it is the latency of five launches.  The input is Gaussian noise against itself at 0 dB SNR: every frame is kept,
which is the most work a row of this length can be (silent frames shorten the silence-removed signal).  The script also prints the float64
fma rate of the whole call.  None of the figures is a gate.
"""
import argparse
import functools
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_timing  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, W, H, NFFT, N = audio.STOI_SR, audio.STOI_WINDOW, audio.STOI_HOP, audio.STOI_NFFT, audio.STOI_SEGMENT
timed = functools.partial(bench_timing.timed, warmup=5, host_clock=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stoi_bench.json"))
    args = ap.parse_args()
    bands = audio.third_octave_bands()
    nbin = int(bands[:, 1].max() - bands[:, 0].min())
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "window": W, "hop": H, "n_fft": NFFT, "bands": int(bands.shape[0]), "bins": nbin,
           "segment_frames": N, "shapes": {}}
    g = torch.Generator().manual_seed(0)
    eng = Engine(0)
    eng.load_stoi(audio.stoi_window(W), audio.stoi_twiddle(NFFT), bands, H, NFFT, N)
    for B, seconds in ((64, 6), (1, 6)):
        L = seconds * SR
        x = (0.1 * torch.randn(B, L, generator=g)).cuda()
        y = x + (0.1 * torch.randn(B, L, generator=g)).cuda()
        NF = -(-(L - W) // H)
        NSEG = NF - 1 - N + 1
        seg = torch.empty(B, NSEG, 2, dtype=torch.float64, device="cuda")
        score = torch.empty(B, 2, dtype=torch.float64, device="cuda")
        counts = torch.empty(B, 3, dtype=torch.int32, device="cuda")

        def measure():
            rc = eng.lib.ev_stoi(eng.h, x.data_ptr(), y.data_ptr(), None, B, L, audio.STOI_SILENCE_RATIO, audio.STOI_CLIP, None, None, seg.data_ptr(),
                                 score.data_ptr(), counts.data_ptr(), _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        measure()
        torch.cuda.synchronize()
        nk = int(counts[0, 1])
        fmas = B * (nk - 1) * 2 * W * nbin * 2                          # the DFT: re and im of every bin, both signals
        nbytes = 2 * 4 * B * L
        src, dst = torch.randn(2 * B * L, device="cuda"), torch.empty(2 * B * L, device="cuda")
        ts = timed(measure, args.calls)
        cp = timed(lambda: dst.copy_(src), args.calls)
        res["shapes"][f"B{B}_{seconds}s"] = {
            "samples_per_signal": B * L, "frames_row0": int(counts[0, 0]), "kept_frames_row0": nk, "segments_row0": int(counts[0, 2]),
            "stoi_row0": float(score[0, 0]), "estoi_row0": float(score[0, 1]), "input_bytes": nbytes, "dft_fmas": fmas, "ev_stoi": ts,
            "copy_of_the_inputs": cp, "ratio_of_medians": ts["median_ms"] / cp["median_ms"], "dft_tera_fma_per_second": fmas / (ts["median_ms"] * 1e-3) / 1e12,
            "audio_seconds_per_second": B * seconds / (ts["median_ms"] * 1e-3)}
        print(f"B={B} {seconds} s: ev_stoi {ts['median_ms']:.4f} ms (min {ts['min_ms']:.4f}, max {ts['max_ms']:.4f})  copy of the inputs {cp['median_ms']:.4f} ms  "
              f"ratio {ts['median_ms'] / cp['median_ms']:.1f}  {fmas / (ts['median_ms'] * 1e-3) / 1e12:.2f} T fma/s over the whole call  "
              f"({B * seconds / (ts['median_ms'] * 1e-3):.0f} s of audio per second; row 0: {nk} of {int(counts[0, 0])} frames kept, STOI {float(score[0, 0]):.4f} "
              f"ESTOI {float(score[0, 1]):.4f}; host clock, back to back: {ts['host_clock_back_to_back_ms']:.4f} / {cp['host_clock_back_to_back_ms']:.4f} ms)")
        del x, y, src, dst
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
