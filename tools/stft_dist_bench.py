#!/usr/bin/env python3
"""Time ev_stft_dist at the three published resolutions (HIP events, median of N calls after warm-up) beside the same metric from
torch.stft in float64 on 16 CPU threads.

    python tools/stft_dist_bench.py [--calls 10] [--cpu_calls 2] [--out profiles/stft_dist_bench.json]

Shape: B = 64 rows of 6 s at 22050 Hz (132 300 samples), Gaussian noise against itself at 20 dB SNR, the resolutions of
audio.MSTFT_RESOLUTIONS.  The call is arithmetic: per row, frame, window sample and bin four float64 fmas (both signals times both basis
planes) — 4.73 G fmas a row over the three resolutions, 303 G at B = 64.  The achieved rate below counts those USEFUL fmas (2 flops each)
over the whole call's event time; the matrix instructions also compute the bins that pad NB = nfft / 2 + 1 to a multiple of 16 and the
frames that pad a row's last tile, which the rate does not credit.  The guides give no float64 roof for the matrix cores and none has been
measured here, so no share of peak is stated and no figure is a gate.  The script also records how far the device's figures are from the
CPU's (float64 order effects) and, for B = 1, what one row costs: 35 to 166 workgroups do not fill the chip.
"""
import argparse
import functools
import math
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_timing  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, SECONDS, CPU_THREADS = 22050, 6, 16
timed = functools.partial(bench_timing.timed, warmup=3, host_clock=True)


def cpu_metric(x, y, nfft, hop, win):
    """(sc, log_mag, lsd_db) per row from torch.stft in float64: the definition audio.stft_distance states."""
    w = torch.hann_window(win, dtype=torch.float64)
    p = []
    for s in (x, y):
        z = torch.stft(s.double(), nfft, hop_length=hop, win_length=win, window=w, center=True, pad_mode="reflect", return_complex=True)
        p.append(torch.clamp(z.real ** 2 + z.imag ** 2, min=audio.MSTFT_POWER_FLOOR))
    mx, my = p[0].sqrt(), p[1].sqrt()
    dl = p[1].log() - p[0].log()
    sc = ((my - mx) ** 2).sum((1, 2)).sqrt() / (mx ** 2).sum((1, 2)).sqrt()
    return sc, 0.5 * dl.abs().mean((1, 2)), (10.0 / math.log(10.0)) * (dl ** 2).mean(1).sqrt().mean(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cpu_calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stft_dist_bench.json"))
    args = ap.parse_args()
    torch.set_num_threads(CPU_THREADS)
    L = SECONDS * SR
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "seconds": SECONDS, "samples": L, "power_floor": audio.MSTFT_POWER_FLOOR,
           "cpu_threads": CPU_THREADS, "float64_matrix_roof": "not stated by the guides, not measured", "shapes": {}}
    g = torch.Generator().manual_seed(0)
    engines = {}
    for nfft, hop, win in audio.MSTFT_RESOLUTIONS:
        engines[(nfft, hop, win)] = e = Engine(0)
        e.load_stft_dist(audio.stft_dist_window(win), audio.stoi_twiddle(nfft), hop, nfft)
    for B in (64, 1):
        x_h = 0.1 * torch.randn(B, L, generator=g)
        y_h = x_h + 0.01 * torch.randn(B, L, generator=g)
        x, y = x_h.cuda(), y_h.cuda()
        shape = {"rows": B, "resolutions": {}}
        total_ms = total_cpu = total_fma = 0.0
        for (nfft, hop, win), e in engines.items():
            NB, nf = nfft // 2 + 1, 1 + L // hop
            sums = torch.empty(B, 4, dtype=torch.float64, device="cuda")
            counts = torch.empty(B, dtype=torch.int32, device="cuda")

            def measure():
                rc = e.lib.ev_stft_dist(e.h, x.data_ptr(), y.data_ptr(), None, B, L, audio.MSTFT_POWER_FLOOR, None, sums.data_ptr(), counts.data_ptr(),
                                        _stream_ptr())
                assert rc == 0, e.lib.ev_last_error(e.h).decode()

            ts = timed(measure, args.calls)
            assert int(counts[0]) == nf
            s = sums.cpu()
            dev = (torch.sqrt(s[:, 0] / s[:, 1]), 0.5 * s[:, 2] / (nf * NB), (10.0 / math.log(10.0)) * s[:, 3] / nf)
            cpu_ms = []
            for _ in range(args.cpu_calls + 1):                           # (the first is the warm-up)
                t0 = time.perf_counter()
                ref = cpu_metric(x_h, y_h, nfft, hop, win)
                cpu_ms.append((time.perf_counter() - t0) * 1e3)
            cpu = statistics.median(cpu_ms[1:])
            diff = max(float(((d - r).abs() / r.abs()).max()) for d, r in zip(dev, ref))
            fmas = B * nf * win * NB * 4
            tiles = B * -(-nf // 16)
            shape["resolutions"][f"{nfft}_{hop}_{win}"] = {
                "frames_per_row": nf, "bins": NB, "workgroups": tiles, "useful_fmas": fmas, "ev_stft_dist": ts,
                "useful_float64_tflops": 2.0 * fmas / (ts["median_ms"] * 1e-3) / 1e12, "torch_stft_float64_cpu_ms": cpu,
                "cpu_over_device": cpu / ts["median_ms"], "worst_relative_difference_device_against_cpu": diff,
                "row0": {"sc": float(dev[0][0]), "log_mag": float(dev[1][0]), "lsd_db": float(dev[2][0])}}
            total_ms += ts["median_ms"]
            total_cpu += cpu
            total_fma += fmas
            print(f"B={B} {nfft}/{hop}/{win}: ev_stft_dist {ts['median_ms']:.3f} ms (min {ts['min_ms']:.3f}, max {ts['max_ms']:.3f}; host clock back to back "
                  f"{ts['host_clock_back_to_back_ms']:.3f})  {2.0 * fmas / (ts['median_ms'] * 1e-3) / 1e12:.2f} useful float64 TFLOP/s  {tiles} workgroups  "
                  f"torch.stft float64 on {CPU_THREADS} CPU threads {cpu:.1f} ms ({cpu / ts['median_ms']:.0f} x)  device against CPU {diff:.2e}  "
                  f"row 0: sc {float(dev[0][0]):.5f} log_mag {float(dev[1][0]):.5f} lsd {float(dev[2][0]):.4f} dB")
        shape["three_resolutions"] = {"ev_stft_dist_ms": total_ms, "torch_stft_float64_cpu_ms": total_cpu, "useful_fmas": total_fma,
                                      "useful_float64_tflops": 2.0 * total_fma / (total_ms * 1e-3) / 1e12,
                                      "audio_seconds_per_second": B * SECONDS / (total_ms * 1e-3)}
        print(f"B={B} three resolutions: {total_ms:.3f} ms on the device, {total_cpu:.1f} ms on the CPU, {2.0 * total_fma / (total_ms * 1e-3) / 1e12:.2f} useful "
              f"float64 TFLOP/s, {B * SECONDS / (total_ms * 1e-3):.0f} s of audio per second")
        res["shapes"][f"B{B}_{SECONDS}s"] = shape
        del x, y
    for e in engines.values():
        e.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
