#!/usr/bin/env python3
"""Time ev_formant_track at the report's setting (five candidates per frame tracked to three: S = 10 states) on the candidates ev_formants finds in
64 x 6 s and 1 x 6 s of audio at 11025 Hz, hop 128 (HIP events, median of N calls after warm-up), beside three yardsticks on the same rows:
  * ev_formants itself (W 512, H 128, order 13, five candidates), whose output is the tracker's input;
  * a device-to-device copy of the tracker's input (the least a call could cost: it reads every candidate once);
  * the numpy restatement of the definition (tests/formant_track_ref.py) on 16 CPU threads.

    python tools/formant_track_bench.py [--calls 30] [--cpu_calls 1] [--out profiles/formant_track_bench.json]

The call is latency-bound, not arithmetic: one workgroup per row walks its frames one after the other, one barrier each, and lane 0 then walks
the back-pointers of every segment; at B = 64 it occupies 64 of the 256 CUs, at B = 1 one.  "us_per_frame" is the call's time over the frames
of one row.  No figure is a gate.
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
import formant_track_ref as R  # noqa: E402
import formants_ref as F  # noqa: E402
from emojivoice_amd import audio  # noqa: E402
from emojivoice_amd._lib import Engine, _stream_ptr  # noqa: E402

SR, SECONDS, CPU_THREADS = 11025, 6, 16
W, H, ORDER, F_LO = 512, 128, 13, 50.0
N_CAND, N_TRACKS = 5, 3
FLOOR = audio.FORMANT_POWER_FLOOR
timed = functools.partial(bench_timing.timed, warmup=3, host_clock=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--cpu_calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "formant_track_bench.json"))
    args = ap.parse_args()
    torch.set_num_threads(CPU_THREADS)
    L = SECONDS * SR
    NF = -(-L // H)
    S = R.n_states(N_CAND, N_TRACKS)
    pre = float(np.exp(-2.0 * np.pi * 50.0 / SR))
    ref = np.asarray(audio.FORMANT_TRACK_REFERENCE, dtype=np.float64)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "seconds": SECONDS, "samples": L, "W": W, "H": H, "order": ORDER,
           "candidates": N_CAND, "tracks": N_TRACKS, "states": S, "reference_hz": ref.tolist(), "costs": [1.0, 1.0, 1.0], "cpu_threads": CPU_THREADS,
           "shapes": {}}
    eng = Engine(0)
    eng.load_formants(audio.formant_window(W), H, ORDER, pre, float(SR), F_LO, N_CAND)
    for B in (64, 1):
        x = torch.from_numpy(np.stack([F.speech_like(L, seed=1 + b, fs=SR) for b in range(B)])).cuda()
        fm = torch.empty(B, NF, N_CAND, 2, dtype=torch.float64, device="cuda")
        ct = torch.empty(B, NF, dtype=torch.int32, device="cuda")
        back = torch.empty(B, NF, S, dtype=torch.int16, device="cuda")
        track = torch.empty(B, NF, N_TRACKS, 2, dtype=torch.float64, device="cuda")
        sel = torch.empty(B, NF, dtype=torch.int32, device="cuda")
        cost = torch.empty(B, NF, dtype=torch.float64, device="cuda")
        dst = torch.empty_like(fm)

        def call_fm():
            rc = eng.lib.ev_formants(eng.h, x.data_ptr(), None, B, L, FLOOR, None, fm.data_ptr(), ct.data_ptr(), _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        def call_track():
            rc = eng.lib.ev_formant_track(eng.h, fm.data_ptr(), ct.data_ptr(), B, NF, N_CAND, N_TRACKS, ref.ctypes.data, 1.0, 1.0, 1.0, back.data_ptr(),
                                          track.data_ptr(), sel.data_ptr(), cost.data_ptr(), _stream_ptr())
            assert rc == 0, eng.lib.ev_last_error(eng.h).decode()

        tf = timed(call_fm, args.calls)
        tt, tcp = timed(call_track, args.calls), timed(lambda: dst.copy_(fm), args.calls)
        fm_h, ct_h = fm.cpu().numpy(), ct.cpu().numpy()
        cpu_ms = []
        for _ in range(args.cpu_calls + 1):                               # (the first is the warm-up)
            t0 = time.perf_counter()
            rt, rs, rc_, _, margin = R.batch(fm_h, ct_h, N_TRACKS)
            cpu_ms.append((time.perf_counter() - t0) * 1e3)
        cpu = statistics.median(cpu_ms[1:])
        ds, dt, dc = sel.cpu().numpy(), track.cpu().numpy(), cost.cpu().numpy()
        tracked = rs >= 0
        other = tracked & (rt[..., 0] != fm_h[:, :, :N_TRACKS, 0]).any(axis=-1)
        ends = tracked & np.concatenate([~tracked[:, 1:], np.ones((B, 1), bool)], axis=1)
        shape = {"rows": B, "frames_per_row": NF, "workgroups": B, "threads_per_workgroup": 64, "ev_formant_track": tt, "ev_formants_same_rows": tf,
                 "device_to_device_copy_of_the_input": tcp, "track_over_formants": tt["median_ms"] / tf["median_ms"],
                 "track_over_copy": tt["median_ms"] / tcp["median_ms"], "us_per_frame": tt["median_ms"] * 1e3 / NF,
                 "numpy_restatement_cpu_ms": cpu, "cpu_over_device": cpu / tt["median_ms"], "tracked_frames": int(tracked.sum()), "frames": int(tracked.size),
                 "segments": int(ends.sum()), "frames_with_another_assignment_than_lowest_n": int(other.sum()),
                 "frames_with_equal_selection": int((ds == rs).sum()), "tracks_equal_to_the_restatement": bool(np.array_equal(dt, rt)),
                 "worst_error_d_cost": R.err(dc, rc_), "least_decision_margin": float(margin.min()),
                 "audio_seconds_per_second": B * SECONDS / (tt["median_ms"] * 1e-3)}
        res["shapes"][f"B{B}_{SECONDS}s"] = shape
        print(f"B={B} {SR} Hz hop {H}, {N_CAND} candidates -> {N_TRACKS} tracks (S = {S}): ev_formant_track {tt['median_ms']:.3f} ms (min {tt['min_ms']:.3f}, max "
              f"{tt['max_ms']:.3f}; {shape['us_per_frame']:.2f} us a frame)  ev_formants {tf['median_ms']:.3f} ms  copy {tcp['median_ms']:.4f} ms  numpy on "
              f"{CPU_THREADS} threads {cpu:.1f} ms ({cpu / tt['median_ms']:.0f} x)  tracked {shape['tracked_frames']} of {shape['frames']} frames in "
              f"{shape['segments']} segments, another assignment than lowest-n on {shape['frames_with_another_assignment_than_lowest_n']}; device against CPU: "
              f"selection equal on {shape['frames_with_equal_selection']}, d_cost {shape['worst_error_d_cost']:.2e}, least margin {shape['least_decision_margin']:.2e}")
        del x, dst
    eng.close()
    bench_timing.write_json(args.out, res)


if __name__ == "__main__":
    main()
