#!/usr/bin/env python3
"""What VelocityUKFBatch.run_log_track (uwvk_vel_run_log_track) costs beside the
plain run_log, and what its in-launch records save.

The C2 log (synth.make_vel_log: 1 kHz gyro + efforts, 5 Hz DVL, 10 Hz depth),
1,000 epochs, at batch 4,096 (the 16-lane-row kernel) and 65,536 (the
lane-per-filter kernel; the 4,096 instances' columns repeated), four ways on one
handle, each from the same initial state:

  (a) run_log + synchronize: the plain kernels;
  (b) run_log_track without a track: the screened kernels, i.e. what the
      per-instance finite tests and branches cost;
  (c) run_log_track with mean + variance records every 10 epochs, written by
      the epoch kernel into device buffers (allocated and freed inside the
      timed call, as a caller of the Python method pays for them);
  (d) what the same records cost without it: run_log cut every 10 epochs with
      get_state (a stream synchronisation and a host copy of x and P) at each cut.

All timed by host wall clock (time.perf_counter around the calls, the device
idle before and after), interleaved in rounds after a warm-up round.  Prints
one JSON line and writes it to --out: per batch the per-round milliseconds,
their medians, the ratios (b)/(a), (c)/(a) and (d)/(c), and whether (c) was
faster than (d) in every round.  same_final_state compares (x, P) of all four
ways bitwise; on the row layout way (d) can differ from the others in the last
bits (every cut reloads the side lane's replica of Sigma into all lanes,
DESIGN.md section 9), (a), (b) and (c) agree (tests/test_gpu_vel_track.py).

  python tools/vel_run_cost.py --out profiles/vel_run_cost.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-uwv_kalman_filters_amd", "python"))

GENERATED = 4096  # instances generated; larger batches repeat their columns


def make_log(B, E):
    from uwvk import synth
    log = synth.make_vel_log(min(B, GENERATED), E)
    if B > GENERATED:
        idx = np.arange(B) % GENERATED
        log = dict(log, batch=B, x0=log["x0"][idx], P0=log["P0"][idx],
                   **{k: np.ascontiguousarray(log[k][:, idx]) for k in ("gyro", "efforts", "dvl", "pressure")})
    return log


def measure(B, E, every, rounds, warmup):
    from uwvk import engine, synth
    log = make_log(B, E)
    f = engine.VelocityUKFBatch(B)
    uwv = synth.default_uwv()
    dlog = f.upload_log(log)

    def reset():
        f.init(log["x0"], log["P0"])
        f.set_gyro(log["gyro"][0])
        f.setup_motion_model(uwv)
        f.get_status(clear=True)

    def plain():
        f.run_log(dlog, sync=False)
        f.synchronize()

    def screened():
        f.run_log_track(dlog, sync=False)
        f.synchronize()

    def track():
        t = f.run_log_track(dlog, every, sync=False)
        f.synchronize()
        return t

    def cut():
        for first in range(0, E, every):
            f.run_log(dlog, first, min(every, E - first), sync=False)
            if first + every <= E:
                f.get_state()
        f.synchronize()

    ways = (("plain", plain), ("screened", screened), ("track", track), ("cut", cut))
    ms = {name: [] for name, _ in ways}
    final = {}
    for rnd in range(warmup + rounds):
        for name, fn in ways:
            reset()
            f.synchronize()
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if rnd >= warmup:
                ms[name].append(round(t, 4))
            final[name] = f.get_state()
    med = {k: statistics.median(v) for k, v in ms.items()}
    layout = "row" if B <= 30720 else "lane"
    return dict(batch=B, layout=layout, ms=ms, median_ms=med,
                ratio_screened_over_plain=round(med["screened"] / med["plain"], 4),
                ratio_track_over_plain=round(med["track"] / med["plain"], 4),
                ratio_cut_over_track=round(med["cut"] / med["track"], 2),
                track_faster_than_cut_every_round=all(a < b for a, b in zip(ms["track"], ms["cut"])),
                plain_ns_per_instance_epoch=round(med["plain"] * 1e6 / (B * E), 4),
                same_final_state=all(np.array_equal(final["plain"][k], final[n][k]) for n in final for k in (0, 1)),
                status_or=int(np.bitwise_or.reduce(f.get_status())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--every", type=int, default=10, help="record stride of (c) and (d)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1, help="untimed rounds")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = dict(tool="vel_run_cost", log="C2 (synth.make_vel_log)", epochs=a.epochs, every=a.every, rounds=a.rounds,
               warmup=a.warmup,
               timing="host wall clock around the calls + synchronize, device idle before, interleaved rounds",
               ways=dict(plain="run_log", screened="run_log_track, no track",
                         track="run_log_track, mean + variance every `every`",
                         cut="run_log cut every `every` epochs + get_state at each cut"),
               results=[measure(B, a.epochs, a.every, a.rounds, a.warmup) for B in a.batches])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
