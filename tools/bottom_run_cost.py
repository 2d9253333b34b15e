#!/usr/bin/env python3
"""What BottomUKFBatch.run_log (uwvk_bottom_run_log, k_bottom_run) gains over the
single calls.

One 200-ping log, 4 beams every ping (per-instance variances) and a normal every
fifth ping, at batch 4,096 and 65,536, two ways on one handle:

  (a) run_log + synchronize: one launch for the 200 epochs;
  (b) the single-call loop (play_bottom_log: set_velocity, predict, 4 x
      update_range and every fifth ping update_normal, each with its host check,
      upload, launch and stream synchronisation): the only way to run that log
      without run_log, host copies included.

Both are timed by host wall clock (time.perf_counter around the calls, the
device idle before and after), interleaved in rounds after a warm-up round.
Prints one JSON line and writes it to --out: per batch the per-round
milliseconds, their medians, the ratio (b) / (a), whether (a) was the faster in
every round, and (a) per instance-epoch.

  python tools/bottom_run_cost.py --out profiles/bottom_run_cost.json
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

BEAMS = [([0.5, 0.0, -0.866], [0.1, 0.0, 0.0]), ([-0.5, 0.0, -0.866], [-0.1, 0.0, 0.0]),
         ([0.0, 0.5, -0.866], [0.0, 0.1, 0.0]), ([0.0, -0.5, -0.866], [0.0, -0.1, 0.0])]


def make_log(B, E, rng, rows=8):
    """rows: the range / normal payload rows the epochs cycle through"""
    e = np.arange(E)
    d = np.array([b[0] for b in BEAMS])
    flags = np.full(E, 0xF, np.uint32)
    flags[4::5] |= 0x100
    n = np.concatenate([rng.normal(0, 0.03, (rows, B, 2)), np.ones((rows, B, 1))], -1)
    return dict(epochs=E, dt=0.2, beams=4, flags=flags,
                velocity=np.stack([rng.normal(0.5, 0.1, (E, B)), rng.normal(0, 0.1, (E, B)),
                                   rng.normal(0, 0.05, (E, B))], -1),
                beam_direction=d / np.linalg.norm(d, axis=1, keepdims=True),
                beam_origin=np.array([b[1] for b in BEAMS]),
                range_index=(e % rows).astype(np.int32), range=10.0 / 0.866 + rng.normal(0, 0.05, (rows, 4, B)),
                range_var=rng.uniform(0.01, 0.03, (rows, 4, B)), range_cov=0.0,
                normal_index=((e // 5) % rows).astype(np.int32), normal=n, normal_cov=np.eye(2) * 4e-4)


def measure(B, E, rounds, warmup):
    from uwvk.small import BottomUKFBatch, play_bottom_log
    rng = np.random.default_rng(B)
    x = np.c_[10.0 + rng.uniform(-1, 1, B), rng.normal(0, 0.1, (B, 2)), np.ones(B)]
    P = np.tile(np.diag([0.3, 0.01, 0.01]), (B, 1, 1))
    log = make_log(B, E, rng)
    f = BottomUKFBatch(B)
    f.init(x, P)
    f.set_process_noise(np.diag([0.02, 0.001, 0.001]))
    dlog = f.upload_log(log)

    def run():
        f.run_log(dlog, sync=False)
        f.synchronize()

    def single():
        play_bottom_log(f, log)
        f.synchronize()

    ms = dict(run=[], single=[])
    for rnd in range(warmup + rounds):
        for name, fn in (("run", run), ("single", single)):
            f.synchronize()
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if rnd >= warmup:
                ms[name].append(round(t, 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(batch=B, ms=ms, median_ms=med, ratio_single_over_run=round(med["single"] / med["run"], 2),
                run_faster_every_round=all(a < b for a, b in zip(ms["run"], ms["single"])),
                run_ns_per_instance_epoch=round(med["run"] * 1e6 / (B * E), 4),
                status_or=int(np.bitwise_or.reduce(f.get_status())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--epochs", type=int, default=200, help="pings in the log")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1, help="untimed rounds")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = dict(tool="bottom_run_cost", epochs=a.epochs, beams=4, normal_every=5, rounds=a.rounds, warmup=a.warmup,
               timing="host wall clock, run_log + synchronize against play_bottom_log, interleaved rounds",
               results=[measure(B, a.epochs, a.rounds, a.warmup) for B in a.batches])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
