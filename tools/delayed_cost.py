#!/usr/bin/env python3
"""Cost of delayed XY fixes inside run_log (uwvk_pose_run_log_delayed: the
position latch k_pose_latch and the delayed kind of k_psp_fix).

C3 at batch 65,536, calls of 200 epochs with the delayed rows (latch, arrival) =
(49, 99) and (149, 199), three ways on one handle, interleaved in rounds after a
warm-up, timed with HIP events on the handle's stream (PoseUKFBatch.timer_start
/ timer_stop):

  (a) run_log with the delayed rows: one latch launch per latch epoch, one
      k_psp_fix launch per arrival epoch;
  (b) without the entry point: run_log cut at each latch epoch with the means
      read back (get_state_mu), and at each arrival epoch with
      uwvk_pose_update_delayed_xy on that position (an upload, a launch and a
      stream synchronisation);
  (c) run_log without delayed rows.

Prints one JSON line and writes it to --out: the per-round milliseconds, their
medians, (a) - (c) and (b) - (c) per sample, and whether (a) was faster than (b)
in every round.

  python tools/delayed_cost.py --out profiles/delayed_cost.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-uwv_kalman_filters_amd", "python"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--epochs", type=int, default=200, help="epochs per call")
    ap.add_argument("--every", type=int, default=100, help="a sample arrives every this many epochs")
    ap.add_argument("--delay", type=int, default=50, help="epochs between a sample's latch and its arrival")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1, help="untimed rounds")
    ap.add_argument("--dof", type=int, default=53)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from uwvk import engine, synth

    B, E = a.batch, a.epochs
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, E, "C3", dof=a.dof)
    arrivals = list(range(a.every - 1, E, a.every))
    rows = [(e - a.delay, e) for e in arrivals if e - a.delay >= 0]
    rng = np.random.default_rng(1)
    cov = np.eye(2) * 0.25
    dl = dict(index=np.full(E, -1, np.int32), latch_epoch=np.array([L for L, _ in rows], np.int32), xy_cov=cov,
              xy=np.empty((len(rows), B, 2)))
    for r, (L, A) in enumerate(rows):
        dl["index"][A] = r
        dl["xy"][r] = log["truth"].pos[L + 1][:2] + 0.5 * rng.standard_normal((B, 2))

    f = engine.PoseUKFBatch(B, a.dof)
    f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    f.set_process_noise_from_config(cfg, log["dt"])
    dlog, ddl = f.upload_log(log), f.upload_delayed(dl)
    kernels = dict(pair=f.pair_active(), param_block=f.param_block())

    def in_run():
        f.run_log(dlog, 0, E, delayed=ddl, sync=False)

    def cut():
        latched, first = {}, 0
        for e in sorted({L for L, _ in rows} | {A for _, A in rows}):
            f.run_log(dlog, first, e + 1 - first, sync=False)
            if dl["index"][e] >= 0:
                r = dl["index"][e]
                f.update("delayed_xy", dl["xy"][r], cov, extra=latched[r])
            for r, (L, _) in enumerate(rows):
                if L == e:
                    latched[r] = np.ascontiguousarray(f.get_state_mu()[:, 0:2])
            first = e + 1
        if first < E:
            f.run_log(dlog, first, E - first, sync=False)

    def plain():
        f.run_log(dlog, 0, E, sync=False)

    variants = (("in_run", in_run), ("cut", cut), ("plain", plain))
    ms = {k: [] for k, _ in variants}
    for rnd in range(a.warmup + a.rounds):
        for name, fn in variants:
            f.timer_start()
            fn()
            t = f.timer_stop()
            if rnd >= a.warmup:
                ms[name].append(round(t, 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in ms.items()}
    out = dict(tool="delayed_cost", batch=B, dof=a.dof, epochs=E, rows=rows, rounds=a.rounds,
               kernels_at_start=kernels, kernels_at_end=dict(pair=f.pair_active(), param_block=f.param_block()),
               ms=ms, median_ms=med, spread_ms=spread,
               in_run_minus_plain_ms_per_sample=round((med["in_run"] - med["plain"]) / len(rows), 4),
               cut_minus_plain_ms_per_sample=round((med["cut"] - med["plain"]) / len(rows), 4),
               in_run_faster_than_cut_every_round=all(x < y for x, y in zip(ms["in_run"], ms["cut"])),
               status_or=int(np.bitwise_or.reduce(f.get_status())))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
