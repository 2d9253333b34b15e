#!/usr/bin/env python3
"""Cost of position fixes inside run_log (uwvk_pose_run_log_fixes, k_psp_fix).

C3 at batch 65,536, calls of 200 epochs with an XY + Z fix every 100 epochs,
three ways on one handle, interleaved in rounds after a warm-up, timed with HIP
events on the handle's stream (PoseUKFBatch.timer_start / timer_stop):

  (a) run_log with fixes: one fused k_psp_fix launch per fix epoch;
  (b) run_log cut at the fix epochs with the host update calls
      (uwvk_pose_update_xy / _z: an upload, a launch and a stream
      synchronisation each) at the cuts;
  (c) run_log without fixes.

Prints one JSON line and writes it to --out: the per-round milliseconds, their
medians, (a) - (c) per fix epoch and whether (a) was faster than (b) in every
round.

  python tools/fix_cost.py --out profiles/fix_cost.json
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
    ap.add_argument("--fix-every", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1, help="untimed rounds")
    ap.add_argument("--dof", type=int, default=53)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from uwvk import abi, engine, synth

    B, E = a.batch, a.epochs
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, E, "C3", dof=a.dof)
    fix_epochs = list(range(a.fix_every - 1, E, a.fix_every))
    rng = np.random.default_rng(1)
    fx = dict(flags=np.zeros(E, np.uint32), xy_index=np.full(E, -1, np.int32), z_index=np.full(E, -1, np.int32),
              xy=np.empty((len(fix_epochs), B, 2)), z=np.empty((len(fix_epochs), B)),
              xy_cov=np.eye(2) * 0.25, z_cov=np.array([0.04]))
    for r, e in enumerate(fix_epochs):
        p = log["truth"].pos[e + 1]
        fx["flags"][e] = abi.FIX_XY | abi.FIX_Z
        fx["xy_index"][e] = fx["z_index"][e] = r
        fx["xy"][r] = p[:2] + 0.5 * rng.standard_normal((B, 2))
        fx["z"][r] = p[2] + 0.2 * rng.standard_normal(B)

    f = engine.PoseUKFBatch(B, a.dof)
    f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    f.set_process_noise_from_config(cfg, log["dt"])
    dlog, dfx = f.upload_log(log), f.upload_fixes(fx)
    kernels = dict(pair=f.pair_active(), param_block=f.param_block())

    def fused():
        f.run_log(dlog, 0, E, fixes=dfx, sync=False)

    def cut():
        first = 0
        for r, e in enumerate(fix_epochs):
            f.run_log(dlog, first, e + 1 - first, sync=False)
            f.update("xy", fx["xy"][r], fx["xy_cov"])
            f.update("z", fx["z"][r][:, None], fx["z_cov"].reshape(1, 1))
            first = e + 1
        if first < E:
            f.run_log(dlog, first, E - first, sync=False)

    def plain():
        f.run_log(dlog, 0, E, sync=False)

    variants = (("fused", fused), ("cut", cut), ("plain", plain))
    ms = {k: [] for k, _ in variants}
    for rnd in range(a.warmup + a.rounds):
        for name, fn in variants:
            f.timer_start()
            fn()
            t = f.timer_stop()
            if rnd >= a.warmup:
                ms[name].append(round(t, 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(tool="fix_cost", batch=B, dof=a.dof, epochs=E, fix_epochs=fix_epochs, kinds="XY+Z", rounds=a.rounds,
               kernels_at_start=kernels, kernels_at_end=dict(pair=f.pair_active(), param_block=f.param_block()),
               ms=ms, median_ms=med,
               fused_minus_plain_ms_per_fix_epoch=round((med["fused"] - med["plain"]) / len(fix_epochs), 4),
               cut_minus_plain_ms_per_fix_epoch=round((med["cut"] - med["plain"]) / len(fix_epochs), 4),
               fused_faster_than_cut_every_round=all(x < y for x, y in zip(ms["fused"], ms["cut"])),
               status_or=int(np.bitwise_or.reduce(f.get_status())))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
