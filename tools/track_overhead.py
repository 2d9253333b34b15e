#!/usr/bin/env python3
"""What a track costs: uwvk_pose_run_log against uwvk_pose_run_log_track at
several strides, timed with the handle's event timer (timer_start / timer_stop
on its stream), on the C3 shape of the benchmark (batch 65,536, 53 DOF, 2,000
epochs by default).

Per stride two tracked variants: the means and variances of every instance
(mean+variance) and the ensemble statistics alone (stats).  The variants run
alternately, `--rounds` times in one process, after one untimed pass of each.
Every run replays epochs [0, E) of the same log on the state the run before it
left (a C3 log has no BodyEfforts epoch, so the kernel choice never changes);
the track's buffers are allocated before the timer starts.  Prints one JSON
line per run and a markdown table of the median rates, the spread between
rounds and the overhead against the untracked run of the same round."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-uwv_kalman_filters_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--dof", type=int, default=53)
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--every", default="1000,100,10")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from uwvk import abi, engine, synth
    if not engine.device_available(0):
        sys.exit("track_overhead: no gfx950 device")
    B, E, dof = a.batch, a.epochs, a.dof
    strides = [int(s) for s in a.every.split(",")]
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, E, "C3", dof=dof)
    f = engine.PoseUKFBatch(B, dof)
    f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    f.set_process_noise_from_config(cfg, log["dt"])
    dlog = f.upload_log(log)
    store, nout = f.lay["store"], 3 * f.lay["store"] + 2
    truth_all = log["truth"]
    del log

    def timed(every, what):
        """ms of one run over [0, E); every = 0: the untracked run_log"""
        bufs, tr, truth = [], None, None
        if every:
            n = f.track_records(0, E, every)
            tr = abi.PoseTrack()
            tr.every, tr.capacity = every, n
            for name, per in (("mean", B * store), ("variance", B * dof)) if what == "mean+variance" else \
                    (("stats", nout),):
                bufs.append(engine.DeviceBuffer.empty(n * per * 8))
                setattr(tr, name, bufs[-1].ptr)
            if what == "stats":
                truth = np.array([truth_all.state(e + 1, dof) for e in range(every - 1, E, every)])
                tr.truth = truth.ctypes.data_as(C.c_void_p)
        f.synchronize()
        f.timer_start()
        if every:
            engine._chk(f.L.uwvk_pose_run_log_track(f.h, C.byref(dlog.s), C.c_int64(0), C.c_int64(E), None,
                                                    C.byref(tr)), "run_log_track")
        else:
            f.run_log(dlog, 0, E, sync=False)
        ms = f.timer_stop()
        for b in bufs:
            b.free()
        return ms

    variants = [(0, "none")] + [(s, w) for s in strides for w in ("mean+variance", "stats")]
    for v in variants:  # code objects, first-touch of the buffers
        timed(*v)
    ms = {v: [] for v in variants}
    for r in range(a.rounds):
        for v in variants:
            t = timed(*v)
            ms[v].append(t)
            print(json.dumps(dict(round=r, every=v[0], track=v[1], ms=round(t, 3),
                                  msteps_per_s=round(B * E / t / 1e3, 2))), flush=True)
    if f.get_status().any():
        sys.exit("track_overhead: instances flagged")
    rate = lambda t: B * E / t / 1e3  # noqa: E731  (M filter steps per second)
    print("\nbatch %d, %d DOF, %d epochs, %d rounds (M steps/s: median, min..max)\n" % (B, dof, E, a.rounds))
    print("| every | records | track | M steps/s | min..max | overhead |")
    print("|---|---|---|---|---|---|")
    base = np.array(ms[(0, "none")])
    for v in variants:
        t = np.array(ms[v])
        over = np.median(t / base - 1.0) * 100.0  # against the untracked run of the same round
        print("| %s | %d | %s | %.1f | %.1f..%.1f | %s |" % (
            v[0] or "-", f.track_records(0, E, v[0]) if v[0] else 0, v[1], rate(np.median(t)), rate(t.max()),
            rate(t.min()), "%+.1f %%" % over if v[0] else "-"))


if __name__ == "__main__":
    main()
