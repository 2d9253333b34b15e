#!/usr/bin/env python3
"""What IndirectPoseUKFBatch.run_log (uwvk_ipose_run_log, k_ipose_run) gains over
the single calls.

One 200-epoch marker-localisation log: a new pose reference every epoch and one
4-feature marker observation every second epoch (per-instance marker poses, a
shared pixel covariance), at batch 4,096 and 65,536, two ways on one handle:

  (a) run_log + synchronize: one launch for the 200 epochs;
  (b) the single-call loop (play_ipose_log: set_pose_reference, predict and
      every second epoch update_visual, each with its host check, upload, launch
      and stream synchronisation): the only way to run that log without
      run_log, host copies included.

Both are timed by host wall clock (time.perf_counter around the calls, the
device idle before and after), interleaved in rounds after a warm-up round.
Prints one JSON line and writes it to --out: per batch the per-round
milliseconds, their medians, the ratio (b) / (a), whether (a) was the faster in
every round, and (a) per instance-epoch.

  python tools/ipose_run_cost.py --out profiles/ipose_run_cost.json
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

CAMERA = np.array([600.0, 620.0, 320.0, 240.0])
CAM_IN_BODY = np.array([0.1, 0.0, 0.05, 0.5, -0.5, 0.5, -0.5])  # z_cam = x_body, x_cam = -y_body, y_cam = -z_body
CORNERS = 0.2 * np.array([[1.0, 1.0, 0.0], [-1.0, 1.0, 0.0], [-1.0, -1.0, 0.0], [1.0, -1.0, 0.0]])
PIXEL_VAR = 4.0
INIT = dict(pos_std=[0.1, 0.1, 0.2], ori_std=[0.01, 0.01, 0.02], tau=20.0, init_pos_std=[0.5, 0.5, 0.5])


def qmul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx], -1)


def qrot(q, v, inv=False):
    q = q * np.array([1.0, -1.0, -1.0, -1.0]) if inv else q
    qv = np.concatenate([np.zeros(v.shape[:-1] + (1,)), v], -1)
    return qmul(qmul(q, qv), q * np.array([1.0, -1.0, -1.0, -1.0]))[..., 1:]


def qexp(rv):
    th = np.linalg.norm(rv, axis=-1, keepdims=True)
    s = np.where(th > 0, np.sin(th / 2) / np.where(th > 0, th, 1), 0.5)
    return np.concatenate([np.cos(th / 2), s * rv], -1)


def make_log(B, E, rng, every=2):
    """A marker 3 m ahead of each true body pose (reference * a small pose error),
    its four corners projected through the camera plus 0.3 px noise per row; the
    references and the markers drift together, so the pixels stay valid."""
    ref_t, ref_q = rng.normal(0, 5, (B, 3)), qexp(rng.normal(0, 0.3, (B, 3)))
    body_t = ref_t + qrot(ref_q, rng.normal(0, 0.3, (B, 3)))
    body_q = qmul(ref_q, qexp(rng.normal(0, 0.02, (B, 3))))
    marker_t = body_t + qrot(body_q, np.broadcast_to([3.0, 0.0, 0.0], (B, 3)))
    fn = qrot(body_q[:, None], CORNERS[None]) + marker_t[:, None]
    w = qrot(body_q[:, None], fn - body_t[:, None], inv=True) - CAM_IN_BODY[:3]
    fc = qrot(np.broadcast_to(CAM_IN_BODY[3:], w.shape[:-1] + (4,)), w, inv=True)
    px = np.stack([CAMERA[0] * fc[..., 0] / fc[..., 2] + CAMERA[2], CAMERA[1] * fc[..., 1] / fc[..., 2] + CAMERA[3]], -1)
    rows = np.arange(every - 1, E, every)          # the epochs that hold a row
    drift = np.array([0.03, -0.02, 0.005])
    off = np.zeros(E + 1, np.int64)
    off[1:] = np.cumsum(np.isin(np.arange(E), rows))
    pose_ref = np.empty((E, B, 7))
    pose_ref[..., :3] = ref_t + drift * np.arange(E)[:, None, None]
    pose_ref[..., 3:] = ref_q
    marker = np.empty((len(rows), B, 7))
    marker[..., :3] = marker_t + drift * rows[:, None, None]
    marker[..., 3:] = body_q
    return dict(batch=B, epochs=E, dt=0.1, dt_epoch=None, pose_ref=pose_ref, visual_offset=off, n_features=4,
                features=px + rng.normal(0, 0.3, (len(rows), B, 4, 2)), feature_cov=None,
                shared_feature_cov=np.tile(np.eye(2).reshape(4) * PIXEL_VAR, (4, 1)), feature_positions=CORNERS,
                marker_pose=marker, shared_marker_pose=None,
                cov_marker_pose=np.diag([1e-4] * 3 + [1e-5] * 3), camera=CAMERA, camera_in_body=CAM_IN_BODY)


def measure(B, E, rounds, warmup):
    from uwvk.small import IndirectPoseUKFBatch, play_ipose_log
    rng = np.random.default_rng(B)
    log = make_log(B, E, rng)
    f = IndirectPoseUKFBatch(B)
    f.init(INIT["pos_std"], INIT["ori_std"], INIT["tau"], rng.normal(0, 0.1, (B, 3)), INIT["init_pos_std"])
    dlog = f.upload_log(log)

    def run():
        f.run_log(dlog, sync=False)
        f.synchronize()

    def single():
        play_ipose_log(f, log)
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
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1, help="untimed rounds")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = dict(tool="ipose_run_cost", epochs=a.epochs, features=4, visual_every=2, rounds=a.rounds, warmup=a.warmup,
               timing="host wall clock, run_log + synchronize against play_ipose_log, interleaved rounds",
               results=[measure(B, a.epochs, a.rounds, a.warmup) for B in a.batches])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
