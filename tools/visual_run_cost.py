#!/usr/bin/env python3
"""Cost of visual-landmark rows inside run_log (uwvk_pose_run_log_visual: one
k_pose_visual_run launch per visual epoch, the payload in device memory)
against the cut loop it replaces.

C3, calls of 200 epochs with a 4-feature row every 10th epoch (one row per
visual epoch, and a second variant with two), at each batch two ways on one
handle, interleaved in rounds after a warm-up, timed on the host (wall clock
from the first call to the end of a final synchronize):

  (a) in_run: run_log with the visual rows;
  (b) cut: run_log cut after every visual epoch with one
      uwvk_pose_update_visual_landmark per row (host arrays, a NaN check over
      the batch, an H2D copy, a launch and a stream synchronisation each).

The handle is put back to the same initial state before every timed run (not
timed), so both ways run the same kernels on the same numbers: parameter
decoupled until the first row, the general kernel after it.  The rows are made
once, before the rounds, by a cut run on the GPU: at each visual epoch a marker
3 m ahead of every instance's current estimate and the pinhole projection of
its corners from a pose near it (pixel noise 0.3 px), so every corner is ahead
of the camera.

Prints one JSON line and writes it to --out: per batch and variant the
per-round milliseconds of both ways, their medians, the saving per visual
epoch, and whether (a) was faster than (b) in every round.

  python tools/visual_run_cost.py --out profiles/visual_run_cost.json
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

CAMERA = np.array([600.0, 620.0, 320.0, 240.0])  # fx, fy, cx, cy
CORNERS = 0.2 * np.array([[1.0, 1.0, 0.0], [-1.0, 1.0, 0.0], [-1.0, -1.0, 0.0], [1.0, -1.0, 0.0]])
# camera in IMU: 10 cm ahead, 5 cm up, z_cam = x_body, x_cam = -y_body, y_cam = -z_body
CAM_IN_IMU = np.array([0.1, 0.0, 0.05, 0.5, -0.5, 0.5, -0.5])
COV_MARKER = np.diag([1e-4] * 3 + [1e-5] * 3)
FCOV = np.tile(np.eye(2) * 0.09, (4, 1, 1))


def qmul(a, b):
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx], -1)


def qrot(q, v):
    qv = np.concatenate([np.zeros(v.shape[:-1] + (1,)), v], -1)
    return qmul(qmul(q, qv), q * np.array([1.0, -1.0, -1.0, -1.0]))[..., 1:]


def make_row(x, rng):
    """(marker [B][7], pixels [B][4][2]) for the estimates x: the marker 3 m
    ahead of a true pose 0.2 m (sigma) and 0.01 rad off the estimate."""
    B = len(x)
    t = x[:, :3] + rng.normal(0, 0.2, (B, 3))
    rv = rng.normal(0, 0.01, (B, 3))
    th = np.linalg.norm(rv, axis=1, keepdims=True)
    q = qmul(np.concatenate([np.cos(th / 2), np.sin(th / 2) / th * rv], 1), x[:, 3:7])
    marker = np.concatenate([t + qrot(q, np.broadcast_to([3.0, 0.0, 0.0], t.shape)), q], 1)
    conj = np.array([1.0, -1.0, -1.0, -1.0])
    fn = qrot(marker[:, None, 3:], CORNERS[None]) + marker[:, None, :3]
    w = qrot(q[:, None] * conj, fn - t[:, None]) - CAM_IN_IMU[:3]
    fc = qrot(np.broadcast_to(CAM_IN_IMU[3:] * conj, w.shape[:-1] + (4,)), w)
    if not (fc[..., 2] > 1.0).all():
        raise RuntimeError("a corner is not ahead of the camera")
    px = np.stack([CAMERA[0] * fc[..., 0] / fc[..., 2] + CAMERA[2], CAMERA[1] * fc[..., 1] / fc[..., 2] + CAMERA[3]], -1)
    return marker, px + 0.3 * rng.standard_normal(px.shape)


def measure(engine, synth, B, E, every, rows_per_epoch, rounds, warmup, dof):
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, E, "C3", dof=dof)
    vis_epochs = list(range(every - 1, E, every))
    per = np.zeros(E, np.int64)
    per[vis_epochs] = rows_per_epoch
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    f = engine.PoseUKFBatch(B, dof)

    def reset():
        f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
        f.set_process_noise_from_config(cfg, log["dt"])
        f.synchronize()

    dlog = f.upload_log(log)
    cuts = [0] + [e + 1 for e in vis_epochs] + ([E] if vis_epochs[-1] + 1 < E else [])
    # the rows, from a cut run on the GPU
    rng = np.random.default_rng(1)
    feats, markers = [], []
    reset()
    kernels = dict(pair=f.pair_active(), param_block=f.param_block())
    for a, b in zip(cuts[:-1], cuts[1:]):
        f.run_log(dlog, a, b - a)
        for r in range(off[b - 1], off[b]):
            marker, px = make_row(f.get_state_mu(), rng)
            f.update_visual(px, FCOV, CORNERS, marker, COV_MARKER, CAMERA, CAM_IN_IMU)
            feats.append(px)
            markers.append(marker)
    feats, markers = np.array(feats), np.array(markers)
    scene_status = int(np.bitwise_or.reduce(f.get_status(clear=True)))
    vis = dict(visual_offset=off, n_features=4, features=feats, shared_feature_cov=FCOV.reshape(4, 4),
               feature_positions=CORNERS, marker_pose=markers, cov_marker_pose=COV_MARKER, camera=CAMERA,
               camera_in_imu=CAM_IN_IMU)
    dvis = f.upload_visual(vis, counts=True)

    def in_run():
        f.run_log(dlog, 0, E, visual=dvis, sync=False)

    def cut():
        for a, b in zip(cuts[:-1], cuts[1:]):
            f.run_log(dlog, a, b - a, sync=False)
            for r in range(off[b - 1], off[b]):
                f.update_visual(feats[r], FCOV, CORNERS, markers[r], COV_MARKER, CAMERA, CAM_IN_IMU)

    variants = (("in_run", in_run), ("cut", cut))
    ms = {k: [] for k, _ in variants}
    last = {}
    for rnd in range(warmup + rounds):
        for name, fn in variants:
            reset()
            t0 = time.perf_counter()
            fn()
            f.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            if rnd >= warmup:
                ms[name].append(round(t, 3))
            last[name] = f.get_state_mu()
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_rows = int(off[-1])
    return dict(batch=B, rows_per_visual_epoch=rows_per_epoch, visual_epochs=len(vis_epochs), rows=n_rows,
                kernels_at_start=kernels, kernels_at_end=dict(pair=f.pair_active(), param_block=f.param_block()),
                ms=ms, median_ms=med,
                saved_ms_per_visual_epoch=round((med["cut"] - med["in_run"]) / len(vis_epochs), 4),
                in_run_faster_than_cut_every_round=all(x < y for x, y in zip(ms["in_run"], ms["cut"])),
                means_bitwise_equal=bool(np.array_equal(last["in_run"], last["cut"])),
                applied_min=int(dvis.applied(f.stream).min()) // (warmup + rounds),
                scene_status_or=scene_status, status_or=int(np.bitwise_or.reduce(f.get_status())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--epochs", type=int, default=200, help="epochs per call")
    ap.add_argument("--every", type=int, default=10, help="a visual epoch every this many epochs")
    ap.add_argument("--rows", default="1,2", help="rows per visual epoch, one variant each")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1, help="untimed rounds")
    ap.add_argument("--dof", type=int, default=53)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from uwvk import engine, synth

    cases = [measure(engine, synth, int(b), a.epochs, a.every, int(r), a.rounds, a.warmup, a.dof)
             for b in a.batches.split(",") for r in a.rows.split(",")]
    out = dict(tool="visual_run_cost", mode="C3", dof=a.dof, epochs=a.epochs, every=a.every, features=4,
               rounds=a.rounds, clock="host wall clock, first call to the end of synchronize", cases=cases,
               in_run_faster_than_cut_every_round=all(c["in_run_faster_than_cut_every_round"] for c in cases))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
