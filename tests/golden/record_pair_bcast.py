#!/usr/bin/env python3
"""Records tests/golden/pair_bcast_{dvl,adcp,nan}.npz: the pair kernel's mean,
covariance and status for the scenes of tests/test_gpu_pair_bcast.py, from the
library of the commit BEFORE the fused broadcasts,

    1b046c3  run_log: merge the row-layout, launcher and visual-row duplicates

built from that commit's sources and selected with UWVK_LIB; run once on an
MI355X.  The test compares the current library bitwise with these arrays, and
checks by a digest that its inputs are the recorded ones.

usage: UWVK_LIB=/path/to/that/commit's/libuwvk.so python tests/golden/record_pair_bcast.py [outdir]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "slam-uwv_kalman_filters_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
PARENT = "1b046c3"


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    if not os.environ.get("UWVK_LIB"):
        raise SystemExit("UWVK_LIB must name the library built from commit %s" % PARENT)
    from uwvk import engine
    import test_gpu_pair_bcast as T
    if not engine.device_available(0):
        raise SystemExit("no gfx950 device")

    def put(d, key, got, digest):
        d[key + "_x"], d[key + "_P"], d[key + "_status"] = got[0], got[1], got[3]
        d[key + "_inputs"] = np.array(digest)

    for kind in ("dvl", "adcp"):
        d = {"parent_commit": np.array(PARENT)}
        for k, dof, side in T.SCENES:
            if k != kind:
                continue
            st = T.start(engine, kind, 2, dof)
            put(d, T.scene_key(kind, dof, side), T.run(engine, st, True, dof, side), T.inputs_digest(st))
        np.savez_compressed(os.path.join(out, "pair_bcast_%s.npz" % kind), **d)
    st = T.start(engine, "dvl", 6, 53)
    bad = T.nan_logs(st[0])[0]
    d = {"parent_commit": np.array(PARENT)}
    put(d, "clean", T.run(engine, st, True, 53, "right"), T.inputs_digest(st))
    put(d, "nan", T.run(engine, st, True, 53, "right", log=bad), T.inputs_digest(st, bad))
    np.savez_compressed(os.path.join(out, "pair_bcast_nan.npz"), **d)
    for n in ("dvl", "adcp", "nan"):
        p = os.path.join(out, "pair_bcast_%s.npz" % n)
        print("%s: %d bytes, %d arrays" % (p, os.path.getsize(p), len(np.load(p).files)))


if __name__ == "__main__":
    main()
