"""uwvk_pose_visual_check (CPU, host only): every UWVK_EINVAL and UWVK_ENAN case
of include/uwvk.h (tests/pose_visual_run_scenes.py FAULTS), each flipped from
one valid visual struct, and faults that lie outside the range or in inputs no
row of the range uses (UWVK_OK).  The DEVICE pointers of the struct point at
host arrays here: the check never reads through them."""
import ctypes as C

import numpy as np
import pytest

import pose_visual_run_scenes as R
from uwvk import engine
from uwvk.engine import POSE_VISUAL_DEVICE_ARRAYS, pose_visual_struct

OK = 0
E = R.CHECK_EPOCHS


def struct(vis):
    vis = R.copy_visual(vis)
    ptr = {k: vis[k].ctypes.data_as(C.c_void_p) for k in POSE_VISUAL_DEVICE_ARRAYS if vis.get(k) is not None}
    s, host = pose_visual_struct(vis, ptr)
    return s, host, vis


def check(s, first, count, epochs=E):
    return engine.lib().uwvk_pose_visual_check(C.byref(s), C.c_int64(epochs), C.c_int64(first), C.c_int64(count))


def test_valid_structs():
    s, host, _ = struct(R.check_visual())
    assert s.n_visual == 6 and not s.feature_cov and not s.marker_pose
    assert check(s, 0, 6) == OK and check(s, 2, 0) == OK and check(s, 6, 0) == OK and check(s, 3, 2) == OK
    s, host, _ = struct(R.check_visual(per_inst=True))
    assert not s.shared_feature_cov and not s.shared_marker_pose and check(s, 0, 6) == OK
    # no rows at all: no offsets needed, nothing else read
    s, host, _ = struct(dict(n_features=0, cov_marker_pose=np.full(36, np.nan), camera=np.zeros(4),
                             camera_in_imu=np.zeros(7)))
    assert not s.visual_offset and s.n_visual == 0 and check(s, 0, 6) == OK
    # the Python front end on the same dict
    assert engine.pose_visual_check(R.check_visual(), E) == OK
    assert engine.pose_visual_check(R.check_visual(), E, 3, 2) == OK
    assert engine.pose_visual_check(R.check_visual(), E, 4, 3) == R.EINVAL


def test_null_struct_and_negative_epochs():
    assert engine.lib().uwvk_pose_visual_check(None, C.c_int64(E), C.c_int64(0), C.c_int64(0)) == R.EINVAL
    s, host, _ = struct(R.check_visual())
    assert check(s, 0, 0, epochs=-1) == R.EINVAL


@pytest.mark.parametrize("name, mutate, first, count, code", R.FAULTS, ids=[f[0] for f in R.FAULTS])
def test_fault(name, mutate, first, count, code):
    s, host, _ = struct(R.check_visual())
    assert check(s, 0, 6) == OK
    if mutate:
        mutate(s, host)
    assert check(s, first, count) == code


@pytest.mark.parametrize("name, mutate, first, count", R.OUTSIDE, ids=[f[0] for f in R.OUTSIDE])
def test_fault_outside_the_range_is_not_reported(name, mutate, first, count):
    s, host, _ = struct(R.check_visual())
    mutate(s, host)
    assert check(s, first, count) == OK
    assert check(s, 0, 6) != OK


def test_einval_comes_before_enan():
    """A struct with both defects in the range reports the argument error."""
    s, host, _ = struct(R.check_visual())
    host["feature_positions"].reshape(-1)[0] = np.nan
    s.features = None
    assert check(s, 0, 6) == R.EINVAL
