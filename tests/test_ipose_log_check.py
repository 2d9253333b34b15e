"""uwvk_ipose_log_check (CPU, host only): every UWVK_EINVAL and UWVK_ENAN case
of include/uwvk.h (tests/ipose_run_scenes.py FAULTS), each flipped from one
valid recorded log, and faults that lie outside the range or in inputs no row
of the range uses (UWVK_OK).  The DEVICE pointers of the struct point at host
arrays here: the check never reads through them."""
import ctypes as C

import numpy as np
import pytest

import ipose_run_scenes as R
from uwvk import engine
from uwvk.small import IPOSE_DEVICE_ARRAYS, ipose_log_struct

OK = 0
LOG = R.fault_log()


def struct(log):
    log = R.copy_log(log)
    ptr = {k: log[k].ctypes.data_as(C.c_void_p) for k in IPOSE_DEVICE_ARRAYS if log.get(k) is not None}
    s, host = ipose_log_struct(log, ptr)
    return s, host, log


def check(s, first, count):
    return engine.lib().uwvk_ipose_log_check(C.byref(s), C.c_int64(first), C.c_int64(count))


def test_valid_logs():
    s, host, _ = struct(LOG)
    assert check(s, 0, 6) == OK and check(s, 2, 0) == OK and check(s, 6, 0) == OK and check(s, 3, 2) == OK
    s, host, _ = struct(R.per_instance(LOG))
    assert not s.shared_feature_cov and not s.shared_marker_pose and check(s, 0, 6) == OK
    # one dt, no visual rows, no reference: the smallest log
    s, host, _ = struct(dict(batch=2, epochs=3, dt=0.1, n_features=0, cov_marker_pose=np.zeros(36),
                             camera=np.zeros(4), camera_in_body=np.zeros(7)))
    assert not s.visual_offset and s.n_visual == 0 and check(s, 0, 3) == OK


def test_null_log():
    assert engine.lib().uwvk_ipose_log_check(None, C.c_int64(0), C.c_int64(0)) == R.EINVAL


@pytest.mark.parametrize("name, mutate, first, count, code", R.FAULTS, ids=[f[0] for f in R.FAULTS])
def test_fault(name, mutate, first, count, code):
    s, host, _ = struct(LOG)
    if mutate:
        mutate(s, host)
    assert check(s, first, count) == code


@pytest.mark.parametrize("name, mutate, first, count", R.OUTSIDE, ids=[f[0] for f in R.OUTSIDE])
def test_fault_outside_the_range_is_not_reported(name, mutate, first, count):
    s, host, _ = struct(LOG)
    mutate(s, host)
    assert check(s, first, count) == OK
    assert check(s, 0, 6) != OK or name.startswith("unused")
