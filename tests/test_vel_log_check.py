"""uwvk_vel_log_check (CPU, host only): every UWVK_EINVAL and UWVK_ENAN case of
include/uwvk.h, each flipped from one valid log, and the same log over a range
that leaves the bad epoch out (UWVK_OK).  The DEVICE pointers of the struct
point at host arrays here: the check never reads through them."""
import ctypes as C

import numpy as np
import pytest

from uwvk import abi, engine

OK, EINVAL, ENAN = 0, 1, 2
E, B = 6, 2
BAD = 3  # the epoch the per-epoch cases spoil: a DVL and a pressure sample
DEVICE = ("flags", "gyro", "efforts", "dvl_index", "dvl", "pressure_index", "pressure")


def valid():
    D, P = abi.EV_DVL, abi.EV_PRESSURE
    return dict(batch=B, epochs=E, dt=0.02, flags=np.array([P, D, 0, D | P, D, P], np.uint32),
                gyro=np.zeros((E, B, 3)), efforts=np.zeros((E, B, 6)),
                dvl_index=np.array([-1, 0, -1, 2, 1, -1], np.int32), dvl=np.ones((3, B, 3)), dvl_cov=np.eye(3) * 1e-3,
                pressure_index=np.array([0, -1, -1, 1, -1, 2], np.int32), pressure=np.full((3, B), -10.0),
                pressure_cov=1e-3)


def check(log, first=0, count=None, drop=(), host_drop=(), no_host=False):
    """drop: DEVICE pointers of uwvk_vel_log to null; host_drop: fields of uwvk_vel_log_host"""
    arrays = {k: np.ascontiguousarray(log[k]) for k in DEVICE}
    ptr = {k: a.ctypes.data_as(C.c_void_p) for k, a in arrays.items() if k not in drop}
    s, hs, keep = engine.vel_log_struct(log, ptr)
    for k in host_drop:
        setattr(hs, k, None)
    count = E - first if count is None else count
    return engine.lib().uwvk_vel_log_check(C.byref(s), None if no_host else C.byref(hs), C.c_int64(first),
                                           C.c_int64(count))


def test_valid_log():
    assert check(valid()) == OK
    assert check(valid(), 2, 0) == OK and check(valid(), E, 0) == OK
    assert engine.vel_log_check(valid()) == OK and engine.vel_log_check(valid(), 1, 3) == OK
    # a kind that is never flagged needs none of its arrays
    log = valid()
    log["flags"] &= ~np.uint32(abi.EV_DVL)
    assert check(log, drop=("dvl_index", "dvl"), host_drop=("dvl_index",)) == OK


def test_null_log_host_and_ranges():
    L = engine.lib()
    s, hs, keep = engine.vel_log_struct(valid(), {})
    assert L.uwvk_vel_log_check(None, C.byref(hs), C.c_int64(0), C.c_int64(0)) == EINVAL
    assert check(valid(), 0, 0, no_host=True) == EINVAL
    for first, count in ((-1, 2), (0, -1), (0, E + 1), (E, 1), (E + 1, 0)):
        assert check(valid(), first, count) == EINVAL, (first, count)


@pytest.mark.parametrize("dt", [0.0, -0.02, np.nan, np.inf])
def test_dt(dt):
    log = valid()
    log["dt"] = dt
    assert check(log) == EINVAL and check(log, 2, 0) == EINVAL


@pytest.mark.parametrize("what", ["host_flags", "flags", "gyro", "efforts"])
def test_null_flags_or_inputs(what):
    kw = dict(host_drop=("flags",)) if what == "host_flags" else dict(drop=(what,))
    assert check(valid(), **kw) == EINVAL
    assert check(valid(), 2, 1, **kw) == EINVAL  # an epoch without events still needs them
    assert check(valid(), 3, 0, **kw) == OK      # count == 0 reads none of them


def spoil(log, what):
    """-> (DEVICE pointers to null, host fields to null)"""
    if what == "flag_bit_unknown":
        log["flags"][BAD] |= abi.EV_ACC
    elif what == "flag_bit_high":
        log["flags"][BAD] |= 0x100
    elif what == "dvl_index_negative":
        log["dvl_index"][BAD] = -1
    elif what == "dvl_index_past":
        log["dvl_index"][BAD] = 3
    elif what == "pressure_index_negative":
        log["pressure_index"][BAD] = -1
    elif what == "pressure_index_past":
        log["pressure_index"][BAD] = 3
    elif what.startswith("null_host_"):
        return (), (what[len("null_host_"):],)
    else:
        return (what[len("null_"):],), ()
    return (), ()


@pytest.mark.parametrize("what", ["flag_bit_unknown", "flag_bit_high", "dvl_index_negative", "dvl_index_past",
                                  "pressure_index_negative", "pressure_index_past",
                                  "null_host_dvl_index", "null_dvl_index", "null_dvl",
                                  "null_host_pressure_index", "null_pressure_index", "null_pressure"])
def test_einval_at_a_flagged_epoch(what):
    log = valid()
    drop, host_drop = spoil(log, what)
    kw = dict(drop=drop, host_drop=host_drop)
    assert check(log, **kw) == EINVAL
    assert check(log, BAD, 1, **kw) == EINVAL
    if drop or host_drop:  # a NULL array: ranges without that kind pass, any with it fails
        if "dvl" in what:
            assert check(log, 0, 1, **kw) == OK and check(log, 5, 1, **kw) == OK and check(log, 2, 1, **kw) == OK
            assert check(log, 1, 1, **kw) == EINVAL and check(log, 4, 1, **kw) == EINVAL
        else:
            assert check(log, 1, 2, **kw) == OK and check(log, 4, 1, **kw) == OK
            assert check(log, 0, 1, **kw) == EINVAL and check(log, 5, 1, **kw) == EINVAL
    else:          # a bad entry at epoch BAD: the ranges on either side of it pass
        assert check(log, 0, BAD, **kw) == OK and check(log, BAD + 1, E - BAD - 1, **kw) == OK


def test_unflagged_epochs_index_is_not_read():
    """the -1 of the epochs without a sample (synth.make_vel_log's layout), or any other value there"""
    log = valid()
    log["dvl_index"][2] = 1000
    log["pressure_index"][1] = -7
    assert check(log) == OK


def test_row_counts_come_from_the_host_struct():
    log = valid()
    arrays = {k: np.ascontiguousarray(log[k]) for k in DEVICE}
    s, hs, keep = engine.vel_log_struct(log, {k: a.ctypes.data_as(C.c_void_p) for k, a in arrays.items()})
    assert (hs.n_dvl, hs.n_pressure) == (3, 3)
    L = engine.lib()
    hs.n_dvl = 2  # row 2 is used at epoch 3
    assert L.uwvk_vel_log_check(C.byref(s), C.byref(hs), C.c_int64(0), C.c_int64(E)) == EINVAL
    assert L.uwvk_vel_log_check(C.byref(s), C.byref(hs), C.c_int64(4), C.c_int64(2)) == OK
    hs.n_dvl, hs.n_pressure = 3, 0
    assert L.uwvk_vel_log_check(C.byref(s), C.byref(hs), C.c_int64(0), C.c_int64(1)) == EINVAL
    assert L.uwvk_vel_log_check(C.byref(s), C.byref(hs), C.c_int64(1), C.c_int64(2)) == OK


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_enan_shared_covariances(bad):
    log = valid()
    log["dvl_cov"] = np.eye(3) * 1e-3
    log["dvl_cov"][1, 2] = bad
    assert check(log) == ENAN and check(log, 1, 1) == ENAN
    assert check(log, 0, 1) == OK and check(log, 5, 1) == OK and check(log, 2, 1) == OK  # no DVL there
    log = valid()
    log["pressure_cov"] = bad
    assert check(log) == ENAN and check(log, 0, 1) == ENAN
    assert check(log, 1, 2) == OK and check(log, 4, 1) == OK                            # no pressure there


def test_einval_before_enan():
    log = valid()
    log["pressure_cov"] = np.nan
    log["dvl_index"][4] = 9
    assert check(log) == EINVAL
