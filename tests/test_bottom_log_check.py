"""uwvk_bottom_log_check (CPU, host only): every UWVK_EINVAL and UWVK_ENAN case
of include/uwvk.h, each flipped from one valid log, and the same log over a
range that leaves the bad epoch out (UWVK_OK).  The DEVICE pointers of the
struct point at host arrays here: the check never reads through them."""
import ctypes as C

import numpy as np
import pytest

from uwvk import abi, engine
from uwvk.small import bottom_log_struct

OK, EINVAL, ENAN = 0, 1, 2
E, B = 6, 2
BAD = 3  # the epoch the per-epoch cases spoil: beams 0 and 1 and a normal


def valid():
    log = dict(epochs=E, dt=0.2, beams=2, velocity=np.zeros((E, B, 3)),
               flags=np.array([1, 2, 0, 3 | abi.BEV_NORMAL, 1, abi.BEV_NORMAL], np.uint32),
               beam_direction=[[0.5, 0.0, -0.866], [-0.5, 0.0, -0.866]], beam_origin=[[0.1, 0, 0], [-0.1, 0, 0]],
               range_index=np.array([0, 1, 0, 2, 3, 0], np.int32), range=np.full((4, 2, B), 11.0), range_var=None,
               range_cov=0.02, normal_index=np.array([0, 0, 0, 0, 0, 1], np.int32), normal=np.ones((2, B, 3)),
               normal_cov=np.eye(2) * 4e-4)
    return log


def check(log, first=0, count=None, drop=()):
    ptr = {k: log[k].ctypes.data_as(C.c_void_p) for k in ("velocity", "range", "range_var", "normal")
           if log.get(k) is not None and k not in drop}
    s, keep = bottom_log_struct(log, ptr)
    for k in drop:
        if k in ("flags", "range_index", "normal_index"):
            setattr(s, k, None)
    count = E - first if count is None else count
    return engine.lib().uwvk_bottom_log_check(C.byref(s), C.c_int64(first), C.c_int64(count))


def test_valid_log():
    assert check(valid()) == OK
    assert check(valid(), 2, 0) == OK and check(valid(), E, 0) == OK
    v = valid()
    v["range_var"] = np.full((4, 2, B), 0.02)
    assert check(v) == OK


def test_null_log_and_ranges():
    assert engine.lib().uwvk_bottom_log_check(None, C.c_int64(0), C.c_int64(0)) == EINVAL
    for first, count in ((-1, 2), (0, -1), (0, E + 1), (E, 1), (E + 1, 0)):
        assert check(valid(), first, count) == EINVAL, (first, count)


@pytest.mark.parametrize("dt", [0.0, -0.2, np.nan])
def test_dt(dt):
    log = valid()
    log["dt"] = dt
    assert check(log) == EINVAL


def test_beams():
    for beams in (-1, 9):
        log = valid()
        log["beams"] = beams
        assert check(log, 2, 1) == EINVAL  # epoch 2 has no flag at all
    log = valid()
    log["beams"] = 0
    assert check(log, 2, 1) == OK and check(log, 5, 1) == OK


def spoil(log, what):
    """-> the keys of the struct to null"""
    if what == "flag_bit_beyond_beams":
        log["flags"][BAD] |= abi.bev_beam(2)
    elif what == "flag_bit_unknown":
        log["flags"][BAD] |= 0x200
    elif what == "range_index_negative":
        log["range_index"][BAD] = -1
    elif what == "range_index_past":
        log["range_index"][BAD] = 4
    elif what == "normal_index_negative":
        log["normal_index"][BAD] = -1
    elif what == "normal_index_past":
        log["normal_index"][BAD] = 2
    else:
        return (what[len("null_"):],)
    return ()


@pytest.mark.parametrize("what", ["flag_bit_beyond_beams", "flag_bit_unknown", "range_index_negative",
                                  "range_index_past", "normal_index_negative", "normal_index_past",
                                  "null_range_index", "null_range", "null_normal_index", "null_normal"])
def test_einval_at_a_flagged_epoch(what):
    log = valid()
    drop = spoil(log, what)
    assert check(log, drop=drop) == EINVAL
    assert check(log, BAD, 1, drop=drop) == EINVAL
    # ranges without the bad epoch, and for the NULL arrays without that kind
    kind = "normal" if "normal" in what else "range"
    if drop and kind == "range":
        assert check(log, 2, 1, drop=drop) == OK and check(log, 5, 1, drop=drop) == OK  # no beam flagged there
        assert check(log, 0, 1, drop=drop) == EINVAL
    elif drop:
        assert check(log, 0, 3, drop=drop) == OK and check(log, 4, 1, drop=drop) == OK  # no normal flagged there
        assert check(log, 5, 1, drop=drop) == EINVAL
    else:
        assert check(log, 0, BAD, drop=drop) == OK and check(log, BAD + 1, E - BAD - 1, drop=drop) == OK


@pytest.mark.parametrize("what", ["flags", "velocity"])
def test_null_flags_or_velocity(what):
    assert check(valid(), drop=(what,)) == EINVAL
    assert check(valid(), 3, 0, drop=(what,)) == OK  # count == 0 reads neither


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_enan_shared_values(bad):
    log = valid()
    log["range_cov"] = bad
    assert check(log) == ENAN
    assert check(log, 2, 1) == OK and check(log, 5, 1) == OK  # no range there
    log["range_var"] = np.full((4, 2, B), 0.02)                  # range_cov unused with range_var
    assert check(log) == OK
    log = valid()
    log["normal_cov"] = np.array([[4e-4, bad], [0.0, 4e-4]])
    assert check(log) == ENAN
    assert check(log, 0, 3) == OK and check(log, 4, 1) == OK     # no normal there
    for key in ("beam_direction", "beam_origin"):
        log = valid()
        log[key] = np.array(log[key], float)
        log[key][1, 2] = bad                                     # beam 1: epochs 1 and 3
        assert check(log) == ENAN and check(log, 1, 1) == ENAN
        assert check(log, 0, 1) == OK and check(log, 4, 2) == OK   # beam 0 alone, or none


def test_einval_before_enan():
    log = valid()
    log["range_cov"] = np.nan
    log["normal_index"][5] = 7
    assert check(log) == EINVAL
