"""BottomLogRecorder and play_bottom_log (CPU, no device): small_scenes.
bottom_sequence driven into a recorder and, in parallel, directly into an
OracleBottomBatch; the recorded log played onto a second OracleBottomBatch is
bitwise the direct one, and onto the numpy twin within the twin's 1e-10 sigma
(tests/test_small_twin.py).  Then what the log cannot express."""
import numpy as np
import pytest

import oracle_ctypes as O
import small_scenes as S
import visual_scene as V
from test_small_twin import BottomTwinBatch
from uwvk import abi
from uwvk.small import BottomLogRecorder, play_bottom_log

B, STEPS, DT = 5, 30, 0.2
TWIN_TOL = 1e-10


@pytest.fixture(scope="module")
def recorded():
    x, P = V.bottom_state(B)
    direct = O.OracleBottomBatch(B)
    direct.init(x, P)
    direct.set_process_noise(S.BOTTOM_Q)
    rec = BottomLogRecorder(B, DT)
    S.bottom_sequence((rec, direct), B, steps=STEPS)
    return x, P, rec.log(), direct.get_state()


def test_recorded_layout(recorded):
    _, _, log, _ = recorded
    assert log["epochs"] == STEPS and log["dt"] == DT and log["beams"] == 4
    np.testing.assert_array_equal(log["beam_direction"], [b[0] for b in S.BEAMS])
    np.testing.assert_array_equal(log["beam_origin"], [b[1] for b in S.BEAMS])
    want = [abi.bev_beam(e % 4) | (abi.BEV_NORMAL if e % 5 == 4 else 0) for e in range(STEPS)]
    np.testing.assert_array_equal(log["flags"], want)
    assert log["velocity"].shape == (STEPS, B, 3) and log["range"].shape == (STEPS, 4, B)
    assert log["range_var"].shape == (STEPS, 4, B)  # bottom_sequence's variances are per instance
    assert log["normal"].shape == (STEPS // 5, B, 3)
    np.testing.assert_array_equal(log["range_index"], np.arange(STEPS))
    np.testing.assert_array_equal(log["normal_index"][4::5], np.arange(STEPS // 5))
    np.testing.assert_array_equal(log["normal_cov"], np.eye(2) * 4e-4)


def test_play_is_bitwise_the_direct_calls(recorded):
    x, P, log, (xd, Pd) = recorded
    o = O.OracleBottomBatch(B)
    o.init(x, P)
    o.set_process_noise(S.BOTTOM_Q)
    issued = play_bottom_log(o, log, 0, 12)
    issued += play_bottom_log(o, log, 12, STEPS - 12)
    xo, Po = o.get_state()
    np.testing.assert_array_equal(xo, xd)
    np.testing.assert_array_equal(Po, Pd)
    np.testing.assert_array_equal(issued, np.tile([STEPS, STEPS // 5], (B, 1)))


def test_play_on_the_twin(recorded):
    x, P, log, (xd, Pd) = recorded
    t = BottomTwinBatch(B)
    t.init(x, P)
    t.set_process_noise(S.BOTTOM_Q)
    play_bottom_log(t, log)
    es, ec = S.bottom_err(*t.get_state(), xd, Pd)
    print("twin against the direct oracle: state %.3g sigma, covariance %.3g" % (es, ec))
    assert es < TWIN_TOL and ec < TWIN_TOL, (es, ec)


def test_play_masks_what_the_run_skips(recorded):
    """a NaN range, an Inf variance and a zero normal each leave exactly their
    instance out of exactly that update; a NaN velocity has no single-call form"""
    x, P, log, _ = recorded
    bad = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in log.items()}
    bad["range"][2, 2, 1] = np.nan        # epoch 2 is beam 2
    bad["range_var"][3, 3, 4] = np.inf
    bad["normal"][0, 0] = 0.0             # epoch 4
    calls = []

    class Spy(O.OracleBottomBatch):
        def update_range(self, mu, cov, direction, origin, mask=None):
            calls.append(("r", None if mask is None else np.array(mask)))
            assert np.isfinite(mu).all() and np.isfinite(cov).all()
            super().update_range(mu, cov, direction, origin, mask=mask)

        def update_normal(self, mu, cov, mask=None):
            calls.append(("n", None if mask is None else np.array(mask)))
            super().update_normal(mu, cov, mask=mask)

    o = Spy(B)
    o.init(x, P)
    o.set_process_noise(S.BOTTOM_Q)
    issued = play_bottom_log(o, bad, 0, 5)
    masks = [m for _, m in calls]
    assert [k for k, _ in calls] == ["r", "r", "r", "r", "r", "n"]
    assert masks[0] is None and masks[1] is None and masks[4] is None
    np.testing.assert_array_equal(masks[2], np.arange(B) != 1)
    np.testing.assert_array_equal(masks[3], np.arange(B) != 4)
    np.testing.assert_array_equal(masks[5], np.arange(B) != 0)
    want = np.tile([5, 1], (B, 1))
    want[1, 0] -= 1
    want[4, 0] -= 1
    want[0, 1] -= 1
    np.testing.assert_array_equal(issued, want)
    bad["velocity"][1, 2, 0] = np.nan
    with pytest.raises(ValueError):
        play_bottom_log(o, bad, 1, 1)


def test_shared_range_covariance():
    rec = BottomLogRecorder(2, DT)
    for e in range(3):
        rec.predict(DT)
        rec.update_range([11.0, 11.1], 0.02, *S.BEAMS[e % 2])
    log = rec.log()
    assert log["range_var"] is None and log["range_cov"] == 0.02 and log["beams"] == 2
    np.testing.assert_array_equal(log["velocity"], 0.0)  # never set: the handle's zero velocity
    rec.predict(DT)
    rec.update_range([11.0, 11.1], 0.03, *S.BEAMS[0])     # a second scalar: per-instance rows instead
    log = rec.log()
    assert [log["range_var"][e, b, 1] for e, b in enumerate((0, 1, 0, 0))] == [0.02, 0.02, 0.02, 0.03]


def fresh():
    rec = BottomLogRecorder(2, DT)
    rec.set_velocity([0.5, 0.0, 0.0])
    rec.predict(DT)
    return rec


def test_what_the_log_cannot_express():
    z, n = [11.0, 11.1], [[0.0, 0.0, 1.0]] * 2
    rec = fresh()
    with pytest.raises(ValueError):
        rec.predict(0.1)                                   # a dt that changes
    rec = fresh()
    with pytest.raises(ValueError):
        rec.update_normal(n, np.tile(np.eye(2) * 4e-4, (2, 1, 1)))  # per-instance normal covariance
    rec = fresh()
    rec.update_normal(n, np.eye(2) * 4e-4)
    rec.predict(DT)
    with pytest.raises(ValueError):
        rec.update_normal(n, np.eye(2) * 5e-4)             # ... or one that changes
    rec = fresh()
    for k in range(8):
        rec.update_range(z, 0.02, [0.0, 0.0, -1.0], [0.1 * k, 0.0, 0.0])
    with pytest.raises(ValueError):
        rec.update_range(z, 0.02, [0.0, 0.0, -1.0], [0.9, 0.0, 0.0])  # a ninth beam
    assert rec.log()["beams"] == 8
    rec = fresh()
    rec.update_range(z, 0.02, *S.BEAMS[0])
    with pytest.raises(ValueError):
        rec.update_range(z, 0.02, *S.BEAMS[0])             # a beam twice in one epoch
    rec.update_range(z, 0.02, *S.BEAMS[1])
    rec.predict(DT)
    rec.update_range(z, 0.02, *S.BEAMS[1])
    with pytest.raises(ValueError):
        rec.update_range(z, 0.02, *S.BEAMS[0])             # out of beam order
    rec = fresh()
    rec.update_normal(n, np.eye(2) * 4e-4)
    with pytest.raises(ValueError):
        rec.update_range(z, 0.02, *S.BEAMS[0])             # a range after the normal
    with pytest.raises(ValueError):
        rec.update_normal(n, np.eye(2) * 4e-4)             # two normals in one epoch
    with pytest.raises(ValueError):
        BottomLogRecorder(2, DT).update_range(z, 0.02, *S.BEAMS[0])  # before the first predict
    with pytest.raises(ValueError):
        fresh().update_range(z, 0.02, *S.BEAMS[0], mask=[1, 0])      # a mask
