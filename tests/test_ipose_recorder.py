"""IPoseLogRecorder and play_ipose_log (CPU, pure Python) on the oracle: the
direct calls against recorder -> log -> play_ipose_log, bitwise; the layout of
the recorded log; what the recorder refuses; how play masks non-finite entries."""
import numpy as np
import pytest

import ipose_run_scenes as R
import oracle_ctypes as O
import small_scenes as S
import visual_scene as V
from uwvk.small import IPoseLogRecorder, play_ipose_log


def oracle(B):
    return R.init(O.OracleIndirectPoseBatch(B), B)


@pytest.mark.parametrize("kw", [dict(), dict(shared_marker=True), dict(fcov="per instance"), dict(dts=(0.1,))],
                         ids=["per-instance marker", "shared inputs", "per-instance covariance", "one dt"])
def test_recorded_log_replays_bitwise(kw):
    B = 3
    if kw.get("fcov"):
        kw = dict(fcov=S.per_instance_fcov(B, 4))
    direct, rec = oracle(B), IPoseLogRecorder(B)
    R.drive((direct, rec), B, **kw)
    log = rec.log()
    played = oracle(B)
    issued = play_ipose_log(played, log)
    for a, b in zip(direct.get_state(), played.get_state()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(direct.get_corrected_pose(), played.get_corrected_pose())
    np.testing.assert_array_equal(issued, np.full(B, sum(R.ROWS6)))
    # adjacent ranges of the log are the whole log
    split = oracle(B)
    play_ipose_log(split, log, 0, 2)
    play_ipose_log(split, log, 2, 4)
    for a, b in zip(direct.get_state(), split.get_state()):
        np.testing.assert_array_equal(a, b)


def test_layout_of_the_recorded_log():
    B = 3
    log = R.record(B)
    assert log["batch"] == B and log["epochs"] == 6 and log["n_features"] == 4
    assert list(log["visual_offset"]) == [0, 0, 1, 3, 4, 4, 6] and log["visual_offset"].dtype == np.int64
    np.testing.assert_array_equal(log["dt_epoch"], R.DTS6)
    assert log["pose_ref"].shape == (6, B, 7) and log["features"].shape == (6, B, 4, 2)
    assert log["feature_cov"] is None and log["shared_feature_cov"].shape == (4, 4)
    assert log["marker_pose"].shape == (6, B, 7) and log["shared_marker_pose"] is None
    log = R.record(B, shared_marker=True, dts=(0.1,))
    assert log["dt"] == 0.1 and log["dt_epoch"] is None
    assert log["marker_pose"] is None and log["shared_marker_pose"].shape == (6, 7)
    rec = IPoseLogRecorder(B)  # no reference, no rows
    rec.predict(0.1)
    rec.predict(0.1)
    log = rec.log()
    assert log["pose_ref"] is None and log["epochs"] == 2 and list(log["visual_offset"]) == [0, 0, 0]
    assert log["features"].shape[0] == 0


def test_refusals():
    B = 2
    ref, _, _, marker, px = V.ipose_scene(B)
    fcov, fpos, cm, cam, cib = V.visual_common(B)
    args = (px, fcov, fpos, marker, cm, cam, cib)

    def rec(epochs=1):
        r = IPoseLogRecorder(B)
        r.set_pose_reference(ref)
        for _ in range(epochs):
            r.predict(0.1)
        return r

    with pytest.raises(ValueError, match="mask"):
        rec().update_visual(*args, mask=np.ones(B, bool))
    with pytest.raises(ValueError, match="before the first predict"):
        rec(0).update_visual(*args)
    r = rec()
    r.update_visual(*args)
    with pytest.raises(ValueError, match="feature count"):
        r.update_visual(np.tile(V.ipose_scene(B, corners=V.CORNERS7)[4], 1), V.visual_common(B, V.CORNERS7)[0],
                        V.CORNERS7, marker, cm, cam, cib)
    for k, other in ((2, fpos * 1.5), (4, cm * 2), (5, cam + 1.0), (6, cib[::-1].copy())):
        a = list(args)
        a[k] = other
        with pytest.raises(ValueError, match="change"):
            r.update_visual(*a)
    r.set_pose_reference(ref)
    with pytest.raises(ValueError, match="between"):
        r.update_visual(*args)
    with pytest.raises(ValueError, match="after the last predict"):
        r.log()
    late = IPoseLogRecorder(B)
    late.predict(0.1)
    with pytest.raises(ValueError, match="first set after"):
        late.set_pose_reference(ref)


class Calls:
    """records what play_ipose_log issues"""

    def __init__(self):
        self.refs, self.masks, self.args = [], [], []

    def set_pose_reference(self, pose):
        self.refs.append(np.array(pose))

    def predict(self, dt):
        pass

    def update_visual(self, *a, mask=None):
        self.args.append([np.array(v) for v in a])
        self.masks.append(None if mask is None else np.array(mask))


def test_play_masks_non_finite_entries():
    B = 3
    log = R.per_instance(R.record(B, rows=(1, 1, 1), shared_marker=True))
    log["features"][0, 1, 2, 0] = np.nan
    log["feature_cov"][1, 0, 3, 1] = np.inf
    log["marker_pose"][2, 2, 4] = np.nan
    log["pose_ref"][1, 0, 6] = np.nan
    c = Calls()
    issued = play_ipose_log(c, log)
    np.testing.assert_array_equal(issued, [2, 2, 2])
    np.testing.assert_array_equal(c.masks, [[1, 0, 1], [0, 1, 1], [1, 1, 0]])
    assert all(np.isfinite(v).all() for a in c.args for v in a)
    np.testing.assert_array_equal(c.refs[1][0], log["pose_ref"][0, 0])  # the last finite reference
    np.testing.assert_array_equal(c.refs[1][1:], log["pose_ref"][1, 1:])
    np.testing.assert_array_equal(c.refs[2], log["pose_ref"][2])
    log["pose_ref"][0, 1, 0] = np.nan
    with pytest.raises(ValueError, match="before any finite one"):
        play_ipose_log(Calls(), log)
