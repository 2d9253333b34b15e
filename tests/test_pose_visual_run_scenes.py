"""The scenes of tests/test_gpu_pose_visual_run.py, checked on the CPU first
(tests/pose_visual_run_scenes.py): on every healthy scene the oracle integrates
each visual row without an error (its update raises otherwise; V.pose_scene
asserts zc > 1 at every row), everything stays finite, and every row moves the
oracle's estimate of every instance by at least 1e-3 of its standard deviation,
the project's bar for a scene that tests something."""
import numpy as np
import pytest

import pose_visual_run_scenes as R

# the scenes the GPU tests use: (batch, dof, right, nf, shared marker)
SCENES = [
    pytest.param(4, 53, True, 4, False, id="b4_dof53"),
    pytest.param(3, 53, True, 4, False, id="b3_dof53"),
    pytest.param(4, 26, True, 4, False, id="b4_dof26"),
    pytest.param(4, 53, False, 4, False, id="b4_dof53_left"),
    pytest.param(4, 26, False, 4, False, id="b4_dof26_left"),
    pytest.param(4, 53, True, 4, True, id="b4_shared_marker"),
]


@pytest.mark.parametrize("B,dof,right,nf,shared", SCENES)
def test_scene_is_healthy_and_every_row_counts(B, dof, right, nf, shared):
    sc = R.scene(B, dof, right, nf=nf, shared_marker=shared)
    vis = sc["visual"]
    off = vis["visual_offset"]
    assert list(np.flatnonzero(np.diff(off))) == [5, 11, 12, 23] and off[-1] == 5 and off[12] - off[11] == 2
    assert vis["features"].shape == (5, B, nf, 2) and np.isfinite(vis["features"]).all()
    assert np.isfinite(sc["x"]).all() and np.isfinite(sc["P"]).all()
    assert (np.linalg.eigvalsh(sc["P"]) > 0).all()
    print("rows move the oracle by (sigma, min over the batch):", sc["moves"].min(1))
    assert sc["moves"].shape == (5, B) and (sc["moves"] >= R.MOVE_SIGMA).all(), sc["moves"]
    for r in range(5):
        assert R.finite_mask(vis, r, B).all()
    # the same run through row_args, the arguments the single calls get
    x, P = R.oracle_cut_run(sc, B, dof, right)
    np.testing.assert_array_equal(x, sc["x"])
    np.testing.assert_array_equal(P, sc["P"])


def test_one_feature_scene():
    sc = R.scene(4, 53, True, rows_at=((5, 1),), nf=1)
    assert sc["visual"]["features"].shape == (1, 4, 1, 2) and np.isfinite(sc["x"]).all()
    print("the one-feature row moves the oracle by", sc["moves"])
    assert (sc["moves"] >= R.MOVE_SIGMA).all(), sc["moves"]


def test_per_instance_form_holds_the_same_values():
    sc = R.scene(4, 53, True, shared_marker=True)
    vis, pi = sc["visual"], R.per_instance(sc["visual"], 4)
    assert pi["shared_feature_cov"] is None and pi["shared_marker_pose"] is None
    for r in range(5):
        np.testing.assert_array_equal(pi["feature_cov"][r], np.broadcast_to(vis["shared_feature_cov"], (4, 4, 4)))
        np.testing.assert_array_equal(pi["marker_pose"][r], np.broadcast_to(vis["shared_marker_pose"][r], (4, 7)))
    assert vis["marker_pose"] is None and vis["feature_cov"] is None  # the shared scene is left as it was


def test_many_rows_scene_is_healthy():
    """66 rows on one epoch (two launches of the run kernel): the oracle takes them all."""
    sc = R.many_rows_scene()
    off = sc["visual"]["visual_offset"]
    assert off[6] - off[5] == R.MANY_ROWS > 64 and off[-1] == R.MANY_ROWS
    assert sc["visual"]["features"].shape == (R.MANY_ROWS, 2, 1, 2)
    assert np.isfinite(sc["x"]).all() and np.isfinite(sc["P"]).all() and (np.linalg.eigvalsh(sc["P"]) > 0).all()
