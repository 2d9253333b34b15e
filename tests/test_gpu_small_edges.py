"""Edge cases of the lane-group kernels (csrc/uwvk_small.hip, uwvk_pose_visual.hip,
uwvk_aug_dev.hpp) through the C ABI, fp64, batches of at most 40:

 a. an instance's result does not depend on its slot in the wave, on its
    neighbours or on the batch size (bitwise against a batch of one);
 b. masks of update_normal and of both visual updates;
 c. shared against per-instance arguments;
 d. the not-positive-definite path: UWVK_ST_NOTPD at exactly the failed
    instance, its state untouched, its neighbours in the block unaffected;
 e. large errors, the rotated process noise, feature counts 0 / 1 / 7 against
    the oracle.

Every scene compared with the oracle here is one on which the oracle and the
numpy twin agree to 1e-11 on the CPU (tests/test_small_twin.py, named next to
each use).  IPB below is Engine::IPB, the instances per 64-lane block: 8
(BottomUKF), 4 (IndirectPoseUKF predict), 2 (its visual update), 1 (PoseUKF's).

Not reachable through the ABI, so not tested: more than one iteration of
Engine::mean in predict.  Sigma points are symmetric about the mean and both
process models keep them so, so the first Gauss-Newton step is already below
the threshold; there is no back door for it."""
import numpy as np
import pytest

import oracle_ctypes as O
import small_scenes as S
import visual_scene as V
from helpers import cov_err, pivots, pose_setup, state_err
from uwvk import abi, engine, synth
from uwvk.small import BottomUKFBatch, IndirectPoseUKFBatch

pytestmark = pytest.mark.gpu
TOL = 1e-9
NOTPD = 0x1


def same(a, b, rows=slice(None)):
    """(x, P) pairs bitwise equal on `rows`"""
    np.testing.assert_array_equal(a[0][rows], b[0][rows])
    np.testing.assert_array_equal(a[1][rows], b[1][rows])


def masks(B, off):
    """a mask that splits a wave (alternating bits), then one whole lane group off"""
    return [np.arange(B) % 2 == 0, np.arange(B) != off]


def mask_contract(make, call, B, off):
    """make() -> a fresh handle holding the state; call(f, mask, poison) applies
    the update with `mask`, the measurement of row `poison` made NaN."""
    full = make()
    call(full, None, None)
    ref = full.get_state()
    for mask in masks(B, off):
        f = make()
        before = f.get_state()
        call(f, mask, None)
        after = f.get_state()
        same(after, before, ~mask)  # masked-out instances untouched
        same(after, ref, mask)      # masked-in: as the call without a mask
        assert (after[1][mask] != before[1][mask]).any(axis=(1, 2)).all()
        assert not f.get_status().any()
        f = make()
        call(f, mask, np.flatnonzero(~mask)[0])  # NaN in a masked-out row: accepted
        same(f.get_state(), after)
        f = make()
        with pytest.raises(engine.UWVKError) as e:
            call(f, mask, np.flatnonzero(mask)[-1])  # NaN in a masked-in row
        assert e.value.code == 2  # UWVK_ENAN
        same(f.get_state(), before)


def notpd_contract(bad, healthy, oracle, op, j, err):
    """`bad` differs from `healthy` in instance j alone, whose Sigma (or input)
    makes the Cholesky fail; op(f) applies one call; err(state, oracle_state)."""
    B = bad.batch
    others = np.arange(B) != j
    before = bad.get_state()
    same(before, healthy.get_state(), others)
    assert not bad.get_status().any()
    for f in (bad, healthy, oracle):
        op(f)
    st = bad.get_status()
    assert st[j] & NOTPD and not st[others].any(), st  # exactly that instance
    assert not healthy.get_status().any()
    after = bad.get_state()
    same(after, before, j)                      # the failed instance is untouched
    same(after, healthy.get_state(), others)    # its neighbours are unaffected
    assert (after[1][others] != before[1][others]).any()
    es, ec = err(*healthy.get_state(), *oracle.get_state())
    assert es < TOL and ec < TOL, (es, ec)
    assert bad.get_status(clear=True)[j] & NOTPD
    assert not bad.get_status().any()


# ===========================================================================
# BottomUKF
# ===========================================================================
class BottomCase:
    """K distinct instances and the per-instance inputs of predict, range, predict, normal"""

    def __init__(self, K, seed=41):
        rng = np.random.default_rng(seed)
        self.K = K
        self.x, self.P = V.bottom_state(K, seed=seed, tilt=0.2)
        self.v = np.c_[rng.normal(0.5, 0.1, K), rng.normal(0, 0.1, K), rng.normal(0, 0.05, K)]
        self.z = 10.0 / 0.866 + rng.normal(0, 0.05, K)
        self.zc = rng.uniform(0.01, 0.03, K)
        self.n = V.unit(np.c_[rng.normal(0, 0.05, (K, 2)), np.ones(K)])
        A = rng.normal(0, 0.01, (K, 2, 2))
        self.nc = A @ np.swapaxes(A, 1, 2) + np.eye(2) * rng.uniform(2e-4, 8e-4, (K, 1, 1))

    def make(self, cls, idx=None, P=None):
        idx = np.arange(self.K) if idx is None else np.asarray(idx)
        f = cls(len(idx))
        f.init(self.x[idx], (self.P if P is None else P)[idx])
        f.set_process_noise(S.BOTTOM_Q)
        f.set_velocity(self.v[idx])
        return f

    def predict(self, f, idx=slice(None)):
        f.predict(0.2)

    def range(self, f, idx=slice(None), **kw):
        f.update_range(self.z[idx], self.zc[idx], *S.BEAMS[0], **kw)

    def normal(self, f, idx=slice(None), **kw):
        f.update_normal(self.n[idx], self.nc[idx], **kw)

    def run(self, idx):
        f = self.make(BottomUKFBatch, idx)
        self.predict(f)
        self.range(f, idx)
        self.predict(f)
        self.normal(f, idx)
        assert not f.get_status().any()
        return f.get_state()


@pytest.fixture(scope="module")
def bottom_case():
    c = BottomCase(17)
    one = [c.run([k]) for k in range(c.K)]
    c.single = (np.concatenate([s[0] for s in one]), np.concatenate([s[1] for s in one]))
    return c


@pytest.mark.parametrize("B", [1, 7, 8, 9, 17])  # 1, IPB-1, IPB, IPB+1, 2 IPB+1
def test_bottom_slot_and_batch_independence(bottom_case, B):
    """k_bottom_predict / k_bottom_range / k_bottom_normal"""
    c = bottom_case
    for idx in (np.arange(B), np.random.default_rng(B).permutation(c.K)[:B]):
        same(c.run(idx), (c.single[0][idx], c.single[1][idx]))


def test_bottom_normal_mask(bottom_case):
    c = bottom_case

    def call(f, mask, poison):
        n = c.n.copy()
        if poison is not None:
            n[poison, 1] = np.nan
        f.update_normal(n, c.nc, mask=mask)
    mask_contract(lambda: c.make(BottomUKFBatch), call, c.K, off=11)
    # a non-finite covariance is UWVK_ENAN too (shared and per-instance), a zero normal UWVK_EINVAL
    f = c.make(BottomUKFBatch)
    before = f.get_state()
    nc = c.nc.copy()
    nc[3, 0, 1] = np.inf
    n0 = c.n.copy()
    n0[5] = 0.0
    for n, cov, code in ((c.n, nc, 2), (c.n, np.array([[4e-4, np.nan], [0.0, 4e-4]]), 2), (n0, c.nc, 1)):
        with pytest.raises(engine.UWVKError) as e:
            f.update_normal(n, cov)
        assert e.value.code == code
    same(f.get_state(), before)


def test_bottom_normal_cov_shared_vs_per_instance(bottom_case):
    c = bottom_case
    cov = np.array([[4e-4, 1e-4], [1e-4, 6e-4]])
    f, g = c.make(BottomUKFBatch), c.make(BottomUKFBatch)
    f.update_normal(c.n, cov)
    g.update_normal(c.n, np.tile(cov, (c.K, 1, 1)))  # identical rows: bitwise the shared form
    same(f.get_state(), g.get_state())
    # differing rows: the oracle.  Scene: test_small_twin.py::test_bottom_sequence[per_instance_cov]
    # at B = 5 (4.2e-14 there); here 17 instances of the same generator
    B = 17
    x, P = V.bottom_state(B)
    g, o = BottomUKFBatch(B), O.OracleBottomBatch(B)
    for h in (g, o):
        h.init(x, P)
        h.set_process_noise(S.BOTTOM_Q)
    S.bottom_sequence((g, o), B, steps=10, per_instance_cov=True)
    es, ec = S.bottom_err(*g.get_state(), *o.get_state())
    assert es < TOL and ec < TOL, (es, ec)
    assert not g.get_status().any()


@pytest.mark.parametrize("pivot", ["leading", "last"])
@pytest.mark.parametrize("op", ["predict", "range", "normal"])
def test_bottom_notpd(bottom_case, op, pivot):
    """one finite, symmetric, indefinite Sigma among 2 IPB+1 instances"""
    c, j = bottom_case, 10  # the third lane group of the second block
    P = c.P.copy()
    if pivot == "leading":
        P[j, 0, 0] = -0.1
        assert pivots(P[j])[0] < 0
    else:
        P[j, 2, 2] = -0.002
        d = pivots(P[j])
        assert (d[:2] > 0).all() and d[2] < 0
    notpd_contract(c.make(BottomUKFBatch, P=P), c.make(BottomUKFBatch), c.make(O.OracleBottomBatch),
                   lambda f: getattr(c, op)(f), j, S.bottom_err)


def test_bottom_failed_respread_leaves_state_untouched(bottom_case):
    """The first Cholesky succeeds and the one in apply_delta fails: a finite but
    negative range variance makes Sigma - C K^T indefinite.  The kernel leaves
    (x, P) untouched and sets the status bit (include/uwvk.h);
    the oracle reports UWVK_ENOTPD with Sigma already reduced, so it is only
    checked to fail."""
    c, j = bottom_case, 12
    zc = c.zc.copy()
    zc[j] = -0.05
    bad, healthy = c.make(BottomUKFBatch), c.make(BottomUKFBatch)
    before = bad.get_state()
    bad.update_range(c.z, zc, *S.BEAMS[0])
    healthy.update_range(c.z, c.zc, *S.BEAMS[0])
    others = np.arange(c.K) != j
    st = bad.get_status()
    assert st[j] & NOTPD and not st[others].any(), st
    same(bad.get_state(), before, j)
    same(bad.get_state(), healthy.get_state(), others)
    o = O.OracleBottomBatch(1)
    o.init(c.x[j:j + 1], c.P[j:j + 1])
    with pytest.raises(RuntimeError, match="NOTPD"):
        o.update_range(c.z[j:j + 1], zc[j:j + 1], *S.BEAMS[0])


def test_bottom_tilted_normals_against_oracle():
    """normals up to 60 degrees from +e3.  Scene: test_small_twin.py::
    test_bottom_sequence[tilted_60deg] (oracle and twin 2.6e-13 apart)."""
    B = 17
    x, P = V.bottom_state(B, tilt=0.5)
    x[:, 1:] = S.limit_tilt(x[:, 1:])
    assert np.degrees(np.arccos(x[:, 3])).max() > 45.0
    g, o = BottomUKFBatch(B), O.OracleBottomBatch(B)
    for f in (g, o):
        f.init(x, P)
        f.set_process_noise(S.BOTTOM_Q)
    S.bottom_sequence((g, o), B, steps=10, per_instance_cov=True, tilt=0.5)
    es, ec = S.bottom_err(*g.get_state(), *o.get_state())
    assert es < TOL and ec < TOL, (es, ec)
    assert not g.get_status().any()


# ===========================================================================
# IndirectPoseUKF
# ===========================================================================
class IPoseCase:
    """K distinct instances of the 0.02 rad scene, the dense Q"""

    def __init__(self, K, right, seed=11):
        self.K, self.right = K, right
        self.ref, _, _, self.marker, self.px = V.ipose_scene(K, seed)
        self.ipe = np.random.default_rng(2).normal(0, 0.1, (K, 3))
        self.fcov, self.fpos, self.cm, self.cam, self.cib = V.visual_common(K)

    def make(self, cls=IndirectPoseUKFBatch, idx=None, ori_std=(0.01, 0.01, 0.02)):
        """(an oracle batch takes its side from O.so3_side(self.right) around its calls)"""
        idx = np.arange(self.K) if idx is None else np.asarray(idx)
        f = cls(len(idx))
        if cls is IndirectPoseUKFBatch and not self.right:
            f.set_so3_right(False)
        f.init([0.1, 0.1, 0.2], list(ori_std), 20.0, self.ipe[idx], [0.5, 0.5, 0.5])
        f.set_process_noise(S.ipose_q())
        f.set_pose_reference(self.ref[idx])
        return f

    def visual(self, f, idx=slice(None), px=None, fcov=None, marker=None, cm=None, **kw):
        f.update_visual(self.px[idx] if px is None else px, self.fcov if fcov is None else fcov, self.fpos,
                        self.marker[idx] if marker is None else marker, self.cm if cm is None else cm, self.cam,
                        self.cib, **kw)

    def run(self, idx):
        f = self.make(idx=idx)
        for step in range(2):
            f.predict(0.1)
            self.visual(f, idx)
        assert not f.get_status().any()
        return f.get_state()


@pytest.fixture(scope="module", params=[True, False], ids=["right", "left"])
def ipose_case(request):
    c = IPoseCase(9, request.param)
    one = [c.run([k]) for k in range(c.K)]
    c.single = (np.concatenate([s[0] for s in one]), np.concatenate([s[1] for s in one]))
    return c


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 9])  # IPB = 4 (predict) and 2 (visual)
def test_ipose_slot_and_batch_independence(ipose_case, B):
    """k_ipose_predict<0/1>, k_ipose_visual<0/1>"""
    c = ipose_case
    for idx in (np.arange(B), np.random.default_rng(B).permutation(c.K)[:B]):
        same(c.run(idx), (c.single[0][idx], c.single[1][idx]))


def test_ipose_visual_mask(ipose_case):
    c = ipose_case

    def call(f, mask, poison):
        px = c.px.copy()
        if poison is not None:
            px[poison, 2, 0] = np.nan
        c.visual(f, px=px, mask=mask)
    mask_contract(c.make, call, c.K, off=4)


def test_ipose_shared_vs_per_instance(ipose_case):
    c = ipose_case
    # feature covariance (nf, 2, 2) against (B, nf, 2, 2) with identical rows: bitwise
    f, g = c.make(), c.make()
    c.visual(f)
    c.visual(g, fcov=np.tile(c.fcov, (c.K, 1, 1, 1)))
    same(f.get_state(), g.get_state())
    # one marker pose (7,) against (B, 7): every instance watches marker 0 from reference
    # pose 0 (the initial position errors differ)
    f, g = c.make(), c.make()
    for h in (f, g):
        h.set_pose_reference(np.tile(c.ref[0], (c.K, 1)))
    px = np.tile(c.px[0], (c.K, 1, 1))
    c.visual(f, px=px, marker=c.marker[0])
    c.visual(g, px=px, marker=np.tile(c.marker[0], (c.K, 1)))
    same(f.get_state(), g.get_state())
    assert not f.get_status().any()
    # differing rows: the oracle.  Scene: test_small_twin.py::
    # test_ipose_small_scene_per_instance_feature_cov (5.4e-12 / 1.8e-12 there)
    B = 5
    g, o = IndirectPoseUKFBatch(B), O.OracleIndirectPoseBatch(B)
    if not c.right:
        g.set_so3_right(False)
    with O.so3_side(c.right):
        S.ipose_small_run((g, o), B, S.per_instance_fcov(B, 4))
    es, ec = S.ipose_err(*g.get_state(), *o.get_state())
    assert es < TOL and ec < TOL, (es, ec)


def _ipose_with_indefinite(c, cls, j, pivot, bad):
    """Sigma cannot be set through the ABI, so it is driven indefinite: two masked
    visual updates shrink instance j's Sigma alone, then one predict with a Q that
    has one negative entry (finite, shared) takes that entry of j's Sigma below
    zero while every other instance stays positive definite."""
    f = c.make(cls, ori_std=(0.02, 0.02, 0.02))
    if bad:
        m = np.arange(c.K) == j
        for k in range(2):
            c.visual(f, mask=m)
    Qn = np.zeros((6, 6))
    if pivot == "leading":
        Qn[0, 0] = -5.0
    else:
        Qn[5, 5] = -1e-2
    f.set_process_noise(Qn)
    f.predict(0.1)
    f.set_process_noise(S.ipose_q())
    return f


@pytest.mark.parametrize("pivot", ["leading", "last"])
@pytest.mark.parametrize("op", ["predict", "visual"])
def test_ipose_notpd(ipose_case, op, pivot):
    c, j = ipose_case, 5  # shares a block with 4, 6, 7 in predict and with 4 in the visual update
    bad, healthy = (_ipose_with_indefinite(c, IndirectPoseUKFBatch, j, pivot, b) for b in (True, False))
    P = bad.get_state()[1]
    d = pivots(P[j])
    if pivot == "leading":
        assert d[0] < 0
    else:
        assert len(d) == 6 and (d[:5] > 0).all() and d[5] < 0, d
    assert all(np.linalg.eigvalsh(P[i]).min() > 0 for i in range(c.K) if i != j)
    with O.so3_side(c.right):
        oracle = _ipose_with_indefinite(c, O.OracleIndirectPoseBatch, j, pivot, False)
        notpd_contract(bad, healthy, oracle, (lambda f: f.predict(0.1)) if op == "predict" else c.visual, j,
                       S.ipose_err)


def test_ipose_visual_notpd_from_inputs(ipose_case):
    """Sigma fine, the inputs make a Cholesky fail: an indefinite cov_marker_pose
    (shared, so a mask selects the one instance; first Cholesky) and one negative
    per-instance pixel variance (Sigma - C K^T indefinite; the re-spread)."""
    c, j = ipose_case, 4
    others = np.arange(c.K) != j
    cm = c.cm.copy()
    cm[1, 1] = -1e-4
    f = c.make()
    before = f.get_state()
    c.visual(f, cm=cm, mask=~others)
    st = f.get_status(clear=True)
    assert st[j] & NOTPD and not st[others].any()
    same(f.get_state(), before)
    c.visual(f, cm=cm)  # no mask: every instance fails, none changes
    assert (f.get_status(clear=True) & NOTPD).all()
    same(f.get_state(), before)
    assert not f.get_status().any()
    fcov = np.tile(c.fcov, (c.K, 1, 1, 1))
    fcov[j, 2] = -0.01 * np.eye(2)
    healthy = c.make()
    c.visual(f, fcov=fcov)
    c.visual(healthy)
    st = f.get_status()
    assert st[j] & NOTPD and not st[others].any(), st
    same(f.get_state(), before, j)
    same(f.get_state(), healthy.get_state(), others)


@pytest.mark.parametrize("right", [True, False], ids=["right", "left"])
def test_ipose_rotated_process_noise_large_errors(right):
    """Two visual updates on the 0.3 rad scene leave the estimated orientation
    error far from identity, then 5 predicts with the dense Q: R Q_o R^T with
    R != I.  Scene: test_small_twin.py::test_ipose_predict_and_visual_large_errors
    with nf = 4, steps = 2 (oracle and twin 3e-13 apart, both sides)."""
    B = 5
    g, o = IndirectPoseUKFBatch(B), O.OracleIndirectPoseBatch(B)
    if not right:
        g.set_so3_right(False)
    with O.so3_side(right):
        S.ipose_large_error_run((g, o), B, V.CORNERS, steps=2)
        x = g.get_state()[0]
        assert (2 * np.arccos(np.abs(x[:, 3])) > 0.1).all()  # not the Rm = I case
        es, ec = S.ipose_err(*g.get_state(), *o.get_state())
        assert es < TOL and ec < TOL, (es, ec)
        for k in range(5):
            g.predict(0.1)
            o.predict(0.1)
    es, ec = S.ipose_err(*g.get_state(), *o.get_state())
    assert es < TOL and ec < TOL, (es, ec)
    np.testing.assert_allclose(g.get_corrected_pose(), o.get_corrected_pose(), atol=1e-9)
    assert not g.get_status().any()


@pytest.mark.parametrize("right", [True, False], ids=["right", "left"])
@pytest.mark.parametrize("nf", [0, 1, 7])
def test_ipose_feature_counts(nf, right):
    """Scenes: test_small_twin.py::test_ipose_predict_and_visual_large_errors with
    nf = 1 and nf = 7, steps = 4 (at most 3.2e-13); the 7 points are V.CORNERS7, all in front of the
    camera (ipose_scene asserts zc > 1)."""
    B = 5
    g, o = IndirectPoseUKFBatch(B), O.OracleIndirectPoseBatch(B)
    if not right:
        g.set_so3_right(False)
    with O.so3_side(right):
        if nf == 0:
            S.ipose_small_run((g,), B, steps=1)
            before = g.get_state()
            ref, _, _, marker, _ = V.ipose_scene(B)
            g.update_visual(np.zeros((B, 0, 2)), np.zeros((0, 2, 2)), np.zeros((0, 3)), marker, np.eye(6) * 1e-4,
                            V.CAMERA, V.CAM_IN_BODY)  # returns UWVK_OK
            same(g.get_state(), before)
            return
        corners = V.CORNERS[:1] if nf == 1 else V.CORNERS7
        S.ipose_large_error_run((g, o), B, corners, steps=4)
    es, ec = S.ipose_err(*g.get_state(), *o.get_state())
    assert es < TOL and ec < TOL, (es, ec)
    assert not g.get_status().any()


# ===========================================================================
# PoseUKF visual-landmark update (one 128-lane block per instance)
# ===========================================================================
class PoseCase:
    """3 PoseUKF states after a 60-epoch log (from the oracle) and their marker scene"""

    def __init__(self, dof):
        self.dof, self.K = dof, 3
        cfg, self.uwv, log = pose_setup(3, dof=dof, epochs=60)
        o = O.OraclePoseBatch(3, dof)
        o.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, self.uwv)
        o.set_process_noise_from_config(cfg, log["dt"])
        o.run_log(log)
        self.x, self.P = o.get_state()
        _, _, self.marker, self.px = V.pose_scene(self.x)
        self.fcov, self.fpos, self.cm, self.cam, self.cib = V.visual_common(3)

    def make(self, cls=engine.PoseUKFBatch, idx=None, x=None, P=None):
        idx = np.arange(self.K) if idx is None else np.asarray(idx)
        f = cls(len(idx), self.dof)
        f.init_from_state((self.x if x is None else x)[idx], (self.P if P is None else P)[idx],
                          abi.Location(synth.LAT0, synth.LON0, 0.0), self.uwv, abi.PoseParameter())
        return f

    def visual(self, f, idx=slice(None), px=None, fcov=None, marker=None, cm=None, **kw):
        f.update_visual(self.px[idx] if px is None else px, self.fcov if fcov is None else fcov, self.fpos,
                        self.marker[idx] if marker is None else marker, self.cm if cm is None else cm, self.cam,
                        self.cib, **kw)

    def err(self, xa, Pa, xo, Po):
        return float(state_err(xa, xo, Po, self.dof).max()), float(cov_err(Pa, Po).max())


@pytest.fixture(scope="module", params=[53, 26])
def pose_case(request):
    return PoseCase(request.param)


def test_pose_visual_batch_independence(pose_case):
    """k_pose_visual: B = 3 against B = 1, two calls"""
    c = pose_case
    g = c.make()
    for rep in range(2):
        c.visual(g)
    for k in range(c.K):
        g1 = c.make(idx=[k])
        for rep in range(2):
            c.visual(g1, [k])
        x1, P1 = g1.get_state()
        np.testing.assert_array_equal(x1[0], g.get_state()[0][k])
        np.testing.assert_array_equal(P1[0], g.get_state()[1][k])
    assert not g.get_status().any()


def test_pose_visual_mask(pose_case):
    c = pose_case

    def call(f, mask, poison):
        px = c.px.copy()
        if poison is not None:
            px[poison, 1, 1] = np.nan
        c.visual(f, px=px, mask=mask)
    mask_contract(c.make, call, c.K, off=2)


def test_pose_visual_marker_shared_vs_per_instance(pose_case):
    """every instance starts from state 0 (positions shifted) and watches marker 0"""
    c = pose_case
    x = np.tile(c.x[0], (c.K, 1))
    x[:, :3] += np.random.default_rng(8).normal(0, 0.05, (c.K, 3))
    P = np.tile(c.P[0], (c.K, 1, 1))
    px = np.tile(c.px[0], (c.K, 1, 1))
    f, g = c.make(x=x, P=P), c.make(x=x, P=P)
    c.visual(f, px=px, marker=c.marker[0])
    c.visual(g, px=px, marker=np.tile(c.marker[0], (c.K, 1)))
    same(f.get_state(), g.get_state())
    assert not f.get_status().any()
    assert np.abs(f.get_state()[0][1] - f.get_state()[0][2]).max() > 1e-3  # the rows do differ
    # differing rows against the oracle: test_small_filters.py::test_gpu_pose_visual_landmark


@pytest.mark.parametrize("pivot", ["leading", "last"])
def test_pose_visual_notpd(pose_case, pivot):
    """an indefinite filter Sigma in one of three instances.  Scene of the healthy
    ones: test_small_twin.py::test_pose_visual_update, dof 53 / 26 with nf = 4 (3.3e-12)."""
    c, j = pose_case, 1
    P = c.P.copy()
    k = 0 if pivot == "leading" else c.dof - 1
    P[j, k, k] = -abs(P[j, k, k])
    d = pivots(P[j])
    assert len(d) == k + 1 and (d[:k] > 0).all() and d[k] < 0
    notpd_contract(c.make(P=P), c.make(), c.make(O.OraclePoseBatch), c.visual, j, c.err)


def test_pose_visual_notpd_from_inputs(pose_case):
    """as test_ipose_visual_notpd_from_inputs"""
    c, j = pose_case, 2
    others = np.arange(c.K) != j
    cm = c.cm.copy()
    cm[4, 4] = -1e-5
    f = c.make()
    before = f.get_state()
    c.visual(f, cm=cm, mask=~others)
    st = f.get_status(clear=True)
    assert st[j] & NOTPD and not st[others].any()
    same(f.get_state(), before)
    fcov = np.tile(c.fcov, (c.K, 1, 1, 1))
    fcov[j, 1] = -0.01 * np.eye(2)
    healthy = c.make()
    c.visual(f, fcov=fcov)
    c.visual(healthy)
    st = f.get_status()
    assert st[j] & NOTPD and not st[others].any(), st
    same(f.get_state(), before, j)
    same(f.get_state(), healthy.get_state(), others)


@pytest.mark.parametrize("nf", [0, 1, 7])
def test_pose_visual_feature_counts(nf):
    """Scenes: test_small_twin.py::test_pose_visual_update, dof 53 with nf = 1 (5.9e-14)
    and nf = 7 (4.3e-13; 4 px^2 pixels, V.SEVEN_PIXEL_VAR); pose_scene asserts zc > 1."""
    c = PoseCase(53)
    g, o = c.make(), c.make(O.OraclePoseBatch)
    before = g.get_state()
    if nf == 0:
        g.update_visual(np.zeros((3, 0, 2)), np.zeros((0, 2, 2)), np.zeros((0, 3)), c.marker, c.cm, c.cam, c.cib)
        same(g.get_state(), before)
        return
    corners = V.CORNERS[:1] if nf == 1 else V.CORNERS7
    _, _, marker, px = V.pose_scene(c.x, corners=corners)
    fcov, fpos, cm, cam, cib = V.visual_common(3, corners, V.SEVEN_PIXEL_VAR if nf == 7 else 0.09)
    for rep in range(2):
        for f in (g, o):
            f.update_visual(px, fcov, fpos, marker, cm, cam, cib)
    es, ec = c.err(*g.get_state(), *o.get_state())
    assert es < TOL and ec < TOL, (es, ec)
    assert not g.get_status().any()
