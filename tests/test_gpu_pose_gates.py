"""The d2p95 gate of the PoseUKF kernels, pinned at its limit: the scenes of
tests/pose_gate_scenes.py (each proven on the CPU first:
tests/test_pose_gate_scenes.py), whose measurements are built at d2 = K (1 -+
1e-6), 0.5 and 60 for the state they meet, so the decision of every instance,
ADCP cell and GPS row is known by construction and only then compared with
the oracle's.

 G1 single calls (pose_update of the dense / literal kernels, psp_update of
    k_psp_update): water velocity and geographic position, per-instance and
    shared R, neighbours deciding differently, one instance masked out with
    NaN in its value and covariance; xy, delayed_xy and velocity at d2 = 60
    (no gate).  `accepted` is the constructed vector, accepted instances match
    the oracle to 1e-9, rejected and masked ones are bitwise the state before.
 G2 the ADCP cell loop in run_log on every epoch kernel (dense, psp, pd, pair;
    with a pressure sample on the ADCP epoch: the pressure-capable kernels):
    accept counts 1, 3, 2, 4, 0, 2, unlike between the halves of every pair
    unit; an all-rejected instance is bitwise the run without the ADCP flag;
    a half of a pair unit does not see its partner's decisions.
 G3 GEO rows in run_log_fixes (k_psp_fix: after XY and Z of the same epoch,
    alone, on the last epoch): the constructed counts, bitwise the
    cut-and-single-call run, the oracle to 1e-7.

Paths as in tests/test_gpu_pose_edges.py, and literal (set_literal_apply_delta).
Tolerances (tests/test_gpu_parity.py): 1e-9 sigma for a single call, 1e-7 for
a log, 1e-9 pair against the one-instance kernel.

Measured on an MI355X (max over instances, paths, layouts and sides; state in
the oracle's sigma, covariance relative to sqrt(P_ii P_jj)):
 G1 the state the calls start from (five predicts, four updates) 4.2e-11 /
    1.0e-10; accepted instances after the gated call 3.0e-11 / 1.0e-10; the
    ungated kinds at d2 = 60 5.7e-11 / 1.0e-10; rejected and masked bitwise;
 G2 run_log against the oracle 5.0e-11 / 6.4e-11; pair against the
    one-instance kernel 0 / 1.4e-16;
 G3 run_log_fixes against the oracle 5.1e-11 / 1.8e-12.
No kernel fault was found: every test passed on the unchanged kernels.

Mutants of csrc/ this file was run against (tests failed of 98), and whether
tests/test_gpu_parity.py, test_gpu_fixes.py and test_gpu_pair_rankm.py (105
tests) see them at the commit before this file:
  kD2P95 = 6.0 (uwvk_dev.hpp)                                66   unseen
  d2 without its cross term in psp_update                    47   unseen
  gate 0 for MK_GEO in do_update_pos (uwvk_psp_k.hip)        13   2 (*)
  the pair kernel's ADCP call with gate 0                    12   1 (*)
  k_psp_fix's GEO counter incremented unconditionally         5   2 (*)
  gate 0 for MK_WATER in the dense / literal do_update        8   unseen
(*) test_gpu_fixes.py::test_fixes_match_oracle: the GPS row a kilometre off
(d2 ~ 1e6) and the ADCP rows of its 900-epoch C4 log (d2 up to 788) catch a
gate that is switched off or miscounted, not one that is misplaced.  With a
pressure sample on the ADCP epoch the pair handle runs that epoch on the
one-instance kernel, so the pair mutant fails the plain variants only."""
import contextlib
import functools

import numpy as np
import pytest

import numpy_twin as T
import oracle_ctypes as O
import pose_gate_scenes as G
import pose_scenes as PS
from helpers import cov_err, state_err
from uwvk import engine

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-9
TOL_LOG = 1e-7
TOL_PAIR = 1e-9
SIDES = ["right", "left"]
SINGLE_PATH_DOF = [("dense", 53), ("literal", 53), ("psp", 53), ("psp", 26)]
PATH_DOF = [("dense", 53), ("psp", 53), ("pd", 53), ("pair", 53), ("psp", 26), ("pair", 26)]
# path, dof, batch, side: every path at batch 6, the pair kernel on both SO3
# sides, the odd batch on the one-instance kernels it falls back to
ADCP_CASES = ([(p, d, 6, "right") for p, d in PATH_DOF] + [("pair", 53, 6, "left"), ("pair", 26, 6, "left"),
                                                            ("pd", 53, 5, "right"), ("psp", 26, 5, "right")])
NAMES = ("state", "covariance", "accept counts", "status", "rotation rate")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")


@contextlib.contextmanager
def sided(right):
    """the oracle and the twin (the scene builder) on one SO3 side"""
    prev = T.SO3_RIGHT
    T.SO3_RIGHT = right
    try:
        with O.so3_side(right):
            yield
    finally:
        T.SO3_RIGHT = prev


def handle(path, dof, B, right=True):
    g = engine.PoseUKFBatch(B, dof)
    g.set_so3_right(right)
    if path == "dense":
        g.set_dense_sigma(True)
    elif path == "literal":
        g.set_literal_apply_delta(True)
    elif path == "psp":
        g.set_pair(False)
        g.set_param_block(False)
    elif path == "pd":
        g.set_pair(False)
    else:
        assert path == "pair" and B % 2 == 0
    return g


def check_path(g, path, dof):
    assert g.pair_active() == (1 if path == "pair" else 0)
    if path != "dense":
        assert g.param_block() == (1 if dof == 53 and path in ("pd", "pair") else 0)


def errors(x, P, xo, Po, dof):
    assert np.isfinite(x).all() and np.isfinite(P).all()
    np.testing.assert_array_equal(P, np.swapaxes(P, 1, 2))
    return float(state_err(x, xo, Po, dof).max()), float(cov_err(P, Po).max())


# ---- G1. single calls --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_ref(dof, kind, shared, right):
    with sided(right):
        sc = G.single_scene(dof, kind, shared) if kind in G.GATED else G.ungated_scene(dof, kind)
        if kind in G.GATED:
            ref = G.oracle_single(sc, dof)
        else:
            o = G.single_state(O.OraclePoseBatch(G.B_SINGLE, dof), sc["log"])
            acc = o.update(kind, sc["mu"], sc["cov"], extra=sc["extra"])
            ref = o.get_state() + (acc,)
    return sc, ref


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shared", [False, True], ids=["per_instance_R", "shared_R"])
@pytest.mark.parametrize("kind", G.GATED)
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
def test_single_gated(path, dof, kind, shared, side):
    right = side == "right"
    sc, (xo, Po, acc_o) = single_ref(dof, kind, shared, right)
    g = G.single_state(handle(path, dof, G.B_SINGLE, right), sc["log"])
    x0, P0 = g.get_state()
    e0 = errors(x0, P0, sc["x"], sc["P"], dof)
    assert max(e0) < TOL_STEP, e0  # the state the scene was built for
    assert not g.get_status().any()
    acc = g.update(kind, sc["mu"], sc["cov"], extra=sc["extra"], mask=sc["mask"])
    x, P = g.get_state()
    np.testing.assert_array_equal(acc, sc["accept"], err_msg="against the constructed decisions")
    np.testing.assert_array_equal(acc, acc_o, err_msg="against the oracle")
    assert acc[G.MASKED] == 0
    np.testing.assert_array_equal(g.get_status(), np.zeros(G.B_SINGLE, np.uint32))  # no UWVK_ST_NAN for the masked one
    took = sc["accept"].astype(bool)
    e = errors(x[took], P[took], xo[took], Po[took], dof)
    print("%s dof %d %s %s %s: before %.3g %.3g, accepted %.3g %.3g"
          % ((path, dof, kind, "shared" if shared else "per-instance", side) + e0 + e))
    assert max(e) < TOL_STEP, e
    assert (x[took] != x0[took]).any(axis=1).all()
    np.testing.assert_array_equal(x[~took], x0[~took], err_msg="a rejected / masked instance's state")
    np.testing.assert_array_equal(P[~took], P0[~took], err_msg="a rejected / masked instance's covariance")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", G.UNGATED)
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
def test_single_ungated_far_out(path, dof, kind, side):
    """xy, delayed_xy, velocity at d2 = 60: they share do_update_pos / psp_update with the gated kinds"""
    right = side == "right"
    sc, (xo, Po, acc_o) = single_ref(dof, kind, False, right)
    g = G.single_state(handle(path, dof, G.B_SINGLE, right), sc["log"])
    x0 = g.get_state()[0]
    acc = g.update(kind, sc["mu"], sc["cov"], extra=sc["extra"])
    assert acc.all() and acc_o.all()
    assert not g.get_status().any()
    x, P = g.get_state()
    e = errors(x, P, xo, Po, dof)
    print("%s dof %d %s %s: %.3g %.3g" % ((path, dof, kind, side) + e))
    assert max(e) < TOL_STEP, e
    assert (x != x0).any(axis=1).all()


# ---- G2. ADCP cells in run_log ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adcp_ref(B, dof, pressure, right, patterns=G.ADCP_PATTERNS):
    with sided(right):
        sc = G.adcp_scene(B, dof, pressure, patterns)
        o = PS.start(O.OraclePoseBatch(B, dof), sc["log"])
        counts = o.run_log(sc["log"])
        ref = o.get_state() + (counts,)
    np.testing.assert_array_equal(sc["oracle_accept"], sc["accept"])
    np.testing.assert_array_equal(counts[:, 2], sc["counts"])
    return sc, ref


def run(path, dof, log, right):
    B = log["batch"]
    g = PS.start(handle(path, dof, B, right), log)
    check_path(g, path, dof)
    acc = engine.DeviceBuffer(np.zeros((B, 4), np.uint32))
    g.run_log(g.upload_log(log), accept_counts=acc)
    x, P = g.get_state()
    return x, P, acc.read(np.uint32, (B, 4)), g.get_status(), g.get_rotation_rate()


@pytest.mark.parametrize("pressure", [False, True], ids=["plain", "pressure"])
@pytest.mark.parametrize("path,dof,B,side", ADCP_CASES)
def test_adcp_run_log(path, dof, B, side, pressure):
    right = side == "right"
    sc, (xo, Po, counts) = adcp_ref(B, dof, pressure, right)
    got = run(path, dof, sc["log"], right)
    np.testing.assert_array_equal(got[2][:, 2], sc["counts"], err_msg="against the constructed counts")
    np.testing.assert_array_equal(got[2], counts, err_msg="against the oracle")
    assert not got[3].any()
    e = errors(got[0], got[1], xo, Po, dof)
    print("%s dof %d B %d %s %s run_log: %.3g %.3g" % ((path, dof, B, side, "pressure" if pressure else "plain") + e))
    assert max(e) < TOL_LOG, e
    if B > 4:  # instance 4: all four cells rejected -> bitwise the run without the ADCP flag
        bare = run(path, dof, G.without_adcp(sc["log"]), right)
        assert not bare[2][:, 2].any()
        for name, u, v in zip(NAMES, got, bare):
            np.testing.assert_array_equal(u[4], v[4], err_msg=name)
        assert (got[0][3] != bare[0][3]).any()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("pressure", [False, True], ids=["plain", "pressure"])
@pytest.mark.parametrize("dof", [53, 26])
def test_adcp_pair_against_one_instance(dof, pressure, side):
    right = side == "right"
    sc, _ = adcp_ref(6, dof, pressure, right)
    pair = run("pair", dof, sc["log"], right)
    one = run("pd" if dof == 53 else "psp", dof, sc["log"], right)
    np.testing.assert_array_equal(pair[2], one[2])
    np.testing.assert_array_equal(pair[3], one[3])
    es, ec = state_err(pair[0], one[0], one[1], dof).max(), cov_err(pair[1], one[1]).max()
    print("dof %d %s %s pair vs one-instance: %.3g %.3g" % (dof, "pressure" if pressure else "plain", side, es, ec))
    assert es < TOL_PAIR and ec < TOL_PAIR


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("pressure", [False, True], ids=["plain", "pressure"])
@pytest.mark.parametrize("dof", [53, 26])
def test_adcp_partner_independence(dof, pressure, side):
    """Pair unit 2 holds instances 4 (lower half, all cells rejected) and 5;
    unit 1 holds 2 and 3 (upper half, all cells accepted).  With instance 4's
    rows rebuilt for all-accept, and instance 3's for all-reject, the partners
    5 and 2 (and unit 0) come out bitwise as before, accept counts included."""
    right = side == "right"
    base_sc, _ = adcp_ref(6, dof, pressure, right)
    pat = list(G.ADCP_PATTERNS)
    pat[4], pat[3] = G.ALL_ACCEPT, G.ALL_REJECT
    swap_sc, _ = adcp_ref(6, dof, pressure, right, tuple(pat))
    np.testing.assert_array_equal(swap_sc["counts"], [1, 3, 2, 0, 4, 2])
    base = run("pair", dof, base_sc["log"], right)
    swap = run("pair", dof, swap_sc["log"], right)
    np.testing.assert_array_equal(swap[2][:, 2], swap_sc["counts"])
    np.testing.assert_array_equal(base[2][:, 2], base_sc["counts"])
    for i in (0, 1, 2, 5):
        for name, u, v in zip(NAMES, base, swap):
            np.testing.assert_array_equal(u[i], v[i], err_msg="%s of instance %d" % (name, i))
    for i in (3, 4):
        assert (base[0][i] != swap[0][i]).any()
    assert not base[3].any() and not swap[3].any()


# ---- G3. GEO rows in run_log_fixes -------------------------------------------------------------
def _fix_paths():
    from test_gpu_fixes import PATHS
    out = [pytest.param(*(p.values + (False,)), id=p.id) for p in PATHS]
    return out + [pytest.param(6, 53, True, True, (0, 0), True, id="literal")]


@functools.lru_cache(maxsize=None)
def geo_ref(B, dof, right):
    with sided(right):
        sc = G.geo_scene(B, dof)
        ref = G.oracle_run_fixes(sc["log"], sc["fixes"], dof)
    np.testing.assert_array_equal(sc["oracle_accept"], sc["accept"])
    return sc, ref


@pytest.mark.parametrize("B,dof,pd,right,kernels,literal", _fix_paths())
def test_geo_fixes(B, dof, pd, right, kernels, literal):
    from test_gpu_fixes import _by_cuts, _handle, _same, _with_fixes
    sc, (xo, Po, acc_o, facc_o) = geo_ref(B, dof, right)
    log, fx = sc["log"], sc["fixes"]
    ga, gb = (_handle(engine, log, dof, pd, right, literal) for _ in range(2))
    if not literal:
        assert (ga.pair_active(), ga.param_block()) == kernels
    got = _with_fixes(engine, ga, log, fx)
    np.testing.assert_array_equal(got["facc"][:, 2], sc["counts"], err_msg="against the constructed counts")
    np.testing.assert_array_equal(got["facc"], facc_o, err_msg="against the oracle")
    np.testing.assert_array_equal(got["facc"][:, :2], [[1, 1]] * B)
    ref = _by_cuts(engine, gb, log, fx)
    _same(got, ref)
    assert not got["status"].any()
    e = errors(got["x"], got["P"], xo, Po, dof)
    print("geo fixes B %d dof %d pd %d right %d literal %d: %.3g %.3g" % ((B, dof, pd, right, literal) + e))
    assert max(e) < TOL_LOG, e
