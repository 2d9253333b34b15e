"""The PoseUKF gate scenes of tests/pose_gate_scenes.py are what they claim
before a kernel sees them.

For every scene, both layouts (53 / 26 DOF) and both SO3 sides:
  * the oracle and the numpy twin take the constructed decision for every
    instance, cell and GEO row (at DELTA = 1e-6; the same at 1e-9 is printed,
    not required);
  * the twin's own d2 is within 1e-9 relative of the target;
  * the oracle's run_log over the rebuilt log is bitwise its per-call loop,
    with the constructed accept counts;
  * a rejected (or masked) call leaves the oracle bitwise unchanged;
  * teeth: at every threshold measurement, d2 without the off-diagonal of S^-1,
    d2 with gps_in_body = 0 and d2 with the neighbouring cell's weighting are
    each more than 1e-2 relative away from K, so a kernel with one of these
    faults decides differently at K (1 +- 1e-6).

Measured (max over scenes, layouts and sides): |d2 / target - 1| 7.8e-16
(ADCP), 2.7e-10 (GEO: the round trip through latitude / longitude); oracle
against twin after the calls 1.2e-13 sigma; the least tooth 6.9e-2 (cross
term), 1.3e-1 (lever arm), 7.0e-2 (cell weighting); at DELTA = 1e-9 every
decision of oracle and twin is still the constructed one."""
import numpy as np
import pytest

import numpy_twin as T
import oracle_ctypes as O
import pose_gate_scenes as G
import pose_scenes as PS
from helpers import cov_err, state_err

TOL = 1e-10   # oracle against twin, in the oracle's sigma (tests/test_oracle_twin.py)
D2_TOL = 1e-9
TOOTH = 1e-2
DOFS = [53, 26]


@pytest.fixture(params=["right", "left"])
def side(request):
    right = request.param == "right"
    prev = T.SO3_RIGHT
    T.SO3_RIGHT = right
    with O.so3_side(right):
        yield request.param
    T.SO3_RIGHT = prev


def far_from_k(d2, what):
    assert abs(d2 / G.K - 1.0) > TOOTH, (what, d2)
    return abs(d2 / G.K - 1.0)


def teeth(t, kind, z, R, extra, what):
    """-> (cross, lever arm or cell weighting): the relative distances from K"""
    a = far_from_k(G.twin_d2(t, kind, z, R, extra, cross=False), what + ("cross term",))
    if kind == "geographic":
        b = far_from_k(G.twin_d2(t, kind, z, R, np.zeros(3)), what + ("gps_in_body = 0",))
    else:
        b = far_from_k(G.twin_d2(t, kind, z, R, G.neighbour_cw(extra)), what + ("neighbour's cw",))
    return a, b


def twin_err(t, xo, Po, dof):
    return max(state_err(t.mu[None], xo[None], Po[None], dof).max(), cov_err(t.P[None], Po[None]).max())


# ---- single calls -------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["per_instance_R", "shared_R"])
@pytest.mark.parametrize("kind", G.GATED)
@pytest.mark.parametrize("dof", DOFS)
def test_single_scene(dof, kind, shared, side):
    sc = G.single_scene(dof, kind, shared)
    assert sc["names"] == ("K-", "K+", "in", "out", "K+", "K-", "masked", "K-")
    np.testing.assert_array_equal(sc["accept"], [1, 0, 1, 0, 0, 1, 0, 1])
    assert sc["mask"][G.MASKED] == 0 and np.isnan(sc["mu"][G.MASKED]).all()
    if shared:
        assert sc["cov"].shape == (2, 2)
    else:
        assert np.isnan(sc["cov"][G.MASKED]).all() and len({tuple(c.ravel()) for c in sc["covs"]}) == G.B_SINGLE
    for c in sc["covs"]:
        assert 0.39 < c[0, 1] / np.sqrt(c[0, 0] * c[1, 1]) < 0.51
    xo, Po, acc = G.oracle_single(sc, dof)
    np.testing.assert_array_equal(acc, sc["accept"])
    worst_d2 = worst_e = 0.0
    least = [np.inf, np.inf]
    for i, name in enumerate(sc["names"]):
        untouched = name == "masked" or not sc["accept"][i]
        if untouched:  # bitwise the state before
            np.testing.assert_array_equal(xo[i], sc["x"][i])
            np.testing.assert_array_equal(Po[i], sc["P"][i])
        else:
            assert (xo[i] != sc["x"][i]).any() and (Po[i] != sc["P"][i]).any()
        if name == "masked":
            continue
        t = G.shell(sc["log"], i, dof, sc["x"][i], sc["P"][i])
        ex = G.extra_of(kind, sc["extra"], i)
        d2 = G.twin_d2(t, kind, sc["mu"][i], sc["covs"][i], ex)
        worst_d2 = max(worst_d2, abs(d2 / sc["d2"][i] - 1.0))
        if G.is_threshold(name):
            least = [min(a, b) for a, b in zip(least, teeth(t, kind, sc["mu"][i], sc["covs"][i], ex, (kind, i)))]
        assert bool(t.update(kind, sc["mu"][i], sc["covs"][i], extra=ex)) == bool(sc["accept"][i]), (kind, i, name)
        if untouched:
            np.testing.assert_array_equal(t.mu, sc["x"][i])
        worst_e = max(worst_e, twin_err(t, xo[i], Po[i], dof))
    print("single %s dof %d %s %s: d2 %.3g, oracle vs twin %.3g, teeth %.3g %.3g"
          % (kind, dof, "shared" if shared else "per-instance", side, worst_d2, worst_e, least[0], least[1]))
    assert worst_d2 < D2_TOL and worst_e < TOL
    # printed only: the decisions at DELTA = 1e-9
    fine = G.single_scene(dof, kind, shared, delta=1e-9)
    acc9 = G.oracle_single(fine, dof)[2]
    tw9 = [int(bool(G.shell(fine["log"], i, dof, fine["x"][i], fine["P"][i]).update(
        kind, fine["mu"][i], fine["covs"][i], extra=G.extra_of(kind, fine["extra"], i))))
        for i in range(G.B_SINGLE) if i != G.MASKED]
    print("   DELTA 1e-9: oracle as constructed %s, twin as constructed %s"
          % ((acc9 == fine["accept"]).all(), tw9 == np.delete(fine["accept"], G.MASKED).tolist()))


@pytest.mark.parametrize("kind", G.UNGATED)
@pytest.mark.parametrize("dof", DOFS)
def test_ungated_scene(dof, kind, side):
    """xy, delayed_xy and velocity at d2 = 60: no gate, accepted"""
    sc = G.ungated_scene(dof, kind)
    o = G.single_state(O.OraclePoseBatch(G.B_SINGLE, dof), sc["log"])
    acc = o.update(kind, sc["mu"], sc["cov"], extra=sc["extra"])
    assert acc.all()
    xo, Po = o.get_state()
    worst = 0.0
    for i in range(G.B_SINGLE):
        t = G.shell(sc["log"], i, dof, sc["x"][i], sc["P"][i])
        ex = G.extra_of(kind, sc["extra"], i)
        d2 = G.twin_d2(t, kind, sc["mu"][i], sc["covs"][i], ex)
        assert abs(d2 / 60.0 - 1.0) < D2_TOL, (kind, i, d2)
        assert t.update(kind, sc["mu"][i], sc["covs"][i], extra=ex)
        worst = max(worst, twin_err(t, xo[i], Po[i], dof))
        assert (xo[i] != sc["x"][i]).any()
    print("ungated %s dof %d %s: oracle vs twin %.3g" % (kind, dof, side, worst))
    assert worst < TOL


# ---- ADCP cells in a log ----------------------------------------------------------------
def test_adcp_patterns():
    counts = [sum(G.targets()[n][1] for n in p) for p in G.ADCP_PATTERNS]
    assert counts == [1, 3, 2, 4, 0, 2]
    dec = np.array([[G.targets()[n][1] for n in p] for p in G.ADCP_PATTERNS])
    for u in range(3):  # the halves of a pair unit: unlike counts, and unlike decisions on some cell
        assert counts[2 * u] != counts[2 * u + 1] and (dec[2 * u] != dec[2 * u + 1]).any()
    assert (dec[0, :2] == [0, 1]).all() and (dec[1, :2] == [1, 0]).all()  # reject -> accept, accept -> reject
    assert not dec[4].any() and dec[3].all()
    assert G.ALL_REJECT is G.ADCP_PATTERNS[4] and G.ALL_ACCEPT is G.ADCP_PATTERNS[3]
    assert sum(G.is_threshold(n) for p in G.ADCP_PATTERNS for n in p) >= 18


@pytest.mark.parametrize("pressure", [False, True], ids=["plain", "pressure"])
@pytest.mark.parametrize("batch", [6, 5])
@pytest.mark.parametrize("dof", DOFS)
def test_adcp_scene(dof, batch, pressure, side):
    from uwvk import abi
    sc = G.adcp_scene(batch, dof, pressure)
    log = sc["log"]
    assert log["epochs"] <= 12 and bool(log["flags"][G.ADCP_EPOCH] & abi.EV_PRESSURE) == pressure
    assert not (log["flags"] & abi.EV_EFFORTS).any()
    r = log["adcp_cov"][0, 1] / np.sqrt(log["adcp_cov"][0, 0] * log["adcp_cov"][1, 1])
    assert 0.39 < r < 0.51
    np.testing.assert_array_equal(sc["oracle_accept"], sc["accept"])
    np.testing.assert_array_equal(sc["counts"], [1, 3, 2, 4, 0, 2][:batch])
    row = log["adcp_index"][G.ADCP_EPOCH]
    worst_d2 = worst_e = 0.0
    least = [np.inf, np.inf]
    for i in range(batch):
        t = G.shell(log, i, dof, *[s[i] for s in sc["states"][0]])  # the twin runs the four cells on its own
        for c in range(4):
            xb, Pb = sc["states"][c]
            xa, Pa = sc["states"][c + 1]
            z, cw = log["adcp"][row, c, i], G.CELL_WEIGHTS[c]
            at = G.shell(log, i, dof, xb[i], Pb[i])
            d2 = G.twin_d2(at, "water_velocity", z, log["adcp_cov"], cw)
            worst_d2 = max(worst_d2, abs(d2 / sc["d2"][i, c] - 1.0))
            if G.is_threshold(sc["names"][i][c]):
                got = teeth(at, "water_velocity", z, log["adcp_cov"], cw, ("adcp", i, c))
                least = [min(a, b) for a, b in zip(least, got)]
            assert bool(t.update("water_velocity", z, log["adcp_cov"], extra=cw)) == bool(sc["accept"][i, c]), (i, c)
            worst_e = max(worst_e, twin_err(t, xa[i], Pa[i], dof))
            if not sc["accept"][i, c]:  # a rejected cell: the oracle bitwise unchanged
                np.testing.assert_array_equal(xa[i], xb[i])
                np.testing.assert_array_equal(Pa[i], Pb[i])
            else:
                assert (xa[i] != xb[i]).any()
    print("adcp dof %d B %d %s %s: d2 %.3g, oracle vs twin %.3g, teeth %.3g %.3g"
          % (dof, batch, "pressure" if pressure else "plain", side, worst_d2, worst_e, least[0], least[1]))
    assert worst_d2 < D2_TOL and worst_e < TOL
    # run_log over the rebuilt log: bitwise the per-call loop, the constructed counts
    whole = PS.start(O.OraclePoseBatch(batch, dof), log)
    counts = whole.run_log(log)
    calls = PS.start(O.OraclePoseBatch(batch, dof), log)
    cc = sum(G.oracle_epoch_calls(calls, log, e) for e in range(log["epochs"]))
    np.testing.assert_array_equal(counts, cc)
    np.testing.assert_array_equal(counts[:, 2], sc["counts"])
    assert (counts[:, 0] == 1).all() and (counts[:, 1] == (1 if pressure else 0)).all()
    for a, b in zip(whole.get_state(), calls.get_state()):
        np.testing.assert_array_equal(a, b)
    # an instance with all four cells rejected: the log without its ADCP flag, bitwise
    if batch > 4:
        bare = PS.start(O.OraclePoseBatch(batch, dof), log)
        bare.run_log(G.without_adcp(log))
        for a, b in zip(whole.get_state(), bare.get_state()):
            np.testing.assert_array_equal(a[4], b[4])
            assert (a[3] != b[3]).any()
    fine = G.adcp_scene(batch, dof, pressure, delta=1e-9)
    print("   DELTA 1e-9: oracle as constructed %s" % (fine["oracle_accept"] == fine["accept"]).all())


@pytest.mark.parametrize("dof", DOFS)
def test_adcp_rows_are_per_instance(dof):
    """swapping one instance's targets (all-reject <-> all-accept) leaves the others' rows as they are"""
    base = G.adcp_scene(6, dof)
    pat = list(G.ADCP_PATTERNS)
    pat[4], pat[3] = G.ALL_ACCEPT, G.ALL_REJECT
    swapped = G.adcp_scene(6, dof, patterns=tuple(pat))
    np.testing.assert_array_equal(swapped["counts"], [1, 3, 2, 0, 4, 2])
    np.testing.assert_array_equal(swapped["oracle_accept"], swapped["accept"])
    keep = [0, 1, 2, 5]
    np.testing.assert_array_equal(swapped["log"]["adcp"][:, :, keep], base["log"]["adcp"][:, :, keep])
    assert (swapped["log"]["adcp"][:, :, [3, 4]] != base["log"]["adcp"][:, :, [3, 4]]).any()
    for k in ("gyro", "acc", "dvl", "pos0", "rot0"):
        np.testing.assert_array_equal(swapped["log"][k], base["log"][k])


# ---- GEO fixes ---------------------------------------------------------------------------------
def test_geo_patterns():
    counts = [sum(G.targets()[n][1] for n in p) for p in G.GEO_PATTERNS]
    assert counts == [2, 1, 3, 0, 2, 1] and sorted(set(counts)) == [0, 1, 2, 3]
    for u in range(3):
        assert counts[2 * u] != counts[2 * u + 1]
    plan = dict(G.GEO_PLAN)
    assert plan[2] == G.XY | G.Z | G.GEO and plan[6] == G.GEO and plan[G.GEO_EPOCHS - 1] == G.GEO
    assert G.GEO_EPOCHS <= 12


@pytest.mark.parametrize("batch", [6, 5])
@pytest.mark.parametrize("dof", DOFS)
def test_geo_scene(dof, batch, side):
    sc = G.geo_scene(batch, dof)
    log, fx = sc["log"], sc["fixes"]
    r = fx["geo_cov"][0, 1] / np.sqrt(fx["geo_cov"][0, 0] * fx["geo_cov"][1, 1])
    assert 0.39 < r < 0.51 and np.abs(fx["gps_in_body"][:2]).min() > 0.1
    np.testing.assert_array_equal(sc["oracle_accept"], sc["accept"])
    np.testing.assert_array_equal(sc["counts"], [2, 1, 3, 0, 2, 1][:batch])
    worst_d2 = worst_e = 0.0
    least = [np.inf, np.inf]
    for row in range(3):
        xb, Pb = sc["states"][row]
        after = None
        if row == 2:  # the last epoch: states[3] is the state right after the row
            after = sc["states"][3]
        for i in range(batch):
            t = G.shell(log, i, dof, xb[i], Pb[i])
            z = fx["geo"][row, i]
            d2 = G.twin_d2(t, "geographic", z, fx["geo_cov"], fx["gps_in_body"])
            worst_d2 = max(worst_d2, abs(d2 / sc["d2"][i, row] - 1.0))
            if G.is_threshold(sc["names"][i][row]):
                got = teeth(t, "geographic", z, fx["geo_cov"], fx["gps_in_body"], ("geo", i, row))
                least = [min(a, b) for a, b in zip(least, got)]
            acc = t.update("geographic", z, fx["geo_cov"], extra=fx["gps_in_body"])
            assert bool(acc) == bool(sc["accept"][i, row]), (i, row)
            if after is not None:
                worst_e = max(worst_e, twin_err(t, after[0][i], after[1][i], dof))
                if not acc:
                    np.testing.assert_array_equal(after[0][i], xb[i])
                    np.testing.assert_array_equal(after[1][i], Pb[i])
    print("geo dof %d B %d %s: d2 %.3g, oracle vs twin %.3g, teeth %.3g %.3g"
          % (dof, batch, side, worst_d2, worst_e, least[0], least[1]))
    assert worst_d2 < D2_TOL and worst_e < TOL
    # run_log on the segments with the fixes at the cuts: bitwise the per-call loop
    x, P, acc, facc = G.oracle_run_fixes(log, fx, dof)
    np.testing.assert_array_equal(x, sc["states"][3][0])
    np.testing.assert_array_equal(P, sc["states"][3][1])
    np.testing.assert_array_equal(facc[:, 2], sc["counts"])
    np.testing.assert_array_equal(facc[:, :2], [[1, 1]] * batch)
    fine = G.geo_scene(batch, dof, delta=1e-9)
    print("   DELTA 1e-9: oracle as constructed %s" % (fine["oracle_accept"] == fine["accept"]).all())


def test_delta_is_derived():
    """DELTA is 1000 times a few 1e-9 (the single-call tolerance in d2), and
    far below the least tooth"""
    assert G.DELTA == 1e-6 and G.K == 5.991 and G.DELTA * 1e3 < TOOTH
    tg = G.targets()
    assert tg["K-"] == (5.991 * (1 - 1e-6), 1) and tg["K+"] == (5.991 * (1 + 1e-6), 0)
    assert tg["in"] == (0.5, 1) and tg["out"] == (60.0, 0)
