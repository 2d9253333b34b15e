"""The pair epoch kernel's work-unit boundary (csrc/uwvk_psp_pair.hip, r09).

A wave computes its launch-wide lane constants once, and it issues the next
unit's loads (state, stored rotation rate, per-instance offsets, first inputs)
in the current unit's epilogue, ahead of the fold and the scattered stores.
What can go wrong is a value kept from the previous unit, a prefetch for a
unit that must not be prefetched (a chunk unit, a failing ticket), or a
prefetched value written to LDS before the current unit's stores have read it.

Every handle here starts through init_from_state with each instance's 27
parameter means, density and orientation distinct, so that host::pose_offsets
gives every instance its own `off` row: a per-instance constant wrongly held
across units cannot pass.  Batches are the smallest that put a second / third
unit on a block of an MI355X (3,072 resident blocks at most)."""
import numpy as np
import pytest

from test_gpu_pair_units import NAMES, ST_NAN, _check_pair_against_single

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from uwvk import engine
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")
    return engine


_STARTS = {}


def _start(eng, B, E, dof):
    """(log, x, P) of a C3 log with every instance's start distinct; made once
    per shape, shared and left unchanged."""
    key = (B, E, dof)
    if key not in _STARTS:
        from uwvk import synth
        cfg, uwv = synth.default_pose_config(), synth.default_uwv()
        log = synth.make_pose_log(B, E, "C3", dof=dof)
        g = eng.PoseUKFBatch(B, dof)
        g.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
        x, P = g.get_state()
        i = np.arange(B, dtype=np.float64)
        if dof == 53:  # inertia, linear and quadratic damping (storage 20..46): distinct per instance and entry
            x[:, 20:47] += 1e-3 * (1.0 + i[:, None] / B + np.arange(27)[None, :] / 64.0)
        x[:, -1] *= 1.0 + 1e-3 * (i + 1.0) / B  # water density, the last storage component
        q = x[:, 3:7]
        assert len(np.unique(np.round(q, 12), axis=0)) == B  # make_pose_log's per-instance orientation draw
        assert len(np.unique(x[:, -1])) == B and (dof == 26 or len(np.unique(x[:, 20])) == B)
        _STARTS[key] = (log, x, P)
    return _STARTS[key]


def _run(eng, start, pair, dof=53, slots=-1, chunks=0, pieces=None, log=None, tau=None):
    """tau: every Markov time constant of the configuration (default: the
    synthetic configuration's 600 .. 3,600 s)."""
    from uwvk import abi, synth
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    if tau is not None:
        m, w = cfg.model_noise_parameters, cfg.water_velocity
        cfg.acceleration.bias_tau = cfg.rotation_rate.bias_tau = tau
        m.inertia_tau = m.lin_damping_tau = m.quad_damping_tau = tau
        w.tau = w.adcp_bias_tau = cfg.hydrostatics.water_density_tau = tau
    log0, x, P = start
    log = log or log0
    B = len(x)
    g = eng.PoseUKFBatch(B, dof)
    g.set_pair(pair)
    g.set_tail_slots(slots)
    if chunks:
        g.set_tail_chunks(chunks)
    loc = abi.Location(cfg.location.latitude, cfg.location.longitude, cfg.location.altitude)
    g.init_from_state(x, P, loc, uwv, synth.pose_parameter(cfg))
    g.set_process_noise_from_config(cfg, 1e-3)
    assert g.pair_active() == (1 if pair else 0)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    dlog = g.upload_log(log)
    for a, n in pieces or [(0, log["gyro"].shape[0])]:
        g.run_log(dlog, a, n, accept_counts=acc)
    xo, Po = g.get_state()
    return xo, Po, acc.read(np.uint32, (B, 4)), g.get_status(), g.get_rotation_rate()


_CLEAN = {}


def _clean_6400(eng):
    """The pair kernel's run of the 6,400 x 4 log in one launch (shared)."""
    if "r" not in _CLEAN:
        _CLEAN["r"] = _run(eng, _start(eng, 6400, 4, 53), True)
    return _CLEAN["r"]


@pytest.mark.parametrize("dof,B", [(53, 12800), (26, 6400)])
def test_third_unit_per_block(eng, dof, B):
    """53 DOF: 6,400 pair units on at most 3,072 blocks, so blocks take a
    second and a third unit, each prefetched in the previous unit's epilogue.
    26 DOF (PD = 0): 3,200 units, a second unit per block."""
    st = _start(eng, B, 3, dof)
    _check_pair_against_single(_run(eng, st, True, dof), _run(eng, st, False, dof), dof)


@pytest.mark.parametrize("tau", [2e-3, float("inf")])
def test_two_launches_equal_one(eng, tau):
    """Epochs [0, 2) then [2, 4) on one handle (the second launch's tickets
    start from a non-zero ticket_base) are bitwise one launch of [0, 4).

    Every launch ends with psp_fold, which multiplies the time scale d into
    Sigma~ (Sigma = D Sigma~ D), so a split run folds twice where one launch
    folds once: the two can be bitwise equal only where that product is exact.
    With the synthetic configuration's time constants (600 .. 3,600 s) it is
    rounded, and the split run differs from the whole one in the last bits, on
    this kernel and identically on the kernel before the boundary change
    (MI355X: 34,648 of 345,600 mean entries, max |diff| 4.4e-20; 992,084 of
    17,977,600 covariance entries, max 1.7e-18; counts, status and rotation
    rate equal).  So the comparison runs where the fold is exact:
    tau = 2 ms: A = 1 + dt (-1 / tau) = 0.5 exactly at dt = 1 ms, d a power of
      two, every product with it exact; each mean moves half-way to its
      instance's offset per epoch, so an offset row kept from the previous
      unit changes the result;
    tau = inf: A = 1, d = 1.
    test_two_launches_match_single keeps the default time constants."""
    assert 1.0 + 1e-3 * (-1.0 / tau) in (0.5, 1.0)
    st = _start(eng, 6400, 4, 53)
    ref = _run(eng, st, True, tau=tau)
    got = _run(eng, st, True, pieces=[(0, 2), (2, 2)], tau=tau)
    for name, a, b in zip(NAMES, got, ref):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        print("two launches vs one, %s: %d of %d entries differ, max |diff| %.3g" % (name, (a != b).sum(), a.size, d.max()))
    for name, a, b in zip(NAMES, got, ref):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert not got[3].any()
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # the configuration reached the kernel: not the default configuration's result
    assert not np.array_equal(got[0], _clean_6400(eng)[0])


def test_two_launches_match_single(eng):
    """The same two launches against the one-instance kernel run in the same
    two pieces (each launch ends with its own fold of the time scale, on both
    kernels): the pair bound, so a unit of the second launch that read the
    wrong ticket, instance or offset row fails."""
    st = _start(eng, 6400, 4, 53)
    pieces = [(0, 2), (2, 2)]
    _check_pair_against_single(_run(eng, st, True, pieces=pieces), _run(eng, st, False, pieces=pieces), 53)


@pytest.mark.parametrize("dof", [53, 26])
def test_chunk_units_keep_their_order(eng, dof):
    """Batch 64, one tail slot per XCD, two chunks per tail unit: a chunk unit
    is loaded after tail_wait's acquire, never prefetched.  Bitwise the
    unchunked run, no status bit."""
    st = _start(eng, 64, 3, dof)
    ref = _run(eng, st, True, dof, slots=1)
    got = _run(eng, st, True, dof, slots=1, chunks=2)
    for name, a, b in zip(NAMES, got, ref):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert not got[3].any()


def test_last_unit_and_odd_ends(eng):
    """Batch 6,146 = 3,073 units: with 3,072 blocks exactly one takes a second
    unit and every other block's ticket fails at once (no load past the batch)."""
    st = _start(eng, 6146, 3, 53)
    got = _run(eng, st, True)
    _check_pair_against_single(got, _run(eng, st, False), 53)
    assert not got[3].any()


def test_nan_across_a_boundary(eng):
    """A NaN gyro sample at the last epoch of instance 0 (instance 1, the other
    half of its wave, finite): instance 0 carries UWVK_ST_NAN and keeps the
    rotation rate stored at the epoch before; every other instance, the pair
    its block takes next included, is bitwise the clean run.  The rotation
    rate read back is stored rate - gyro bias - earth rate in the body frame:
    against the one-instance kernel on the same log it may differ by the pair
    tolerance on the bias and orientation (1e-9 sigma, sigma < 0.1 rad/s), so
    1e-10 rad/s; the skipped sample itself is ~1e-4 rad/s away."""
    st = _start(eng, 6400, 4, 53)
    log = st[0]
    E = log["gyro"].shape[0]
    bad = dict(log)
    bad["gyro"] = log["gyro"].copy()
    bad["gyro"][E - 1, 0, 1] = np.nan
    ref = _clean_6400(eng)
    got = _run(eng, st, True, log=bad)
    one = _run(eng, st, False, log=bad)
    assert not ref[3].any()
    assert got[3][0] == ST_NAN and not got[3][1:].any()
    assert one[3][0] == ST_NAN
    for name, a, b in zip(NAMES, got, ref):
        np.testing.assert_array_equal(a[1:], b[1:], err_msg=name)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[4]).all()
    d_one, d_clean = np.abs(got[4][0] - one[4][0]).max(), np.abs(got[4][0] - ref[4][0]).max()
    print("rotation rate of instance 0: vs single %.3g, vs the clean run %.3g rad/s" % (d_one, d_clean))
    assert d_one < 1e-10
    assert d_clean > 1e-7  # the NaN sample was not stored
