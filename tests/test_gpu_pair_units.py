"""The pair epoch kernel (csrc/uwvk_psp_pair.hip) across work units and under a
half-masked wave.

* The 26-in-53 index map of the parameter-decoupled state is tabulated once
  per wave in LDS and read by every work unit's load and store: the units a
  wave takes after its first must see the same table.  At a small batch every
  pair unit has a resident block of its own (the persistent grid is
  min(units, resident blocks), uwvk_plan.hpp persist_geometry; the tail-slot
  setting adds chunk units but never takes blocks away), so the batch-64 cases
  cover one unit, or one chunk, per wave; test_pair_blocks_take_several_units
  runs a batch above twice the resident blocks of an MI355X (256 CUs x 12),
  where every block past units - grid takes a second unit.
* One instance of a pair with non-finite measurements while the other stays
  finite: the wave runs its updates with one 32-lane half masked off, and the
  per-half broadcasts (hbc: row_newbcast, then row_bcast:15 into rows 1 and 3)
  must neither read from nor write into the other half."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ST_NAN = 0x2  # UWVK_ST_NAN
NAMES = ("state", "covariance", "accept counts", "status", "rotation rate")


@pytest.fixture(scope="module")
def eng():
    from uwvk import engine
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")
    return engine


def _run(eng, log, pair, dof=53, slots=-1, chunks=0):
    from uwvk import synth
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    B = log["gyro"].shape[1]
    g = eng.PoseUKFBatch(B, dof)
    g.set_pair(pair)
    g.set_tail_slots(slots)
    if chunks:
        g.set_tail_chunks(chunks)
    g.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    g.set_process_noise_from_config(cfg, 1e-3)
    assert g.pair_active() == (1 if pair else 0)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    g.run_log(g.upload_log(log), accept_counts=acc)
    x, P = g.get_state()
    return x, P, acc.read(np.uint32, (B, 4)), g.get_status(), g.get_rotation_rate()


def _check_pair_against_single(got, ref, dof):
    """Every mean and covariance entry of every instance within the pair
    tolerance (1e-9 in sigma units, as test_gpu_pd.test_pair_matches_single),
    the parameter rows' off-diagonal zeros bitwise 0."""
    from helpers import cov_err, state_err
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[3], ref[3])
    assert not got[3].any()
    es, ec = state_err(got[0], ref[0], ref[1], dof), cov_err(got[1], ref[1])
    print("pair vs single: state %.3g, cov %.3g (sigma units)" % (es.max(), ec.max()))
    assert es.shape == (len(ref[0]),) and es.max() < 1e-9
    assert ec.shape == (len(ref[0]),) and ec.max() < 1e-9
    if dof == 53:
        blk = got[1][:, 19:46, :].copy()
        for t in range(27):
            blk[:, t, 19 + t] = 0.0
        assert not blk.any()


@pytest.fixture(scope="module")
def logs():
    """One 3-epoch, batch-64 C3 log per layout, shared and left unchanged."""
    from uwvk import synth
    return {dof: synth.make_pose_log(64, 3, "C3", dof=dof) for dof in (53, 26)}


@pytest.mark.parametrize("dof", [53, 26])
def test_pair_units_match_single(eng, logs, dof):
    """C3, 3 epochs, batch 64, one tail slot per XCD: pair on against pair off
    (dof 26: PD = 0, no index table)."""
    ref = _run(eng, logs[dof], False, dof, slots=1)
    got = _run(eng, logs[dof], True, dof, slots=1)
    _check_pair_against_single(got, ref, dof)


@pytest.mark.parametrize("dof", [53, 26])
def test_pair_units_tail_chunks_bitwise(eng, logs, dof):
    """tail_chunks = 2 (16 of the 32 pair units run as two chunk units each,
    handed on through HBM: 48 units, every one loads and stores through the
    table) is bitwise tail_chunks = 0, and within the pair tolerance of pair off."""
    ref = _run(eng, logs[dof], True, dof, slots=1)
    got = _run(eng, logs[dof], True, dof, slots=1, chunks=2)
    for name, a, b in zip(NAMES, got, ref):
        np.testing.assert_array_equal(a, b, err_msg=name)
    _check_pair_against_single(got, _run(eng, logs[dof], False, dof, slots=1), dof)


def test_pair_blocks_take_several_units(eng):
    """Batch 6,400 = 3,200 pair units on at most 3,072 resident blocks (MI355X):
    the blocks that finish first take a second unit from the ticket counter and
    load / store it through the table their wave filled before its first."""
    from uwvk import synth
    log = synth.make_pose_log(6400, 3, "C3")
    _check_pair_against_single(_run(eng, log, True), _run(eng, log, False), 53)


def test_pair_half_nonfinite(eng):
    """Batch 4, 205 epochs (the DVL epoch 199 inside).  Instance 0: NaN in acc
    at three epochs and in its DVL sample; instances 1-3 finite.  Instance 1
    shares instance 0's wave: its updates at those epochs run with the lower
    half masked off.  Instances 1-3 are bitwise the run without the NaNs;
    instance 0 carries UWVK_ST_NAN and is the one-instance kernel's on the
    same log (1e-9 in sigma units); status 0 for instances 1-3."""
    from helpers import cov_err, state_err
    from uwvk import abi, synth
    B, E = 4, 205
    clean = synth.make_pose_log(B, E, "C3")
    dv = np.flatnonzero((clean["flags"] & abi.EV_DVL) != 0)
    assert list(dv) == [199]
    bad = dict(clean)
    bad["acc"] = clean["acc"].copy()
    bad["dvl"] = clean["dvl"].copy()
    for e, k in ((7, 0), (120, 2), (199, 1)):  # (the last on the DVL epoch itself)
        bad["acc"][e, 0, k] = np.nan
    bad["dvl"][clean["dvl_index"][199], 0, 1] = np.nan
    ref = _run(eng, clean, True)
    got = _run(eng, bad, True)
    one = _run(eng, bad, False)
    assert not ref[3].any()
    for name, a, b in zip(NAMES, got, ref):
        np.testing.assert_array_equal(a[1:], b[1:], err_msg=name)
    assert list(got[3]) == [ST_NAN, 0, 0, 0] and list(one[3]) == [ST_NAN, 0, 0, 0]
    np.testing.assert_array_equal(got[2], one[2])
    assert got[2][0, 0] == 0  # instance 0's DVL sample was skipped: nothing to accept
    es, ec = state_err(got[0], one[0], one[1], 53), cov_err(got[1], one[1])
    print("half-masked pair vs single: state %s, cov %s" % (es, ec))
    assert es[0] < 1e-9 and ec[0] < 1e-9
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # the skipped measurements changed instance 0 (the NaNs reached the kernel)
    assert not np.array_equal(got[0][0], ref[0][0])
