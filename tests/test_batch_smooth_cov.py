"""Batch smoothed covariances on the device: every member's covariance pass against the longdouble rule of
``smooth_cov_util`` under its bound, the bit rules (the state half is ``smooth_history``'s, symmetry, repeatability, the
members untouched, independence of the batch around a member), consistency with the filtered covariance, failures, dirty
buffers, refusals and ``smooth_replicas(cov=True)``.  Scenes, the oracle with a member's own noise and the shared device runs:
``batch_smooth_cov_util.py`` (``test_batch_smooth_cov_cpu.py`` checks the oracle's margin without a GPU)."""
import numpy as np
import pytest

import batch_smooth_cov_util as bcu
import batch_smooth_util as bu
import smooth_cov_util as scu
import smooth_util as su
import support as sp

pytestmark = pytest.mark.gpu
EKF_ERR_INVALID, EKF_ERR_STATE, EKF_ERR_NUMERIC = -1, -4, -5


def _check_bit_rules(case, members):
    """The bit rules of one ``run_batch``; returns nothing."""
    batch = case["batch"]
    smoothed, cam, filt, first = case["cov0"]
    for b in range(members):
        records = case["records"][b]
        frames = smoothed[b].shape[0]
        # the state half: smooth_history on the same history, before and after the covariance pass
        assert np.array_equal(smoothed[b], case["state0"][b]) and np.array_equal(case["state1"][b], case["state0"][b]), b
        # two passes give the same bits
        for u, v in zip(case["cov0"], case["cov1"]):
            assert sp.same(u[b], v[b], equal_nan=True), b
        # filt_cam_cov is the record's camera block; rows before the first record are NaN; the last record's rows are filtered
        rec_of = np.full(frames, -1)
        for r, rec in enumerate(records):
            rec_of[rec["frame"]:] = r
        for t in range(frames):
            if rec_of[t] < 0:
                assert np.isnan(cam[b][t]).all() and np.isnan(filt[b][t]).all(), (b, t)
                assert np.array_equal(smoothed[b][t], case["poses"][b][:7]), (b, t)
            else:
                assert np.array_equal(filt[b][t], records[rec_of[t]]["P"][:10, :10]), (b, t)
        last = records[-1]["frame"]
        assert np.array_equal(cam[b][last:], filt[b][last:])
        # bitwise symmetric
        live = rec_of >= 0
        assert np.array_equal(cam[b][live], cam[b][live].transpose(0, 2, 1)) and np.array_equal(first[b], first[b].T), b
        assert first[b].shape == (records[0]["dims"],) * 2 and np.array_equal(first[b][:10, :10], cam[b][records[0]["frame"]])
    # members, status() and P are untouched
    assert sp.same(case["before"], case["after"]) and case["status"][0] == case["status"][1] == [0] * members
    assert case["smooth_status"].tolist() == [0] * members and batch.last_smooth_status.tolist() == [0] * members


def _check_oracle(case, members, noise_rows, label, only=None):
    """worst error / bound <= 1 for cam_cov over every frame and first_cov over all entries; the consistency with the
    filtered block on the device's own records.  Returns the worst ratios."""
    _smoothed, cam, filt, first = case["cov0"]
    worst = [0.0, 0.0]
    for b in range(members) if only is None else [only]:
        records = case["records"][b]
        frames = cam[b].shape[0]
        ref = bcu.member_cov_oracle(records, noise_rows[b])
        r_cam, r_first = bcu.worst_ratios(cam[b], first[b], ref, records, frames)
        print(f"{label} member {b}: {len(records)} records, N <= {max(r['dims'] for r in records)}, kappa <= "
              f"{ref['kappa'].max() if len(records) > 1 else 0:.0f}, worst error / bound: cam_cov {r_cam:.4f}, first_cov {r_first:.4f}")
        assert r_cam <= 1.0 and r_first <= 1.0, (label, b, r_cam, r_first)
        worst = [max(worst[0], r_cam), max(worst[1], r_first)]
        # consistency: filt - smoothed is positive semidefinite, position variances do not grow, within N_r bound_r
        bound = scu.record_bound(ref, records)
        for r, rec in enumerate(records):
            t = rec["frame"]
            slack = rec["dims"] * bound[r]
            gap = filt[b][t] - cam[b][t]
            assert np.linalg.eigvalsh(gap).min() >= -slack, (label, b, r)
            assert (np.diag(gap)[:3] >= -slack).all(), (label, b, r)
    return worst


# ---- 1. the scenes ----------------------------------------------------------------------------------------------------------
# (the longdouble rule at N = 160 takes seconds per member: the growing scene has one case per member, on one device run)
SCENE_CASES = [(name, None) for name in bcu.GPU_SCENES if name != "growing"] + [("growing", b) for b in range(3)]


@pytest.mark.parametrize("name,only", SCENE_CASES)
def test_scene_against_the_oracle_under_the_bound_and_the_bit_rules(name, only):
    case = bcu.device_case(name)
    batch = case["batch"]
    assert sorted({r["dims"] for r in case["records"][0]}) == bcu.EXPECTED_DIMS[name]
    if not only:
        _check_bit_rules(case, 3)
    _check_oracle(case, 3, batch.noise, name, only)
    if name == scu.GROWING:      # record 0 is smoothed: returning P_r cannot pass
        for b in range(3):
            rec = case["records"][b][0]
            p0, s0 = rec["P"][:10, :10], case["cov0"][1][b][rec["frame"]]
            assert np.abs(s0 - p0).max() >= 0.05 * np.abs(p0).max(), b


# ---- 2. the mixed batch, and independence of the batch around a member ---------------------------------------------------------
def test_mixed_batch_against_the_oracle_under_the_bound_and_the_bit_rules():
    case = bcu.mixed_case()
    assert [max(r["dims"] for r in recs) for recs in case["records"]] == [40, 34, 160, 34]
    _check_bit_rules(case, 4)
    _check_oracle(case, 4, case["batch"].noise, "mixed")


def test_a_member_does_not_depend_on_the_batch_around_it():
    case = bcu.mixed_case()
    logs = case["logs"]
    other = bcu.run_batch(logs, order=[2, 3, 0, 1], noise=bu.MIXED_NOISE, motion=True, frame_scale=True)
    for slot, i in enumerate(other["order"]):
        for u, v in zip(other["cov0"], case["cov0"]):
            assert sp.same(u[slot], v[i], equal_nan=True), i
    for i in range(4):
        alone = bcu.run_batch(logs, order=[i], noise=bu.MIXED_NOISE, motion=True, frame_scale=True)
        for u, v in zip(alone["cov0"], case["cov0"]):
            assert sp.same(u[0], v[i], equal_nan=True), i


def test_more_members_than_compute_units_all_have_member_zeros_bits():
    log = bu.scene_log("tracking")
    batch = bu.new_batch(300, poses=bu.INIT, max_landmarks=10)
    out = batch.smooth_detection_logs([log] * 300, cov=True)
    first = batch.smooth_history_cov(first=True)[3]
    assert batch.last_smooth_status.tolist() == [0] * 300
    for part in (*out, first):
        stack = np.stack(part)
        assert sp.same(stack, np.broadcast_to(stack[0], stack.shape), equal_nan=True)
    assert not np.isnan(out[3][0]).any() and first[0].shape == (40, 40)
    # and they are the bits of the same member in a batch of three copies
    three = bu.new_batch(3, poses=bu.INIT, max_landmarks=10)
    small = three.smooth_detection_logs([log] * 3, cov=True)
    for u, v in zip(out, small):
        assert sp.same(u[0], v[0], equal_nan=True)


# ---- 3. failures --------------------------------------------------------------------------------------------------------------
def test_a_bad_pivot_stays_with_its_member():
    case = bcu.device_case("tracking")
    batch = case["batch"]
    restore = bu.tamper_member(batch, 1, 20, 39)
    try:
        got = batch.smooth_history_cov(first=True)
        assert batch.last_smooth_status.tolist() == [0, EKF_ERR_NUMERIC, 0]
        for k, part in enumerate(got):
            assert np.isnan(part[1]).all() and part[1].size > 0
            for b in (0, 2):
                assert sp.same(part[b], case["cov0"][k][b], equal_nan=True)
        assert got[3][1].shape == (40, 40)
    finally:
        restore()
    again = batch.smooth_history_cov(first=True)
    assert batch.last_smooth_status.tolist() == [0, 0, 0]
    for u, v in zip(again, case["cov0"]):
        for b in range(3):
            assert sp.same(u[b], v[b], equal_nan=True)
    assert sp.same(case["before"], sp.snap_batch(batch, tables=True)) and batch.status() == [0, 0, 0]


def test_a_member_that_failed_in_the_replay_is_nan_from_its_failing_frame_on():
    """The fixture of ``test_batch_smooth.py::test_a_failed_member_stays_alone``: member 1 fails at its first frame."""
    log = bu.scene_log("tracking")
    head, rest = bu.prefix(log, 3), bu.suffix(log, 3)
    out = []
    for bad in (False, True):
        batch = bu.new_batch(3, noise={"q_cam": [0.3, 0.1, 0.5]})
        batch.process_detection_logs([head] * 3)
        if bad:
            ids = [k for k, _ in sorted(batch.landmarks[1].items(), key=lambda kv: kv[1])]
            s0 = batch.get_state(1)
            batch.set_member(1, s0, -np.eye(s0.shape[0]), ids)      # S = H (Q - I) H^T + R I cannot be positive definite
        batch.process_detection_logs([rest, rest if bad else None, rest], record=True)
        out.append((batch.smooth_history_cov(first=True), batch))
    (good, _b), (got, batch) = out
    assert batch.status() == [0, EKF_ERR_NUMERIC, 0] and batch.last_smooth_status.tolist() == [0, 0, 0]
    for part in got[:3]:
        assert part[1].shape[0] == 37 and np.isnan(part[1]).all()
    assert got[3][1].shape == (0, 0)      # (no record: nothing of its first_cov slab is written)
    for part, want in zip(got, good):
        for b in (0, 2):
            assert sp.same(part[b], want[b], equal_nan=True) and not np.isnan(part[b][-1]).any()


# ---- 4. dirty buffers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", scu.GROWING])
def test_dirty_workspace_and_outputs_give_the_same_bits(name):
    case = bcu.device_case(name)
    batch, mf = case["batch"], case["batch"]._history_frames
    rc, out, status = bcu.direct_batch_smooth_cov(batch, poison=True)
    assert rc == 0 and status.tolist() == [0, 0, 0]
    smoothed, cam, filt, first = case["cov0"]
    for b in range(3):
        rows = slice(int(mf[b]), int(mf[b + 1]))
        for key, want in (("smoothed", smoothed), ("cam_cov", cam), ("filt_cam_cov", filt)):
            assert sp.same(out[key][rows], want[b], equal_nan=True), (b, key)
        n0 = first[b].shape[0]
        assert np.array_equal(out["first_cov"][b, :n0, :n0], first[b])
        # what the rules do not write keeps the sentinel: the slab beyond [0:N_0, 0:N_0]
        rest = out["first_cov"][b].copy()
        rest[:n0, :n0] = su.SENTINEL
        assert (rest == su.SENTINEL).all()
    for key in ("smoothed", "cam_cov", "filt_cam_cov"):
        assert not (out[key] == su.SENTINEL).any(), key


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_enqueued():
    import ctypes as C
    from aruco_slam_amd.hip_backend import EkfError
    log = bu.scene_log("ragged", with_motion=False, with_scale=False)
    batch = bu.new_batch(2)
    batch.smooth_detection_logs([bu.prefix(log, 9), bu.prefix(log, 9)])
    before = sp.snap_batch(batch, tables=True)
    need = C.c_size_t()
    assert batch.lib.ekf_batch_smooth_cov_workspace_bytes(batch.h, C.byref(need)) == 0
    n0 = batch.history_records(0)[0]["dims"]
    for kw in ({"ws_bytes": need.value - 256}, {"first_ld": n0 - 1}, {"flags": 1}):
        rc, out, status = bcu.direct_batch_smooth_cov(batch, **kw)
        assert rc == EKF_ERR_INVALID, kw
        assert all((v == su.SENTINEL).all() for v in out.values()) and status.tolist() == [99, 99], kw
    rc, out, _st = bcu.direct_batch_smooth_cov(batch, handle=False)
    assert rc == -1 and all((v == su.SENTINEL).all() for v in out.values())
    rc, out, status = bcu.direct_batch_smooth_cov(batch)
    assert rc == 0 and status.tolist() == [0, 0] and not (out["cam_cov"] == su.SENTINEL).any()
    # a stale history after reset
    batch.reset(0)
    with pytest.raises(EkfError) as err:
        batch.smooth_history_cov()
    assert err.value.code == EKF_ERR_STATE
    assert sp.same(before[1:], sp.snap_batch(batch, tables=True)[1:])


@pytest.mark.parametrize("kw", [{"large_maps": True}, {"model": "ekf_rotations", "quat_update": None, "max_landmarks": 10,
                                                       "max_visible": 8}])
def test_a_batch_that_cannot_record_is_refused(kw):
    import ctypes as C
    batch = bu.new_batch(2, **kw)
    n = C.c_size_t()
    assert batch.lib.ekf_batch_smooth_history_cov(batch.h, None, 0, None, 0, 0, None, None, None, None, 0, None) == EKF_ERR_STATE
    assert batch.lib.ekf_batch_smooth_cov_workspace_bytes(batch.h, C.byref(n)) == EKF_ERR_STATE


# ---- 6. replicas --------------------------------------------------------------------------------------------------------------
def test_smooth_replicas_with_cov():
    log = bu.scene_log("tracking")
    kw = {"poses": bu.INIT, "max_landmarks": 10}
    plain, batch, bare = (bu.new_batch(bu.REPLICAS, **kw) for _ in range(3))
    want = plain.replay_replicas(log, bu.REPLICA_SIGMA, bu.REPLICA_SEED).trajectory
    filtered, smoothed, filtered_cov, smoothed_cov = batch.smooth_replicas(log, bu.REPLICA_SIGMA, bu.REPLICA_SEED, cov=True)
    assert filtered.shape == smoothed.shape == (bu.REPLICAS, 40, 7) and np.array_equal(filtered, want)
    assert filtered_cov.shape == smoothed_cov.shape == (bu.REPLICAS, 40, 10, 10)
    assert batch.last_smooth_status.tolist() == [0] * bu.REPLICAS and not np.isnan(smoothed_cov).any()
    assert np.array_equal(smoothed_cov[:, -1], filtered_cov[:, -1]) and not np.array_equal(smoothed_cov[:, 0], filtered_cov[:, 0])
    out = bare.smooth_replicas(log, bu.REPLICA_SIGMA, bu.REPLICA_SEED)      # the cov-less return is what it was
    assert len(out) == 2 and np.array_equal(out[0], filtered) and np.array_equal(out[1], smoothed)
