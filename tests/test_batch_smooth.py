"""Batch smoothing on the device: the recorded call against the plain one (bit for bit), the records against the filter and
the plan, every member's backward pass against the longdouble oracle of ``smooth_util`` under its bound, independence of the
batch around a member, a failed member, the refusals, and ``smooth_replicas``.  Logs, sizes and the oracle with a member's
own noise: ``batch_smooth_util.py`` (``test_batch_smooth_cpu.py`` checks them without a GPU)."""
import numpy as np
import pytest

import batch_smooth_util as bu
import motion_util as mu
import smooth_util as su
import support as sp

pytestmark = pytest.mark.gpu
EKF_ERR_CAPACITY, EKF_ERR_STATE, EKF_ERR_NUMERIC = -2, -4, -5


def _batch(members, **kw):
    from aruco_slam_amd.batch import EKFBatch
    kw.setdefault("quat_update", "scalar_first")
    kw.setdefault("max_landmarks", 50)
    kw.setdefault("max_visible", 16)
    poses = kw.pop("poses", None)
    return EKFBatch(members, bu.initial_poses(members) if poses is None else poses, **kw)


# ---- 1. recorded = plain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["motion", "scale", "gate"])
def test_recorded_call_is_the_plain_call_bit_for_bit(case):
    logs = [bu.scene_log("ragged", seed=5, with_scale=case == "scale"), None,
            bu.scene_log("ragged", seed=6, with_scale=case == "scale"), bu.scene_log("ragged", seed=7, with_scale=case == "scale")]
    kw = {"motion": True, "frame_scale": case == "scale", "gate": 1e-3 if case == "gate" else None,
          "noise": {"q_cam": [0.3, 0.3, 0.1, 0.5], "q_lm": [0.01, 0.01, 0.02, 0.005]}}
    out = []
    for record in (False, True):
        batch = _batch(4, **kw)
        rep = batch.process_detection_logs(logs, nis=True, cam_cov=True, mahal=case == "gate", record=record)
        out.append((rep, sp.snap_batch(batch, tables=True), list(batch.num_landmarks), batch.pending_scale, batch.status()))
        assert (batch.last_history is not None) == record
    (plain, snap0, n0, pend0, st0), (rec, snap1, n1, pend1, st1) = out
    for b in range(4):
        assert sp.same(plain.trajectory[b], rec.trajectory[b], equal_nan=True)
        assert sp.same(plain.nis[b], rec.nis[b], equal_nan=True)
        assert sp.same(plain.cam_cov[b], rec.cam_cov[b], equal_nan=True) and np.array_equal(plain.dof[b], rec.dof[b])
        if case == "gate":
            assert sp.same(plain.mahal[b], rec.mahal[b], equal_nan=True) and np.array_equal(plain.rejected[b], rec.rejected[b])
    assert sp.same(snap0, snap1) and n0 == n1 and np.array_equal(pend0, pend1) and st0 == st1 == [0] * 4
    assert rec.trajectory[1].shape == (0, 7)
    if case == "gate":      # the gate leaves frames without a detection: they are not stepped
        assert sum(int(r.sum()) for r in rec.rejected) > 0
        unstepped = [int((rec.dof[b] == 0).sum()) for b in (0, 2, 3)]
        print("frames that were not stepped:", unstepped)
        assert max(unstepped) > 5      # (5 frames of every log are empty anyway: some member's frames lost all they had)


# ---- 2. records are the filter, the table is the plan ----------------------------------------------------------------------
def test_records_are_the_filter_and_the_table_is_the_plan():
    import ctypes as C
    from aruco_slam_amd.batch import _iptr, _lptr
    log = bu.scene_log("ragged")
    kw = {"motion": True, "frame_scale": True, "noise": {"q_cam": [0.3, 0.1, 0.5]}}
    batch = _batch(3, **kw)
    batch.process_detection_logs([log] * 3, record=True)
    records = [batch.history_records(b) for b in range(3)]
    for b in range(3):
        assert [(r["frame"], r["dims"], r["stepped"], r["s_eff"]) for r in records[b]] == su.RAGGED_TABLE
        for r in records[b]:      # moved-only records carry the motion, records of the still frames none
            assert np.array_equal(r["u"], log["motion"][r["frame"]])
        assert not records[b][2]["u"].any() and not records[b][9]["u"].any()
    for r in (0, 6, 13):
        twin = _batch(3, **kw)
        twin.process_detection_logs([bu.prefix(log, records[0][r]["frame"] + 1)] * 3)
        for b in range(3):
            assert np.array_equal(records[b][r]["x"], twin.get_state(b)) and np.array_equal(records[b][r]["P"], twin.get_cov(b)), (r, b)
    # ekf_batch_history_bytes by hand: member 0 has 3 frames that add 2, 0 and 1 markers, member 1 one frame that adds 1
    fresh = _batch(2)
    idx, fo, mf = np.array([0, 1, 0, 1, 2, 0], np.int32), np.array([0, 2, 3, 5, 6], np.int64), np.array([0, 3, 4], np.int64)
    n = C.c_size_t()
    for with_motion, want in ((0, 4608 + 1280 + 1024), (1, 4608 + 1280 + 1280)):
        fresh._check(fresh.lib.ekf_batch_history_bytes(fresh.h, _iptr(idx), _lptr(fo), _lptr(mf), with_motion, C.byref(n)))
        assert n.value == want == bu.history_bytes([[(16, True), (16, True), (19, True)], [(13, True)]], bool(with_motion))
    fo = np.array([0, 2, 2, 5, 6], np.int64)      # member 0's middle frame is empty: a slot only in a call with motions
    idx = np.array([0, 1, 0, 1, 2, 0], np.int32)
    for with_motion in (0, 1):
        fresh._check(fresh.lib.ekf_batch_history_bytes(fresh.h, _iptr(idx), _lptr(fo), _lptr(mf), with_motion, C.byref(n)))
        assert n.value == bu.history_bytes([[(16, True), (16, False), (19, True)], [(13, True)]], bool(with_motion))


# ---- 3. / 4. against the oracle, and independence ---------------------------------------------------------------------------
MIXED_NOISE = {"q_cam": [0.3, 0.1, 0.3, 0.5], "q_lm": [0.01, 0.02, 0.01, 0.005]}


def _mixed_logs():
    return [bu.scene_log("tracking", with_motion=True, with_scale=True), bu.scene_log("ragged"),
            bu.scene_log("growing", with_motion=True, with_scale=True), bu.scene_log("ragged", seed=6)]


def _run(logs, order=None, **kw):
    """A batch over ``logs`` (in ``order``: members permuted, with their poses and noise); returns per ORIGINAL member
    (filtered, smoothed, records, start, noise row) and the batch."""
    members = len(logs)
    order = list(range(members)) if order is None else list(order)
    poses = bu.initial_poses(members)[order]
    noise = {k: np.asarray(v, dtype=np.float64)[order] for k, v in kw.pop("noise", {}).items()}
    gate = kw.pop("gate", None)
    batch = _batch(len(order), poses=poses, noise=noise, gate=None if gate is None else np.asarray(gate)[order], **kw)
    out = batch.smooth_detection_logs([logs[i] for i in order])
    filtered, smoothed = out[0], out[1]
    result = {}
    for slot, i in enumerate(order):
        result[i] = (filtered[slot], smoothed[slot], batch.history_records(slot), poses[slot], batch.noise[slot])
    return result, batch


def _check_members(result, logs):
    worst = 0.0
    for i, (filtered, smoothed, records, start, noise) in sorted(result.items()):
        frames = len(logs[i]["offsets"]) - 1
        ref = bu.member_oracle(records, frames, start, noise)
        ratio = su.worst_ratio(smoothed, ref, records)
        print(f"member {i}: {len(records)} records, N <= {max(r['dims'] for r in records)}, worst error / bound = {ratio:.4f}")
        assert ratio <= 1.0, i
        last, first = records[-1]["frame"], records[0]["frame"]
        assert np.array_equal(smoothed[last:], filtered[last:])                        # from the last record on: the filtered rows
        assert np.array_equal(smoothed[:first], np.tile(start[:7], (first, 1)))        # before the first record: the start camera
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", ["tracking", "ragged", "growing"])
def test_backward_pass_against_the_oracle_under_the_bound(name):
    """Three members over the scene that differ in initial pose, q_cam / q_lm and gate (member 2 gates at the 99.9 % point)."""
    logs = [bu.scene_log(name)] * 3
    kw = {"motion": name == "ragged", "frame_scale": name == "ragged"}
    result, batch = _run(logs, noise={"q_cam": [0.3, 0.1, 0.5], "q_lm": [0.01, 0.02, 0.005]}, gate=[np.inf, np.inf, 16.266], **kw)
    assert batch.status() == [0] * 3 and batch.last_smooth_status.tolist() == [0] * 3
    _check_members(result, logs)
    if name == "growing":
        assert max(r["dims"] for r in result[0][2]) == 160 == su.RESIDENT_DIMS


@pytest.fixture(scope="module")
def mixed():
    logs = _mixed_logs()
    result, batch = _run(logs, noise=MIXED_NOISE, motion=True, frame_scale=True)
    return logs, result, batch


def test_mixed_batch_against_the_oracle_under_the_bound(mixed):
    """All three scenes in one call: the dynamic LDS of every workgroup is sized by the growing member's N = 160."""
    logs, result, batch = mixed
    assert batch.last_smooth_status.tolist() == [0] * 4
    assert [max(r["dims"] for r in result[i][2]) for i in range(4)] == [40, 34, 160, 34]
    _check_members(result, logs)


def test_a_member_does_not_depend_on_the_batch_around_it(mixed):
    logs, result, batch = mixed
    # the pass is read-only and repeatable
    before, status = sp.snap_batch(batch, tables=True), batch.status()
    again = batch.smooth_history()
    assert sp.same(before, sp.snap_batch(batch, tables=True)) and batch.status() == status
    for i in range(4):
        assert np.array_equal(again[i], result[i][1])
    # another order of the members, and every member alone
    other, _b = _run(logs, order=[2, 3, 0, 1], noise=MIXED_NOISE, motion=True, frame_scale=True)
    for i in range(4):
        assert np.array_equal(other[i][0], result[i][0]) and np.array_equal(other[i][1], result[i][1]), i
    for i in (1, 2):
        alone, _b = _run(logs, order=[i], noise=MIXED_NOISE, motion=True, frame_scale=True)
        assert np.array_equal(alone[i][0], result[i][0]) and np.array_equal(alone[i][1], result[i][1]), i


# ---- 5. a bad member stays alone --------------------------------------------------------------------------------------------
def test_a_failed_member_stays_alone():
    log = bu.scene_log("tracking")
    head, rest = bu.prefix(log, 3), bu.suffix(log, 3)
    out = []
    for bad in (False, True):
        batch = _batch(3, noise={"q_cam": [0.3, 0.1, 0.5]})
        batch.process_detection_logs([head] * 3)
        if bad:
            ids = [k for k, _ in sorted(batch.landmarks[1].items(), key=lambda kv: kv[1])]
            s0 = batch.get_state(1)
            batch.set_member(1, s0, -np.eye(s0.shape[0]), ids)      # S = H (Q - I) H^T + R I cannot be positive definite
        filtered, smoothed = batch.smooth_detection_logs([rest, rest if bad else None, rest])
        out.append((filtered, smoothed, batch))
    (f0, s0_, _ref), (f1, s1, batch) = out
    assert batch.status() == [0, EKF_ERR_NUMERIC, 0] and batch.last_smooth_status.tolist() == [0, 0, 0]
    assert batch.history_records(1) == []
    assert f1[1].shape == (37, 7) and np.isnan(f1[1]).all() and np.isnan(s1[1]).all() and s1[1].shape == (37, 7)
    for b in (0, 2):
        assert np.array_equal(f0[b], f1[b]) and np.array_equal(s0_[b], s1[b])
        assert not np.isnan(s1[b]).any()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def _refused(batch, call, code=EKF_ERR_STATE):
    from aruco_slam_amd.hip_backend import EkfError
    before = sp.snap_batch(batch, tables=True)
    with pytest.raises(EkfError) as err:
        call()
    assert err.value.code == code, err.value
    assert sp.same(before, sp.snap_batch(batch, tables=True))


@pytest.mark.parametrize("kw", [{"model": "ekf_rotations", "quat_update": None, "max_landmarks": 10, "max_visible": 8},
                                {"quat_update": None}, {"wide_frames": True}, {"large_maps": True}])
def test_recording_refuses_what_is_not_supported(kw):
    log = mu.ragged_motion_log("rot" if kw.get("model") else "ekf")
    log = {k: log[k] for k in ("ids", "poses", "offsets", "has_detections")}
    batch = _batch(2, **kw)
    _refused(batch, lambda: batch.smooth_detection_logs([log, None]))
    assert batch.last_history is None and batch.num_landmarks == [0, 0]
    assert batch.process_detection_logs([log, None])[0].shape == (14, 7)      # the plain call runs


def test_recording_refuses_a_frozen_member_a_51st_landmark_and_a_small_history():
    import torch
    log = bu.scene_log("tracking")
    batch = _batch(2)
    batch.process_detection_logs([bu.prefix(log, 2), bu.prefix(log, 2)])
    batch.freeze_map(0)
    _refused(batch, lambda: batch.smooth_detection_logs([bu.suffix(log, 2), bu.suffix(log, 2)]))
    _refused(batch, lambda: batch.smooth_detection_logs([bu.suffix(log, 2), None]))
    assert len(batch.smooth_detection_logs([None, bu.suffix(log, 2)])[1][1]) == 38      # a frozen member without a log is fine
    # 51 landmarks: a batch that holds them, a log that reaches them
    big = _batch(2, max_landmarks=60)
    grown = su.growing_scene(16, 35, tail=0)
    grown = {k: grown[k] for k in ("ids", "poses", "offsets")}
    _refused(big, lambda: big.smooth_detection_logs([None, grown]))
    assert big.num_landmarks == [0, 0] and big.process_detection_logs([None, grown])[1].shape == (36, 7)
    # a history one byte short of ekf_batch_history_bytes (two frames that add one marker each: N = 13, 16)
    small = _batch(1)
    idx, fo, mf, poses = np.array([0, 1], np.int32), np.array([0, 1, 2]), np.array([0, 2]), log["poses"][:2]
    need = bu.history_bytes([[(13, True), (16, True)]], False)
    short = torch.empty((need - 256,), dtype=torch.uint8, device=small.device)
    _refused(small, lambda: small.observe_indexed(idx, fo, mf, poses, record=short), EKF_ERR_CAPACITY)
    exact = torch.empty((need,), dtype=torch.uint8, device=small.device)
    assert small.observe_indexed(idx, fo, mf, poses, record=exact).shape == (2, 7)


def test_smoothing_is_bound_to_the_last_recorded_call_and_to_untouched_members():
    log = bu.scene_log("ragged", with_motion=False, with_scale=False)
    batch = _batch(2)
    _f, first = batch.smooth_detection_logs([bu.prefix(log, 9), bu.prefix(log, 9)])
    history = batch.last_history
    assert np.array_equal(batch.smooth_history(history)[1], first[1])
    batch.smooth_detection_logs([bu.suffix(log, 9), None])
    _refused(batch, lambda: batch.smooth_history(history))            # the buffer of an earlier recorded call
    assert batch.smooth_history()[0].shape == (5, 7)
    batch.remove_markers({1: [100]})
    _refused(batch, lambda: batch.smooth_history())
    batch.smooth_detection_logs([None, bu.suffix(log, 9)])
    assert batch.smooth_history()[1].shape == (5, 7)
    batch.reset(0)
    _refused(batch, lambda: batch.smooth_history())
    _refused(batch, lambda: batch.history_records(1))


# ---- 7. replicas, and the point of it all ------------------------------------------------------------------------------------
def test_smooth_replicas_filters_like_replay_replicas_and_smoothing_pays_on_every_replica():
    log = bu.scene_log("tracking")
    kw = {"poses": bu.INIT, "max_landmarks": 10}
    plain, batch = _batch(bu.REPLICAS, **kw), _batch(bu.REPLICAS, **kw)
    want = plain.replay_replicas(log, bu.REPLICA_SIGMA, bu.REPLICA_SEED).trajectory
    filtered, smoothed = batch.smooth_replicas(log, bu.REPLICA_SIGMA, bu.REPLICA_SEED)
    assert filtered.shape == smoothed.shape == (bu.REPLICAS, 40, 7) and np.array_equal(filtered, want)
    assert sp.same(sp.snap_batch(plain, tables=True), sp.snap_batch(batch, tables=True))
    assert batch.last_smooth_status.tolist() == [0] * bu.REPLICAS
    for r in range(bu.REPLICAS):
        e0, e1 = mu.mean_position_error(filtered[r], log), mu.mean_position_error(smoothed[r], log)
        print(f"replica {r} on the device: filtered {e0:.4f} m, smoothed {e1:.4f} m, ratio {e1 / e0:.3f}")
        assert e1 <= su.TRACK_SMOOTH_RATIO * e0, r
    assert not np.array_equal(smoothed[0], smoothed[1])
    # B copies of the tracking scene: the 0.156 m -> 0.042 m of the single filter, per member
    copies = _batch(3, poses=bu.INIT, max_landmarks=10)
    f, s = copies.smooth_detection_logs([log] * 3)
    for b in range(3):
        e0, e1 = mu.mean_position_error(f[b], log), mu.mean_position_error(s[b], log)
        assert abs(e0 - 0.1562) < 5e-4 and abs(e1 - 0.0422) < 5e-4, (b, e0, e1)
        assert np.array_equal(f[b], f[0]) and np.array_equal(s[b], s[0])
