"""Offline smoothing on the device: the recorded replay against the plain one (bit for bit), the records against the filter,
both tiers of the backward pass against the longdouble oracle of ``smooth_util`` under its bound, read-only and repeatable,
and the way up through ``EKF.smooth_detection_log``, ``process_detections(should_filter=False)`` and ``run_slam --smooth``.
Scenes, tables and the bound: ``smooth_util.py`` (``test_smooth_cpu.py`` checks them without a GPU)."""
import numpy as np
import pytest

import motion_util as mu
import smooth_util as su
import support as sp
import update_sweep_util as sw

pytestmark = pytest.mark.gpu
INIT = sw.INIT


def _filter(n=8, m=8, **kw):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    kw.setdefault("quat_update", "scalar_first")
    return EKF(INIT, max_landmarks=n, max_visible=m, **kw)


def _plan(flt, log):
    from aruco_slam_amd.filters.base_filter import plan_detection_log
    return plan_detection_log(flt.landmarks, flt.num_landmarks, log["ids"], log["offsets"], log.get("has_detections"))


def _replay(flt, log, record, motion=None, scale=None, mahal=False):
    """One log call on the back end; returns (trajectory, d2 | None, history | None)."""
    import torch
    b = flt.backend
    plan = _plan(flt, log)
    if plan.num_landmarks > b.max_landmarks:
        b.grow(plan.num_landmarks)
    if plan.widest > b.max_visible:
        b.grow(new_max_visible=plan.widest)
    frames = len(plan.offsets) - 1
    traj = torch.empty((frames, 7), dtype=torch.float64, device=b.device)
    d2 = torch.empty((len(plan.index),), dtype=torch.float64, device=b.device) if mahal else None
    history = b.new_history(plan.index, plan.offsets) if record else None
    b.observe_log(plan.index, plan.offsets, log["poses"], traj, d2, None, scale, motion, **({"history": history} if record else {}))
    b.sync()
    flt.landmarks.update(plan.new_landmarks)
    flt.num_landmarks = plan.num_landmarks
    return traj.cpu().numpy(), None if d2 is None else d2.cpu().numpy(), history


# ---- 1. recorded replay = plain replay ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["motion", "scale", "gate"])
def test_recorded_replay_is_the_plain_replay_bit_for_bit(case):
    log = mu.ragged_motion_log("ekf")
    kw = {"motion": True, "frame_scale": case == "scale", "gate": 1e-3 if case == "gate" else None}
    args = {"motion": log["motion"], "scale": su.RAGGED_SCALE if case == "scale" else None, "mahal": case == "gate"}
    out = []
    for record in (False, True):
        flt = _filter(**kw)
        traj, d2, _h = _replay(flt, log, record, **args)
        out.append((traj, d2, *sp.snap_backend(flt.backend), flt.backend.last_log_stats(),
                    flt.backend.last_gate_stats() if case == "gate" else None))
    plain, rec = out
    assert np.array_equal(plain[0], rec[0]) and np.array_equal(plain[2], rec[2]) and np.array_equal(plain[3], rec[3])
    assert plain[4] == rec[4] and plain[5] == rec[5]
    if case == "gate":
        assert np.array_equal(plain[1], rec[1], equal_nan=True)
        # the gate (1e-3) rejects what is not a first sighting: of the 10 frames with detections, those without one lose
        # all of theirs and are not stepped (frames 1, 3 and 8 sight new markers)
        assert rec[5]["rejected"] > 0 and 3 <= rec[4]["frames_stepped"] < 10


# ---- 2. records are the filter -----------------------------------------------------------------------------------------------
def test_records_are_the_filter_and_the_table_is_the_plan():
    log = mu.ragged_motion_log("ekf")
    flt = _filter(motion=True, frame_scale=True)
    _traj, _d2, history = _replay(flt, log, True, motion=log["motion"], scale=su.RAGGED_SCALE)
    records, info = su.device_records(flt.backend, history)
    table = [(r["frame"], r["dims"], r["stepped"], r["s_eff"]) for r in records]
    assert table == su.RAGGED_TABLE
    assert info["frame_record"].tolist() == list(range(14))
    for r, rec in enumerate(records):      # moved-only records carry the motion, records of the still frames none
        assert np.array_equal(rec["u"], log["motion"][rec["frame"]])
    assert not records[2]["u"].any() and not records[9]["u"].any()
    offs = log["offsets"]
    for r in (0, 6, 13):
        t1 = records[r]["frame"] + 1
        d1 = int(offs[t1])
        prefix = {"ids": log["ids"][:d1], "poses": log["poses"][:d1], "offsets": offs[:t1 + 1],
                  "has_detections": log["has_detections"][:t1]}
        twin = _filter(motion=True, frame_scale=True)
        _replay(twin, prefix, False, motion=log["motion"][:t1], scale=su.RAGGED_SCALE[:t1])
        state, cov = sp.snap_backend(twin.backend)
        assert np.array_equal(records[r]["x"], state) and np.array_equal(records[r]["P"], cov), r
    # ekf_history_bytes: by hand for a 3-frame log that adds 2, 0 and 1 markers to an empty filter (N = 16, 16, 19)
    fresh = _filter()
    assert fresh.backend.history_bytes([0, 1, 0, 1, 2], [0, 2, 3, 5]) == 256 + 1280 + 1280 + 1792


# ---- 3. / 4. the two tiers against the oracle ----------------------------------------------------------------------------------
def _smoothed_case(name, blocked):
    log, motion, scale = su.scene(name)
    flt = _filter(motion=motion is not None, frame_scale=scale is not None)
    traj, _d2, history = _replay(flt, log, True, motion=motion, scale=scale)
    before = sp.snap_backend(flt.backend)
    frames = traj.shape[0]
    got = flt.backend.smooth_history(history, frames, blocked=blocked).cpu().numpy()
    after = sp.snap_backend(flt.backend)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])      # read-only
    records, _info = su.device_records(flt.backend, history)
    ref = su.smooth_records(records, frames, INIT)
    return flt, history, traj, got, records, ref


@pytest.mark.parametrize("name,blocked", [("tracking", False), ("ragged", False), ("n50", False),
                                          ("n18", True), ("n19", True), ("ragged", True), ("n51", False), ("n49_52", False),
                                          ("n82", False), ("g81_2", False)])
def test_backward_pass_against_the_oracle_under_the_bound(name, blocked):
    """Resident tier: tracking (N = 40), ragged with motion and scale, n = 50 (N grows to 160 inside the pass).  Blocked tier:
    forced at N = 64 and 67 and on the ragged log (its motions), natural at N = 163, on the log that grows through 160, at
    N = 256 (exactly four blocks, no padding row) and on the log whose npad goes 256 -> 320 inside the pass (measured worst
    error / bound on one MI355X: 0.0050 and 0.0081)."""
    _flt, _history, traj, got, records, ref = _smoothed_case(name, blocked)
    assert max(r["dims"] for r in records) == su.EXPECTED_DIMS[name]
    assert (max(r["dims"] for r in records) > su.RESIDENT_DIMS) == (name in su.BLOCKED_SCENES)
    ratio = su.worst_ratio(got, ref, records)
    print(f"{name} blocked={blocked}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    last = records[-1]["frame"]
    assert np.array_equal(got[last:], traj[last:])                           # the last record's rows are the filtered ones
    first = records[0]["frame"]
    assert np.array_equal(got[:first], np.tile(INIT[:7], (first, 1)))         # before the first record: the start pose


def test_both_tiers_agree_on_the_tracking_scene():
    flt, history, _traj, got, records, ref = _smoothed_case("tracking", False)
    blocked = flt.backend.smooth_history(history, 40, blocked=True).cpu().numpy()
    assert su.worst_ratio(blocked, ref, records) <= 1.0 and su.worst_ratio(got, ref, records) <= 1.0
    assert np.abs(blocked - got).max() <= 2 * su.bound(ref, records).max()


# ---- 5. read-only and repeatable -----------------------------------------------------------------------------------------------
def test_the_smoother_is_repeatable_and_bound_to_the_last_recorded_call():
    from aruco_slam_amd.hip_backend import EkfError
    flt, history, _traj, got, _records, _ref = _smoothed_case("ragged", False)
    b = flt.backend
    again = b.smooth_history(history, 14).cpu().numpy()
    assert np.array_equal(got, again)
    blocked = [b.smooth_history(history, 14, blocked=True).cpu().numpy() for _ in range(2)]
    assert np.array_equal(blocked[0], blocked[1])
    # a plain observe on the filter changes nothing about the history
    log = mu.ragged_motion_log("ekf")
    sl = slice(int(log["offsets"][-2]), int(log["offsets"][-1]))
    flt.observe(log["ids"][sl], log["poses"][sl])
    assert np.array_equal(b.smooth_history(history, 14).cpu().numpy(), got)
    # after a second recorded call the first buffer is refused
    tail = {"ids": log["ids"][sl], "poses": log["poses"][sl], "offsets": np.array([0, sl.stop - sl.start]),
            "has_detections": np.array([True])}
    _t, _d, second = _replay(flt, tail, True, motion=np.zeros((1, 6)))
    with pytest.raises(EkfError) as err:
        b.smooth_history(history, 14)
    assert err.value.code == -4      # EKF_ERR_STATE
    assert b.smooth_history(second, 1).shape == (1, 7)
    # ... and so is a filter that remove_markers touched since the recording
    flt.remove_markers([100])
    with pytest.raises(EkfError) as err:
        b.smooth_history(second, 1)
    assert err.value.code == -4


@pytest.mark.parametrize("kw", [{"quat_update": "as_written"}, {"cov_dtype": "float32"}])
def test_the_c_entry_points_refuse_what_is_not_supported(kw):
    from aruco_slam_amd.hip_backend import EkfError
    log = mu.ragged_motion_log("ekf")
    flt = _filter(motion=True, **kw)
    before = sp.snap_backend(flt.backend)
    with pytest.raises(EkfError) as err:
        _replay(flt, log, True, motion=log["motion"])
    assert err.value.code == -4 and flt.backend.num_landmarks == 0
    after = sp.snap_backend(flt.backend)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_smooth_detection_log_meets_the_tracking_condition_and_feeds_get_cam_estimate(tmp_path):
    import argparse
    from aruco_slam_amd.main import run_slam
    from aruco_slam_amd.outputs.trajectory_writer import TrajectoryWriter
    scene = mu.tracking_scene("ekf")
    flt, twin = _filter(n=10, m=10), _filter(n=10, m=10)
    filtered, smoothed = flt.smooth_detection_log(scene["ids"], scene["poses"], scene["offsets"])
    plain = twin.process_detection_log(scene["ids"], scene["poses"], scene["offsets"])
    assert np.array_equal(filtered, plain)
    # the filter is where process_detection_log leaves it
    for u, v in zip(sp.snap_backend(flt.backend), sp.snap_backend(twin.backend)):
        assert np.array_equal(u, v)
    e0, e1 = mu.mean_position_error(filtered, scene), mu.mean_position_error(smoothed, scene)
    print(f"tracking scene on the device: filtered {e0:.4f} m, smoothed {e1:.4f} m")
    assert e1 <= su.TRACK_SMOOTH_RATIO * e0
    # process_detections(should_filter=False, iteration=i) returns the smoothed pose and steps nothing
    before = sp.snap_backend(flt.backend)
    sl = slice(int(scene["offsets"][7]), int(scene["offsets"][8]))
    _, cam, _markers, _ = flt.process_detections(scene["ids"][sl], scene["poses"][sl], should_filter=False, iteration=7)
    assert cam.shape == (10,) and np.array_equal(cam[:7], smoothed[7]) and not cam[7:].any()
    assert np.array_equal(before[0], sp.snap_backend(flt.backend)[0])
    with pytest.raises(IndexError):
        flt.get_cam_estimate(40)
    with pytest.raises(NotImplementedError):
        twin.get_cam_estimate(0)
    # run_slam --resident --smooth writes that trajectory
    frames = len(scene["offsets"]) - 1
    stamps = 33.3 * np.arange(frames)
    np.savez(tmp_path / "log.npz", ids=scene["ids"], poses=scene["poses"], offsets=scene["offsets"], timestamps_ms=stamps,
             has_detections=np.ones(frames, dtype=bool))
    run_slam.main(run_slam.build_parser().parse_args(["--detections", str(tmp_path / "log.npz"), "--resident", "--smooth",
                                                      "--output-dir", str(tmp_path / "out")]))
    with TrajectoryWriter(str(tmp_path / "want.txt")) as writer:
        for t in range(frames):
            writer.write(float(stamps[t]), smoothed[t])
    assert (tmp_path / "out" / "trajectory.txt").read_text() == (tmp_path / "want.txt").read_text()
    run_slam.main(argparse.Namespace(filter="ekf", detections=str(tmp_path / "log.npz"), video=None, resident=True,
                                     output_dir=str(tmp_path / "plain"), filter_kwargs={"quat_update": "scalar_first"}))
    assert (tmp_path / "plain" / "trajectory.txt").read_text() != (tmp_path / "want.txt").read_text()
