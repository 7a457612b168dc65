"""Log replay on an MI355X: ``BaseFilter.process_detection_log`` (ekf_observe_log) against a second filter stepped by the
per-frame ``process_detections`` loop on the same log.  EKF: every trajectory row, the state and the full covariance are
bitwise equal.  EKF_Rotations: z is formed on the device (sin / cos may differ from the host's in the last place), 1e-12 on
the trajectory and state, 2^-52 on the quaternion of z."""
import argparse

import numpy as np
import pytest

import support as sp
from conftest import chaos_horizon, load_npz, rel_err, rel_err_elem, report

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])


def _ekf(dtype="float64", n=16, m=8, **kw):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    return EKF(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, **kw)


def _rot(dtype="float64", n=8, m=6, **kw):
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    return EKF_Rotations(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, **kw)


def _load(name):
    det = np.load(name, allow_pickle=False)
    return {k: det[k] for k in det.files}


def _per_frame(flt, log, frames=None):
    """process_detections frame by frame (what run_slam does); the camera pose [0:7] after every frame, as float."""
    offs, has = log["offsets"], log["has_detections"]
    rows = []
    for t in range(len(offs) - 1) if frames is None else frames:
        sl = slice(int(offs[t]), int(offs[t + 1]))
        ids = log["ids"][sl] if has[t] else None
        _, cam, _, _ = flt.process_detections(ids, log["poses"][sl])
        rows.append(np.asarray(cam, dtype=np.float64)[:7])
    return np.array(rows).reshape(-1, 7)


def _replay(flt, log):
    return flt.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"])


def _assert_filters_equal(fa, fb):
    assert fa.landmarks == fb.landmarks and fa.num_landmarks == fb.num_landmarks
    sp.assert_same(np.asarray(fa.state, np.float64), np.asarray(fb.state, np.float64), "state")
    sp.assert_same(fa.uncertainty, fb.uncertainty, "covariance")


@pytest.fixture(scope="module")
def c1(golden_dir):
    return _load(golden_dir / "c1_detections.npz")


@pytest.fixture(scope="module")
def g5(golden_dir):
    return _load(golden_dir / "g5_detections.npz")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_c1_log_bitwise_equals_per_frame_loop(c1, dtype):
    ref = _ekf(dtype)
    want = _per_frame(ref, c1)
    flt = _ekf(dtype)
    got = _replay(flt, c1)
    sp.assert_same(got, want, "trajectory")
    _assert_filters_equal(flt, ref)
    stats = flt.backend.last_log_stats()
    counts = np.diff(c1["offsets"])
    assert stats["frames_stepped"] == int((counts > 0).sum()) == 196
    assert stats["markers_added"] == len(flt.landmarks)
    report(f"log_c1_{dtype}", **stats)


def _run_slam(tmp_path, name, log_path, filt, resident, kwargs):
    from aruco_slam_amd.main import run_slam
    out = tmp_path / name
    args = argparse.Namespace(video="input_video.mp4", filter=filt, detections=str(log_path), output_dir=str(out),
                              filter_kwargs=kwargs, resident=resident)
    run_slam.main(args)
    return (out / "trajectory.txt").read_text(), (out / "map.txt").read_text()


def test_run_slam_resident_c1_matches_per_frame_run(tmp_path, golden_dir):
    kw = {"max_landmarks": 16, "max_visible": 8}
    log = golden_dir / "c1_detections.npz"
    t_res, m_res = _run_slam(tmp_path, "resident", log, "ekf", True, kw)
    t_pf, m_pf = _run_slam(tmp_path, "per_frame", log, "ekf", False, kw)
    assert t_res == t_pf and m_res == m_pf
    # the checks of test_c1_run_slam_outputs_vs_reference_files
    ref_t = (golden_dir / "g3_trajectory.txt").read_text()
    assert t_res.splitlines()[0] == ref_t.splitlines()[0] == "0.0333 0 0 0 1 0 0 0"
    assert [ln.split()[0] for ln in t_res.splitlines()] == [ln.split()[0] for ln in ref_t.splitlines()]
    a, b = sp.parse_trajectory(t_res), sp.parse_trajectory(ref_t)
    assert a.shape == b.shape == (200, 8)
    hz = chaos_horizon(load_npz("g3_free_run.npz"))
    assert rel_err(a[:hz + 1], b[:hz + 1]) <= 1e-4
    ref_m = (golden_dir / "g3_map.txt").read_text()
    assert m_res.splitlines()[:4] == ref_m.splitlines()[:4]
    gi, gx, gu = sp.parse_map(m_res)
    ri, rx, ru = sp.parse_map(ref_m)
    assert gi == ri and gx.shape == rx.shape and gu.shape == ru.shape
    assert np.isfinite(gx).all() and (gu > 0).all()


def test_rotations_g5_log_matches_per_frame_loop(g5):
    ref = _rot()
    want = _per_frame(ref, g5)
    flt = _rot()
    got = _replay(flt, g5)
    assert flt.landmarks == ref.landmarks
    errs = dict(traj=float(np.abs(got - want).max()), state=float(np.abs(flt.state - ref.state).max()))
    report("log_g5_rotations", **errs)
    assert errs["traj"] <= 1e-12 and errs["state"] <= 1e-12, errs


def test_run_slam_resident_rotations_g5(tmp_path, golden_dir):
    t_res, m_res = _run_slam(tmp_path, "resident", golden_dir / "g5_detections.npz", "ekf_rotations", True,
                             {"max_landmarks": 8, "max_visible": 6})
    ref_t, ref_m = (golden_dir / "g5_trajectory.txt").read_text(), (golden_dir / "g5_map.txt").read_text()
    assert t_res.splitlines()[0] == ref_t.splitlines()[0] == "0.0333 0 0 0 1 0 0 0"
    assert [ln.split()[0] for ln in t_res.splitlines()] == [ln.split()[0] for ln in ref_t.splitlines()]
    a = np.array([[float(v) for v in ln.split()] for ln in t_res.splitlines()])
    b = np.array([[float(v) for v in ln.split()] for ln in ref_t.splitlines()])
    assert a.shape == b.shape == (120, 8)
    assert m_res.splitlines()[:4] == ref_m.splitlines()[:4]
    lg, lr = m_res.splitlines()[4:], ref_m.splitlines()[4:]
    assert len(lg) == len(lr)
    assert [int(lg[i]) for i in range(0, len(lg) - 2, 4)] == [int(lr[i]) for i in range(0, len(lr) - 2, 4)]
    num = lambda lines, off: np.array([[float(t) for t in lines[i + off].split(", ")]       # noqa: E731
                                       for i in range(0, len(lines) - 2, 4)])
    errs = dict(traj_norm=rel_err(a, b), traj_elem=rel_err_elem(a, b), map_norm=rel_err(num(lg, 1), num(lr, 1)),
                map_elem=rel_err_elem(num(lg, 1), num(lr, 1)), unc_norm=rel_err(num(lg, 2), num(lr, 2)),
                unc_elem=rel_err_elem(num(lg, 2), num(lr, 2)))
    report("run_slam_resident_rotations", **errs)
    assert max(errs["traj_norm"], errs["map_norm"], errs["unc_norm"]) <= 1e-9, errs
    assert max(errs["traj_elem"], errs["map_elem"], errs["unc_elem"]) <= 1e-6, errs


def test_rotations_device_quaternion_matches_host():
    """z of a few hundred random rvecs, formed by the prepare kernel, against euler_xyz_to_quat (one landmark seen in
    every frame; the z block of the log workspace is read back after the call)."""
    import torch
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    rng = np.random.default_rng(5)
    count = 300
    poses = np.zeros((count, 6))
    poses[:, 0:3] = np.array([0.1, -0.2, 2.0]) + rng.normal(0.0, 0.01, size=(count, 3))
    poses[:, 3:6] = rng.uniform(-np.pi, np.pi, size=(count, 3))
    flt = _rot()
    flt.process_detection_log(np.full(count, 7, dtype=np.int32), poses, np.arange(count + 1), np.ones(count, dtype=bool))
    z = flt.backend._log_keep[1][:count * 7 * 8].view(torch.float64).reshape(count, 7).cpu().numpy()
    sp.assert_same(z[:, 0:3], poses[:, 0:3], "z position")
    err = float(np.abs(z[:, 3:7] - euler_xyz_to_quat(poses[:, 3:6])).max())
    report("log_rot_quaternion", max_abs=err)
    # (device sin / cos are not always correctly rounded: a component may land one or two units in the last place away,
    # at most 2^-52 for components below 1)
    assert err <= 2.0 ** -52, err


def _ragged_test_log(seed=11, n=256, frames=300):
    """m from 1 to 64, a different m every frame (runs of one kpad class, then another), first sightings at the start and
    in the middle, duplicate ids, empty frames, and one wide frame (m = 80)."""
    from aruco_slam_amd.synthetic import SyntheticStream
    stream = SyntheticStream(n, 64, seed=seed)
    rng = stream.rng
    first_half = 200                                   # landmarks 0..199 at the start, 200..255 at frame 150
    classes = [(1, 5), (6, 10), (17, 21), (27, 32), (33, 37), (43, 48), (59, 64)]
    out, prev_m = [], 0
    for t in range(frames):
        if t < 10:
            ids = np.arange(20 * t, 20 * t + 20)
            ids = np.concatenate((ids, ids[:3]))       # duplicates inside a first-sighting frame
        elif t == 150:
            ids = np.concatenate((np.arange(first_half, n), rng.choice(first_half, 4, replace=False)))
        elif t == 200:
            ids = rng.choice(n, 80, replace=False)     # wide frame
        elif t % 37 == 0 or t == 151:
            ids = np.zeros(0, dtype=np.int64)          # empty frame
        else:
            lo, hi = classes[(t // 15) % len(classes)]
            m = prev_m
            while m == prev_m:
                m = int(rng.integers(lo, hi + 1))
            pool = first_half if t < 150 else n
            ids = rng.choice(pool, m, replace=m > pool)
            if t % 5 == 0 and m > 1:
                ids[-1] = ids[0]                       # a duplicate detection
        if len(ids):
            prev_m = len(ids)
        out.append(stream._observe(np.asarray(ids, dtype=np.int64)))
    counts = np.array([len(i) for i, _ in out])
    return {"ids": np.concatenate([i for i, _ in out]).astype(np.int32), "poses": np.concatenate([p for _, p in out]),
            "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64), "has_detections": counts > 0}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_ragged_synthetic_log_bitwise(dtype):
    import torch
    log = _ragged_test_log()
    ref = _ekf(dtype, n=256, m=64)
    want = _per_frame(ref, log)
    flt = _ekf(dtype, n=256, m=64)
    got = _replay(flt, log)
    sp.assert_same(got, want, "trajectory")
    _assert_filters_equal(flt, ref)
    stats = flt.backend.last_log_stats()
    report(f"log_ragged_{dtype}", **stats)
    assert stats["frames_stepped"] == int((np.diff(log["offsets"]) > 0).sum())
    assert stats["markers_added"] == 256
    # is the pipelined mode available on this handle?  A fixed-m probe says so (after the comparison: it steps the filter)
    b = flt.backend
    idx = torch.zeros((2, 8), dtype=torch.int32, device=b.device)
    z = torch.zeros((2, 8, 3), dtype=torch.float64, device=b.device)
    z[..., 2] = 1.0
    b.observe_sequence(idx, z)
    b.sync()
    mode = b.last_sequence_mode()
    if mode != "pipelined":
        pytest.skip(f"the pipelined mode is not available on this handle ({mode}); results were checked")
    assert stats["frames_pipelined"] > 0 and stats["pipelined_runs"] > 1, stats


def test_log_split_and_interop(c1):
    import torch
    ref = _ekf()
    want = _per_frame(ref, c1)
    # one call == three calls back to back
    flt = _ekf()
    got = np.concatenate([_replay(flt, sp.sub_log(c1, a, b)) for a, b in ((0, 70), (70, 71), (71, 200))])
    sp.assert_same(got, want, "trajectory, three calls")
    _assert_filters_equal(flt, ref)
    # per-frame observe before and after a log call
    mix = _ekf()
    rows = [_per_frame(mix, c1, range(0, 40)), _replay(mix, sp.sub_log(c1, 40, 150)), _per_frame(mix, c1, range(150, 200))]
    sp.assert_same(np.concatenate(rows), want, "trajectory, per-frame / log / per-frame")
    _assert_filters_equal(mix, ref)
    # a small filter that grows through process_detection_log == one created large
    small, large = _ekf(n=8, m=4), _ekf(n=64, m=32)
    sp.assert_same(_replay(small, c1), _replay(large, c1), "trajectory, grown")
    _assert_filters_equal(small, large)
    # a device tensor for the poses == the NumPy form
    dev = _ekf()
    poses_t = torch.from_numpy(c1["poses"]).to(dev.backend.device)
    got_t = dev.process_detection_log(c1["ids"], poses_t, c1["offsets"], c1["has_detections"])
    sp.assert_same(got_t, want, "trajectory, tensor poses")
    _assert_filters_equal(dev, ref)


def test_rejected_log_leaves_the_filter_unchanged(c1):
    from aruco_slam_amd.hip_backend import EkfError
    flt = _ekf()
    _replay(flt, sp.sub_log(c1, 0, 120))
    state, cov, known = flt.state.copy(), flt.uncertainty.copy(), dict(flt.landmarks)
    b = flt.backend
    n = flt.num_landmarks
    poses = np.zeros((3, 6))
    poses[:, 2] = 1.0
    for idx, code in (([0, n + 1, 1], -1),          # a first sighting that skips an index
                      ([0, -1, 1], -1)):            # a negative index
        with pytest.raises(EkfError) as err:
            b.observe_log(np.array(idx), np.array([0, 3]), poses)
        assert err.value.code == code
    # more landmarks than the buffers hold: EKF_ERR_CAPACITY (the library never grows inside the call)
    extra = b.max_landmarks - n + 1
    assert 0 < extra <= b.max_visible
    poses_x = np.tile(poses[:1], (extra, 1))
    with pytest.raises(EkfError) as err:
        b.observe_log(np.arange(n, n + extra), np.array([0, extra]), poses_x)
    assert err.value.code == -2
    offs_bad = np.array([0, 2, 1, 3])
    with pytest.raises(EkfError) as err:
        b.observe_log(np.array([0, 1, 2]), offs_bad, poses)
    assert err.value.code == -1
    b.sync()
    sp.assert_same(flt.state, state, "state after rejected logs")
    sp.assert_same(flt.uncertainty, cov, "covariance after rejected logs")
    assert flt.landmarks == known
    # and the filter goes on exactly like one that never saw them
    ref = _ekf()
    _replay(ref, sp.sub_log(c1, 0, 120))
    _replay(flt, sp.sub_log(c1, 120, 200))
    _replay(ref, sp.sub_log(c1, 120, 200))
    _assert_filters_equal(flt, ref)


def _concat(*logs):
    counts = np.concatenate([np.diff(lg["offsets"]) for lg in logs])
    return {"ids": np.concatenate([lg["ids"] for lg in logs]).astype(np.int32),
            "poses": np.concatenate([lg["poses"] for lg in logs]),
            "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64),
            "has_detections": np.concatenate([lg["has_detections"] for lg in logs])}


def _frames(id_lists, poses_from):
    """A small log: one frame per id list (empty list: empty frame), poses taken from the rows of `poses_from`."""
    counts = np.array([len(i) for i in id_lists])
    ids = np.array([i for frame in id_lists for i in frame], dtype=np.int32)
    return {"ids": ids, "poses": np.array([poses_from[k % len(poses_from)] for k in range(len(ids))]).reshape(-1, 6),
            "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64), "has_detections": counts > 0}


def test_state_getter_right_after_observe_log(c1):
    """HipEkf.observe_log on a log that ends in a pipelined run after serial frames, then a state getter with no sync in
    between: it must see the state of the log's last frame."""
    from aruco_slam_amd.filters.base_filter import plan_detection_log
    first = [int(i) for i in c1["ids"][:2]]
    log = _concat(c1, _frames([first] * 6, c1["poses"]))        # 6 frames of m = 2 at the end: one pipelined run
    ref = _ekf()
    _per_frame(ref, log)
    want = ref.state
    flt = _ekf()
    b = flt.backend
    plan = plan_detection_log({}, 0, log["ids"], log["offsets"], log["has_detections"])
    b.observe_log(plan.index, plan.offsets, log["poses"][plan.keep])
    got = b.get_state()                                          # straight after the call
    got_cam = b.get_state(10)
    stats = b.last_log_stats()
    sp.assert_same(got, want, "state right after observe_log")
    sp.assert_same(got_cam, want[:10], "camera right after observe_log")
    report("log_getter_after_call", **stats)
    if stats["frames_pipelined"] == 0:
        pytest.skip("the pipelined mode is not available on this handle; the getter was checked on serial frames only")
    assert stats["frames_stepped"] > stats["frames_pipelined"], stats


def test_first_sighting_after_odd_run_following_a_smaller_checkpoint(c1, tmp_path):
    """A filter that ran a log with pipelined runs loads a checkpoint of a SMALLER map (ekf_set_state / ekf_set_cov, no
    reset), then replays a log whose first pipelined run has an odd number of frames and is followed by a first sighting:
    the new landmark must start with zero cross-covariances, as in the per-frame path."""
    from aruco_slam_amd.filters.base_filter import plan_detection_log
    big = _ekf()
    _replay(big, c1)
    def landmarks_after(t):
        part = sp.sub_log(c1, 0, t)
        return plan_detection_log({}, 0, part["ids"], part["offsets"], part["has_detections"]).num_landmarks
    k = next(t for t in range(1, 200) if landmarks_after(t) >= 3)
    small = _ekf()
    _replay(small, sp.sub_log(c1, 0, k))
    assert 3 <= small.num_landmarks < big.num_landmarks
    ck = tmp_path / "small.npz"
    small.save_checkpoint(str(ck))
    big.load_checkpoint(str(ck))
    ref = _ekf()
    ref.load_checkpoint(str(ck))
    known = sorted(small.landmarks)[:3]
    tail = _frames([known[:2], known[:3], known[:1], [known[0], 777, known[1]], known[:2], known[:3]], c1["poses"])
    got = _replay(big, tail)
    want = _per_frame(ref, tail)
    sp.assert_same(got, want, "trajectory")
    _assert_filters_equal(big, ref)
    report("log_after_smaller_checkpoint", **big.backend.last_log_stats())


def test_back_to_back_log_calls_queue_without_waiting(c1):
    """Four observe_log calls back to back on one handle (the staging is used by turns), then one sync: the same bits as
    one call."""
    from aruco_slam_amd.filters.base_filter import plan_detection_log
    ref = _ekf()
    want = _replay(ref, c1)
    flt = _ekf()
    b = flt.backend
    import torch
    trajs, landmarks, n = [], {}, 0
    for a, e in ((0, 50), (50, 100), (100, 150), (150, 200)):
        part = sp.sub_log(c1, a, e)
        plan = plan_detection_log(landmarks, n, part["ids"], part["offsets"], part["has_detections"])
        landmarks.update(plan.new_landmarks)
        n = plan.num_landmarks
        traj = torch.empty((e - a, 7), dtype=torch.float64, device=b.device)
        b.observe_log(plan.index, plan.offsets, part["poses"][plan.keep], traj)
        trajs.append(traj)
    b.sync()
    got = torch.cat(trajs).cpu().numpy()
    sp.assert_same(got, want, "trajectory, four calls")
    sp.assert_same(b.get_state(), ref.state, "state, four calls")
    sp.assert_same(b.get_cov(), ref.uncertainty, "covariance, four calls")
