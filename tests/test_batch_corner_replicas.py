"""Replicas with pixel noise on the marker corners (``EKFBatch.replay_corner_replicas``, ``replica_corner_poses``,
``replica_corners``) and corner logs in ``process_detection_logs``, on an MI355X: the kernel against the NumPy mirror (poses
and every flip label), the device noise against the mirror and its statistics, replicas equal to explicit logs of the poses
they consumed, zero noise equal to the plain front end, replica identity across batch sizes and calls, the alignment of
``flipped`` with the log's own detections, and bad arguments."""
import numpy as np
import pytest

import corner_replica_util as cu
import support as sp
from conftest import report, synthetic_marker_views

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
MARKER = 0.16
# family: (model, the batch's keyword arguments, corner_log's n, m_range, steady frames)
FAMILIES = {
    "ekf-column": ("ekf", {"max_landmarks": 12, "max_visible": 16}, 12, (1, 4), 30),
    "rot-column": ("ekf_rotations", {"max_landmarks": 12, "max_visible": 8}, 12, (1, 4), 30),
    "ekf-wide": ("ekf", {"max_landmarks": 20, "max_visible": 20, "wide_frames": True}, 20, (14, 20), 12),
}


@pytest.fixture(scope="module")
def camera():
    k, dist, _c, _t, _r = synthetic_marker_views(1, seed=0)
    return k, dist


def _batch(family, members, camera, **extra):
    from aruco_slam_amd.batch import EKFBatch
    model, kw, *_ = FAMILIES[family]
    batch = EKFBatch(members, INIT, model=model, **kw, **extra)
    if camera is not None:
        batch.set_camera(camera[0], camera[1], MARKER)
    return batch


def _log(family, camera, seed=5):
    from aruco_slam_amd.synthetic import corner_log
    _model, _kw, n, m_range, steady = FAMILIES[family]
    return corner_log(n, m_range, steady, seed, camera[0], camera[1], MARKER)


def _pose_log(log, poses):
    return {"ids": log["ids"], "offsets": log["offsets"], "has_detections": log["has_detections"], "poses": poses}


def _corner_only(log):
    return {k: v for k, v in log.items() if k != "poses_clean"}


@pytest.mark.parametrize("sigma_px,flips", [(0.5, 59), (1.0, 124)])
def test_kernel_against_the_mirror(sigma_px, flips):
    """Poses and flip labels of 16 replicas of 48 views.  Bounds: the project's own for this IPPE kernel against this oracle
    (test_pose_front_end_kernel_vs_oracle_and_projected_poses).  Every one of the 768 pairs is compared: the CPU test holds
    the margins that make a disagreement about a choice impossible."""
    from scipy.spatial.transform import Rotation
    from aruco_slam_amd.batch import replica_corner_poses, replica_corners
    k, dist, corners, _t, _r = synthetic_marker_views(48, seed=3, marker_size=MARKER)
    want, cand = cu.replica_corner_poses(corners, sigma_px, 7, 16, k, dist, MARKER)
    got, flipped = replica_corner_poses(corners, sigma_px, 7, k, dist, MARKER, replicas=16, flipped=True)
    noisy = replica_corners(corners, sigma_px, 7, k, dist, MARKER, replicas=16)
    assert got.shape == (16, 48, 6) and flipped.shape == (16, 48) and flipped.dtype == bool and noisy.shape == (16, 48, 4, 2)
    d_noisy = float(np.abs(noisy - cu.replica_corners(corners, sigma_px, 7, 16)).max())
    d_t = float(np.abs(got[..., :3] - want[..., :3]).max())
    rel = Rotation.from_rotvec(got[..., 3:].reshape(-1, 3)) * Rotation.from_rotvec(want[..., 3:].reshape(-1, 3)).inv()
    d_r = float(np.abs(rel.as_rotvec()).max())
    report("corner_replica_poses", sigma_px=sigma_px, pairs=int(flipped.size), flipped=int(flipped.sum()),
           flip_mismatches=int((flipped != cand["flipped"]).sum()), tvec_abs=d_t, rotvec_abs=d_r, corners_abs=d_noisy)
    assert np.isfinite(got).all()
    # corner + sigma g, corner < 2048: the normals' 4e-15 and one ulp of the sum (2.3e-13: an fma rounds once, the mirror twice)
    assert d_noisy <= 5e-13, d_noisy
    assert d_t <= 1e-9, d_t
    assert d_r <= 1e-9, d_r
    assert np.array_equal(flipped, cand["flipped"])
    assert int(flipped.sum()) == flips
    # the poses alone are the same bits, whatever else is asked for
    assert np.array_equal(replica_corner_poses(corners, sigma_px, 7, k, dist, MARKER, replicas=16), got)


def test_device_corner_noise_matches_the_mirror_and_is_standard_normal(camera):
    from aruco_slam_amd.batch import replica_corners
    R, D = 128, 1400                    # 1,433,600 samples
    seed, r0 = 0x1234_5678_9ABC_DEF0, 2 ** 32 - R      # (both key words and the top replica numbers in use)
    g = replica_corners(np.zeros((D, 4, 2)), 1.0, seed, camera[0], camera[1], MARKER, replicas=R, first_replica=r0)
    want = cu.corner_normals(seed, np.arange(r0, r0 + R), np.arange(D))
    err = float(np.abs(g - want).max())
    n = g.size
    mean, var = float(g.mean()), float(g.var())
    flat = g.reshape(R, D, 8)
    comp = np.corrcoef(flat[..., :7].reshape(-1), flat[..., 1:].reshape(-1))[0, 1]
    adj = np.corrcoef(g[:-1].reshape(-1), g[1:].reshape(-1))[0, 1]
    det = np.corrcoef(g[:, :-1].reshape(-1), g[:, 1:].reshape(-1))[0, 1]
    report("corner_replica_normals", samples=n, max_abs_vs_mirror=err, mean=mean, var=var, corr_components=comp,
           corr_adjacent_replicas=adj, corr_adjacent_detections=det)
    assert err <= 4e-15, err
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n)
    for c in range(8):
        gc = flat[..., c].reshape(-1)
        assert abs(gc.mean()) <= 5 / np.sqrt(gc.size) and abs(gc.var() - 1) <= 5 * np.sqrt(2 / gc.size), c
    assert abs(comp) <= 5 / np.sqrt(flat[..., :7].size)
    assert abs(adj) <= 5 / np.sqrt(g[:-1].size) and abs(det) <= 5 / np.sqrt(g[:, :-1].size)


@pytest.mark.parametrize("family,gate", [("ekf-column", None), ("rot-column", None), ("ekf-wide", None),
                                         ("ekf-column", 7.815)])
def test_replicas_equal_explicit_logs_of_their_poses(camera, family, gate):
    from aruco_slam_amd.batch import replica_corner_poses
    B, seed, r0 = 6, 0x5EED_0000_0000_0042, 3
    log = _log(family, camera)
    sigma_px = np.random.default_rng(1).uniform(0.2, 1.0, B)
    extra = {} if gate is None else {"gate": gate}
    batch, explicit = _batch(family, B, camera, **extra), _batch(family, B, None, **extra)
    got = batch.replay_corner_replicas(_corner_only(log), sigma_px, seed, first_replica=r0, nis=True, cam_cov=True,
                                       mahal=gate is not None)
    poses, flipped = replica_corner_poses(log["corners"], sigma_px, seed, *camera, MARKER, first_replica=r0, flipped=True)
    assert poses.shape == (B, log["corners"].shape[0], 6) and np.array_equal(got.flipped, flipped)
    want = explicit.process_detection_logs([_pose_log(log, poses[b]) for b in range(B)], nis=True, cam_cov=True,
                                           mahal=gate is not None)
    assert batch.status() == explicit.status()
    if FAMILIES[family][0] == "ekf":
        assert batch.status() == [0] * B
    assert np.isfinite(got.trajectory).any()
    assert sp.same(got.trajectory, np.stack(want.trajectory), equal_nan=True)
    assert sp.same(got.nis, np.stack(want.nis), equal_nan=True)
    assert sp.same(got.cam_cov, np.stack(want.cam_cov), equal_nan=True)
    if gate is None:
        assert got.mahal is None and got.rejected is None and np.array_equal(got.dof, want.dof[0])
    else:
        assert sp.same(got.mahal, np.stack(want.mahal), equal_nan=True) and np.array_equal(got.rejected, np.stack(want.rejected))
        assert np.array_equal(got.dof, np.stack(want.dof)) and got.dof.shape == got.nis.shape
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(explicit), "state / P", equal_nan=True)
    assert batch.landmarks == explicit.landmarks
    assert not np.array_equal(got.trajectory[0], got.trajectory[1])      # (replicas differ: sigma_px > 0)
    report("corner_replicas_vs_explicit", family=family, gated=gate is not None, flipped=int(got.flipped.sum()),
           rejected=int(got.rejected.sum()) if gate is not None else -1)


@pytest.mark.parametrize("family", ["ekf-column", "rot-column"])
def test_zero_sigma_is_the_plain_front_end(camera, family):
    from aruco_slam_amd import hip_backend
    B = 4
    log = _log(family, camera, seed=3)
    batch, plain = _batch(family, B, camera), _batch(family, B, None)
    got = batch.replay_corner_replicas(_corner_only(log), 0.0, 99, nis=True, cam_cov=True)
    poses = hip_backend.estimate_poses(log["corners"], MARKER, *camera)
    want = plain.process_detection_logs([_pose_log(log, poses)] * B, nis=True, cam_cov=True)
    assert not got.flipped.any() and got.flipped.shape == (B, log["ids"].shape[0])
    assert np.isfinite(got.trajectory).any()
    assert sp.same(got.trajectory, np.stack(want.trajectory), equal_nan=True)
    assert sp.same(got.nis, np.stack(want.nis), equal_nan=True) and sp.same(got.cam_cov, np.stack(want.cam_cov), equal_nan=True)
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(plain), "state / P", equal_nan=True)


def test_corner_logs_in_process_detection_logs(camera):
    from aruco_slam_amd import hip_backend
    logs = [_log("ekf-column", camera, seed=s) for s in range(4)]
    est = [hip_backend.estimate_poses(lg["corners"], MARKER, *camera) for lg in logs]
    # corner logs mixed with pose logs and a member without a log
    mixed = [_corner_only(logs[0]), _pose_log(logs[1], est[1]), None, _corner_only(logs[2]), _pose_log(logs[3], est[3]),
             _corner_only(logs[1])]
    as_poses = [_pose_log(logs[0], est[0]), _pose_log(logs[1], est[1]), None, _pose_log(logs[2], est[2]),
                _pose_log(logs[3], est[3]), _pose_log(logs[1], est[1])]
    a, b = _batch("ekf-column", 6, camera), _batch("ekf-column", 6, None)
    got = a.process_detection_logs(mixed, nis=True, cam_cov=True)
    want = b.process_detection_logs(as_poses, nis=True, cam_cov=True)
    assert a.status() == b.status() == [0] * 6
    for m in range(6):
        assert np.array_equal(got.trajectory[m], want.trajectory[m]) and np.array_equal(got.nis[m], want.nis[m])
        assert np.array_equal(got.cam_cov[m], want.cam_cov[m])
    sp.assert_same(sp.snap_batch(a), sp.snap_batch(b), "state / P", equal_nan=True)
    assert a.landmarks == b.landmarks
    # every log a corner log: the plain return value
    c, d = _batch("ekf-column", 2, camera), _batch("ekf-column", 2, None)
    for x, y in zip(c.process_detection_logs([_corner_only(logs[0]), _corner_only(logs[3])]),
                    d.process_detection_logs([_pose_log(logs[0], est[0]), _pose_log(logs[3], est[3])])):
        assert np.array_equal(x, y)


def test_replica_identity_across_batch_sizes_and_calls(camera):
    seed = 2024
    sigma_px = np.random.default_rng(5).uniform(0.0, 1.0, 16)
    log = _corner_only(_log("ekf-column", camera, seed=11))
    big = _batch("ekf-column", 16, camera)
    whole = big.replay_corner_replicas(log, sigma_px, seed, nis=True, cam_cov=True)
    big_snap = sp.snap_batch(big)
    assert whole.flipped.any()
    for r0 in (0, 8, 4):
        part = _batch("ekf-column", 8, camera)
        out = part.replay_corner_replicas(log, sigma_px[r0:r0 + 8], seed, first_replica=r0, nis=True, cam_cov=True)
        sl = slice(r0, r0 + 8)
        assert np.array_equal(out.trajectory, whole.trajectory[sl]) and np.array_equal(out.flipped, whole.flipped[sl])
        assert np.array_equal(out.nis, whole.nis[sl]) and np.array_equal(out.cam_cov, whole.cam_cov[sl])
        sp.assert_same(sp.snap_batch(part), big_snap[sl], f"members {r0}..{r0 + 7}", equal_nan=True)


def test_flipped_is_aligned_with_the_logs_own_detections(camera):
    """A frame with a duplicate id (kept: both detections count) and a frame flagged as without detections whose ids are
    listed all the same (dropped by the planner): ``flipped`` has the log's own length, the dropped entries are False and
    the others are the labels of the planned detections, which are what the device numbers."""
    from aruco_slam_amd.batch import replica_corner_poses
    log = _corner_only(_log("ekf-column", camera, seed=8))
    offs, boot = log["offsets"], log["bootstrap_frames"]
    ids = log["ids"].copy()
    wide = boot + int(np.argmax(np.diff(offs)[boot:] >= 2))
    ids[offs[wide] + 1] = ids[offs[wide]]                     # a duplicate id inside a frame
    has = log["has_detections"].copy()
    off = [t for t in range(boot + 1, boot + 8) if t != wide][:2]
    has[off] = False                                          # listed, but not detections
    log = dict(log, ids=ids, has_detections=has)
    keep = np.repeat(has, np.diff(offs))
    assert 0 < (~keep).sum() < keep.size
    B, sigma_px, seed = 8, 1.5, 31
    batch = _batch("ekf-column", B, camera)
    got = batch.replay_corner_replicas(log, sigma_px, seed, mahal=True)
    assert batch.status() == [0] * B
    _poses, flipped = replica_corner_poses(log["corners"][keep], sigma_px, seed, *camera, MARKER, replicas=B, flipped=True)
    assert flipped.any()
    assert got.flipped.shape == (B, keep.size) and got.flipped.dtype == bool
    assert np.array_equal(got.flipped[:, keep], flipped) and not got.flipped[:, ~keep].any()
    assert np.isnan(got.mahal[:, ~keep]).all() and got.rejected.shape == got.flipped.shape
    assert got.dof.shape == (B, offs.shape[0] - 1) and (got.dof[:, off] == 0).all()
    assert (got.dof[:, wide] == 3 * (offs[wide + 1] - offs[wide])).all()      # (no gate: nothing rejected, duplicates count)


def test_bad_arguments_raise_before_anything_runs(camera):
    from aruco_slam_amd.hip_backend import EkfError
    from aruco_slam_amd.synthetic import corner_log
    log = _corner_only(_log("ekf-column", camera, seed=2))
    batch = _batch("ekf-column", 3, camera)
    batch.replay_corner_replicas(log, 0.5, 1)
    before, tables = sp.snap_batch(batch), [dict(t) for t in batch.landmarks]
    wide = _corner_only(corner_log(20, (17, 20), 2, 4, camera[0], camera[1], MARKER))
    pose_log = _pose_log(log, np.zeros((log["ids"].shape[0], 6)))
    cases = [
        ("negative", lambda: batch.replay_corner_replicas(log, -0.1, 1), ValueError),
        ("nan", lambda: batch.replay_corner_replicas(log, np.full(3, np.nan), 1), ValueError),
        ("shape", lambda: batch.replay_corner_replicas(log, np.ones(2), 1), ValueError),
        ("first_replica", lambda: batch.replay_corner_replicas(log, 0.5, 1, first_replica=2 ** 32 - 2), ValueError),
        ("poses", lambda: batch.replay_corner_replicas(pose_log, 0.5, 1), ValueError),
        ("corner shape", lambda: batch.replay_corner_replicas(dict(log, corners=log["corners"][:-1]), 0.5, 1), ValueError),
        ("capacity", lambda: batch.replay_corner_replicas(wide, 0.5, 1), EkfError),
        ("both keys", lambda: batch.process_detection_logs([log, dict(log, poses=pose_log["poses"]), None]), ValueError),
        ("log capacity", lambda: batch.process_detection_logs([log, wide, None]), EkfError),
    ]
    for name, call, exc in cases:
        with pytest.raises(exc) as info:
            call()
        if exc is EkfError:
            assert info.value.code == -2, name
        assert batch.landmarks == tables, name
        sp.assert_same(before, sp.snap_batch(batch), name, equal_nan=True)
        assert batch.status() == [0, 0, 0]
    no_camera = _batch("ekf-column", 3, None)
    with pytest.raises(ValueError, match="set_camera"):
        no_camera.replay_corner_replicas(log, 0.5, 1)
    with pytest.raises(ValueError, match="set_camera"):
        no_camera.process_detection_logs([log, None, None])
    assert no_camera.landmarks == [{}, {}, {}]
    batch.reset(1)
    with pytest.raises(ValueError, match="landmark table"):
        batch.replay_corner_replicas(log, 0.5, 1)
    sp.assert_same(before[::2], sp.snap_batch(batch)[::2], "unequal tables", equal_nan=True)
