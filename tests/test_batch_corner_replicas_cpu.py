"""Replicas with pixel noise on the marker corners (``EKFBatch.replay_corner_replicas``), without a GPU: the NumPy mirror's
noise stream, the flips and margins of the inputs the GPU test compares on, ``synthetic.corner_log``, the new C ABI
(declared, exported, validated before any device work), the register / LDS budget of the new kernel, and the host side of
``replay_corner_replicas`` and of corner logs in ``process_detection_logs``."""
import ctypes

import numpy as np
import pytest

import corner_replica_util as cu
import replica_util as ru
import support as sp
from conftest import synthetic_marker_views
from support import lib

NEW_SYMBOLS = ("ekf_batch_replica_corners", "ekf_batch_observe_corner_replicas")
VIEWS, REPLICAS, SEED, MARKER = 48, 16, 7, 0.16


@pytest.fixture(scope="module")
def views():
    k, dist, corners, _tvecs, _rots = synthetic_marker_views(VIEWS, seed=3, marker_size=MARKER)
    return k, dist, corners


@pytest.fixture(scope="module")
def mirror(views):
    """sigma_px -> (poses, candidates) of replicas 0 .. 15 on the 48 views, computed once"""
    k, dist, corners = views
    return {s: cu.replica_corner_poses(corners, s, SEED, REPLICAS, k, dist, MARKER) for s in (0.5, 1.0)}


def test_mirror_corner_normals_are_the_pose_construction_on_counter_words_4_to_7():
    seed, reps, dets = 0xABCD_EF01_2345_6789, np.arange(5, 21), np.arange(40)
    g = cu.corner_normals(seed, reps, dets)
    assert g.shape == (16, 40, 4, 2) and np.isfinite(g).all()
    r, d = reps.astype(np.uint64).reshape(-1, 1), dets.astype(np.uint64).reshape(1, -1)
    for i in range(4):      # ru.normals' construction with counter word 4 + i in place of j
        x = ru.philox4x32_10((d & ru.MASK, d >> ru.S32, r, np.uint64(4 + i)), (seed & 0xFFFFFFFF, seed >> 32))
        ua, ub = ru.unit_open(x[0], x[1]), ru.unit_open(x[2], x[3])
        rad, ang = np.sqrt(-2.0 * np.log(ua)), 2.0 * np.pi * ub
        assert np.array_equal(g[:, :, i, 0], rad * np.cos(ang)) and np.array_equal(g[:, :, i, 1], rad * np.sin(ang))
    # disjoint from the pose stream (words 0 .. 2), and not a function of how many replicas a call holds
    assert np.intersect1d(g.reshape(-1), ru.normals(seed, reps, dets).reshape(-1)).size == 0
    assert np.array_equal(cu.corner_normals(seed, reps[4:9], dets), g[4:9])
    assert np.array_equal(cu.corner_normals(seed, [12], [33]), g[7:8, 33:34])
    assert not np.array_equal(cu.corner_normals(seed + 1, reps, dets), g)
    corners = np.arange(80.0).reshape(10, 4, 2)
    assert np.array_equal(cu.replica_corners(corners, 0.0, seed, 3), np.broadcast_to(corners, (3, 10, 4, 2)))
    want = corners[None] + np.array([0.5, 1.0, 2.0])[:, None, None, None] * cu.corner_normals(seed, [2, 3, 4], np.arange(10))
    assert np.array_equal(cu.replica_corners(corners, [0.5, 1.0, 2.0], seed, 3, first_replica=2), want)


@pytest.mark.parametrize("sigma_px,flips,per_replica", [(0.5, 59, 2), (1.0, 124, 4)])
def test_inputs_contain_flips_and_no_case_is_near_a_tie(mirror, sigma_px, flips, per_replica):
    """What the GPU test relies on: corner noise flips IPPE's choice in these inputs, and with these margins the device and
    the mirror cannot disagree about a choice (the two differ by ~1e-12 in the quantities compared), so the GPU test
    excludes nothing."""
    poses, cand = mirror[sigma_px]
    flipped = cand["flipped"]
    assert poses.shape == (REPLICAS, VIEWS, 6) and np.isfinite(poses).all()
    assert int(flipped.sum()) == flips
    assert flipped.sum(axis=1).min() >= per_replica
    assert np.abs(cand["trace"][..., 0] - cand["trace"][..., 1]).min() >= 2.0e-3
    err = cand["err"]
    assert (err[..., 0] <= err[..., 1]).all()
    assert ((err[..., 1] - err[..., 0]) / err[..., 1]).min() >= 1.3e-2
    # the returned candidate is the first one, and a flipped pose is far from the clean one
    assert np.array_equal(poses[..., :3], cand["tvec"][:, :, 0]) and np.array_equal(poses[..., 3:], cand["rvec"][:, :, 0])


def test_zero_noise_flips_nothing(views):
    k, dist, corners = views
    poses, cand = cu.replica_corner_poses(corners[:6], 0.0, SEED, 2, k, dist, MARKER)
    assert not cand["flipped"].any()
    assert np.array_equal(poses[0], poses[1]) and np.allclose(cand["trace"][..., 0], 3.0, atol=1e-12)


def _corner_log(n=12, m_range=(1, 4), steady=30, seed=5):
    from aruco_slam_amd.synthetic import corner_log
    k, dist, _c, _t, _r = synthetic_marker_views(1, seed=0)
    return k, dist, corner_log(n, m_range, steady, seed, k, dist, MARKER)


def test_corner_log_is_a_ragged_log_of_full_views():
    from scipy.spatial.transform import Rotation
    from oracle.ippe_numpy import estimate_pose_of_markers
    k, dist, log = _corner_log()
    ids, offs, corners, clean = log["ids"], log["offsets"], log["corners"], log["poses_clean"]
    D, F = ids.shape[0], offs.shape[0] - 1
    assert corners.shape == (D, 4, 2) and clean.shape == (D, 6) and offs[0] == 0 and offs[-1] == D
    assert log["has_detections"].shape == (F,) and F == log["bootstrap_frames"] + 30
    assert corners[..., 0].min() >= 0 and corners[..., 0].max() <= 1920
    assert corners[..., 1].min() >= 0 and corners[..., 1].max() <= 1080
    assert clean[:, 2].min() >= 1.4 and clean[:, 2].max() <= 4.1
    counts = np.diff(offs)
    assert counts.min() >= 1 and counts.max() <= 4 and len(set(counts[log["bootstrap_frames"]:])) > 1      # ragged
    boot = ids[:offs[log["bootstrap_frames"]]]
    assert sorted(boot) == list(range(12))                                   # the bootstrap first-sights all n
    for t in range(F):
        assert len(set(ids[offs[t]:offs[t + 1]])) == counts[t]
    # tilts from 0 to about 65 degrees: the angle between the marker's normal and the optical axis
    normal_z = np.array([Rotation.from_rotvec(v).as_matrix()[2, 2] for v in clean[:, 3:]])
    tilt = np.degrees(np.arccos(-normal_z))
    assert tilt.min() >= 0 and tilt.max() <= 70 and tilt.max() >= 30
    # a different camera for each frame: a marker's corners move between its sightings
    first = {}
    moved = 0
    for j, c in zip(ids, corners):
        moved += int(j in first and not np.array_equal(first[j], c))
        first.setdefault(j, c)
    assert moved == D - 12
    # the oracle's IPPE of the corners recovers the poses they were projected from
    est = estimate_pose_of_markers(corners, MARKER, k, dist)
    for j in range(D):
        assert np.abs(est[j, :3] - clean[j, :3]).max() <= 5e-5 * np.linalg.norm(clean[j, :3])
        assert np.abs((Rotation.from_rotvec(est[j, 3:]) * Rotation.from_rotvec(clean[j, 3:]).inv()).as_rotvec()).max() <= 5e-5
    # seeded
    assert all(np.array_equal(v, _corner_log()[2][key]) for key, v in log.items())
    assert not np.array_equal(_corner_log(seed=6)[2]["corners"][:4], corners[:4])


def test_corner_log_flips_at_one_pixel():
    k, dist, log = _corner_log(n=8, m_range=(2, 4), steady=12)
    _poses, cand = cu.replica_corner_poses(log["corners"], 1.0, SEED, 4, k, dist, MARKER)
    assert cand["flipped"].sum() >= 1


def test_new_symbols_are_declared_and_exported(lib):
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    for word in ("4 + i", "R_clean", "trace(R_a R_clean^T) < trace(R_b R_clean^T)"):
        assert word in header, word


def test_replica_corners_validates_before_any_device_work(lib):
    """Bad sigma_px, replica range, camera or marker size: EKF_ERR_INVALID before anything touches a device (no buffers
    are needed to find out)."""
    fake = ctypes.c_void_p(256)        # (never dereferenced: validation fails first)
    dp = ctypes.POINTER(ctypes.c_double)
    cam = np.array([900.0, 0, 960, 0, 900, 540, 0, 0, 1])
    dist = np.zeros(9)

    def call(sigma=(0.5, 0.5, 0.5), replicas=3, first=0, size=0.16, k=cam, n_dist=5):
        s = np.ascontiguousarray(sigma, dtype=np.float64)
        return lib.ekf_batch_replica_corners(fake, 10, s.ctypes.data_as(dp), replicas, 5, first, size,
                                             k.ctypes.data_as(dp) if k is not None else None, dist.ctypes.data_as(dp),
                                             n_dist, fake, fake, fake, None)

    for bad in (-1.0, np.nan, np.inf):
        assert call((0.5, 0.5, bad)) == -1, bad
        assert b"sigma_px" in lib.ekf_last_error_string()
    assert call(first=2 ** 32 - 2) == -1
    assert b"2^32" in lib.ekf_last_error_string()
    assert call(n_dist=9) == -1
    assert b"distortion" in lib.ekf_last_error_string()
    for size in (0.0, -0.16, np.nan):
        assert call(size=size) == -1
        assert b"marker_size" in lib.ekf_last_error_string()
    assert call(k=None) == -1
    assert call(k=np.zeros(9)) == -1
    assert b"focal" in lib.ekf_last_error_string()
    assert lib.ekf_batch_replica_corners(fake, -1, None, 3, 5, 0, 0.16, None, None, 0, fake, fake, fake, None) == -1
    assert call(replicas=0, first=2 ** 32 - 1) == 0          # (nothing to do)
    # the batch call checks its handle first
    assert lib.ekf_batch_observe_corner_replicas(None, None, None, 0, fake, None, 5, 0, 0.16, None, None, 0, fake, 0, fake,
                                                 None, None, None, None) == -1
    assert b"handle" in lib.ekf_last_error_string()


@pytest.mark.parametrize("src,pattern", [
    ("ekf_batch_corner_replicas.hip", r"ekf_corner_replicas_kernel"),
    ("ekf_batch_replicas.hip", r"ekf_replica_poses_kernel"),
    ("ekf_pose_ippe.hip", r"ekf_ippe_square_kernel"),
])
def test_kernels_use_no_scratch_no_spill_no_static_lds(src, pattern):
    """The new kernel, and the two that now share its headers: no scratch memory, no VGPR spills, no static LDS."""
    found = sp.kernel_resources(src, pattern)
    assert len(found) == 1, found
    for name, res in found.items():
        assert [res[k] for k in sp.BUDGET_FIELDS] == [0, 0, 0], (name, res)


def test_the_shared_device_code_has_one_definition():
    """Both IPPE kernels and both noise kernels run the headers' definitions: no copy is left in a kernel file."""
    from aruco_slam_amd import _build
    for header, word, users in (("ekf_ippe_device.h", "ippe_translation(const", ("ekf_pose_ippe.hip", "ekf_batch_corner_replicas.hip")),
                                ("ekf_philox.h", "void philox4x32_10(", ("ekf_batch_replicas.hip", "ekf_batch_corner_replicas.hip"))):
        assert word in (_build.CSRC / header).read_text() and header in _build.HEADERS
        for user in users:
            text = (_build.CSRC / user).read_text()
            assert f'#include "{header}"' in text and word not in text, (header, user)
    assert "ekf_batch_corner_replicas.hip" in _build.SOURCES


def test_sigma_px_shapes_and_values():
    from aruco_slam_amd.batch import replica_sigma_px
    assert np.array_equal(replica_sigma_px(0.5, 3), np.full(3, 0.5))
    assert np.array_equal(replica_sigma_px(0, 2), np.zeros(2))
    row = np.arange(4.0)
    got = replica_sigma_px(row[::-1], 4)
    assert np.array_equal(got, row[::-1]) and got.flags.c_contiguous and got.dtype == np.float64
    for bad in (-0.1, np.nan, np.inf, np.ones(3), np.ones((4, 1)), np.ones((4, 6)), [1.0, 1.0, 1.0, -1.0]):
        with pytest.raises(ValueError, match="sigma_px"):
            replica_sigma_px(bad, 4)


def test_camera_arguments():
    from aruco_slam_amd.batch import EKFBatch, camera_arrays
    k = np.array([[900.0, 0, 960], [0, 910, 540], [0, 0, 1]])
    cm, d, size = camera_arrays(k)
    assert cm.shape == (9,) and cm[4] == 910 and d.shape == (0,) and size == 0.16
    assert camera_arrays(k, np.arange(5.0).reshape(1, 5), 0.2)[1].shape == (5,)
    for args in ((np.eye(4),), (k, np.zeros(9)), (k, [np.nan]), (np.zeros((3, 3)),), (k, None, 0.0), (k, None, -1.0),
                 (k, None, np.inf)):
        with pytest.raises(ValueError):
            camera_arrays(*args)
    batch = object.__new__(EKFBatch)
    assert batch.camera is None
    with pytest.raises(ValueError):
        batch.set_camera(k, np.zeros(9))
    assert batch.camera is None           # (nothing changes)
    batch.set_camera(k, np.zeros(5), 0.1)
    assert batch.camera[2] == 0.1


def _host_batch(members=3, model="ekf", camera=True):
    """An EKFBatch without device state or library: observe_indexed records what would reach the library."""
    from aruco_slam_amd.batch import EKFBatch, LM_DIMS
    batch = object.__new__(EKFBatch)
    batch.members = members
    batch.model = model
    batch.lm_dims = LM_DIMS[model]
    batch.landmarks = [{} for _ in range(members)]
    batch.num_landmarks = [0] * members
    batch.calls = []
    if camera:
        batch.set_camera(np.array([[900.0, 0, 960], [0, 900, 540], [0, 0, 1]]))

    def observe_indexed(*args, **kw):
        batch.calls.append((args, kw))
        raise AssertionError("the library was reached")

    batch.observe_indexed = observe_indexed
    batch._estimate_corner_logs = observe_indexed
    batch._num_landmarks_device = lambda: np.zeros(members, dtype=np.int32)
    return batch


def test_replay_corner_replicas_checks_before_the_library():
    batch = _host_batch(3)
    log = {"ids": np.array([1, 2], np.int32), "corners": np.zeros((2, 4, 2)), "offsets": np.array([0, 1, 2])}
    batch.landmarks[1] = {5: 0}
    batch.num_landmarks[1] = 1
    with pytest.raises(ValueError, match="landmark table"):
        batch.replay_corner_replicas(log, 0.5, 1)
    batch.landmarks[1], batch.num_landmarks[1] = {}, 0
    for kw in ({"sigma_px": -1.0}, {"sigma_px": np.ones(2)}, {"sigma_px": np.ones((3, 6))}, {"sigma_px": np.nan},
               {"first_replica": -1}, {"first_replica": 2 ** 32 - 2}, {"seed": -3}, {"seed": 2 ** 64}):
        args = {"sigma_px": 0.5, "seed": 1, **kw}
        with pytest.raises(ValueError):
            batch.replay_corner_replicas(log, args.pop("sigma_px"), args.pop("seed"), **args)
    with pytest.raises(ValueError):
        batch.replay_corner_replicas(dict(log, offsets=np.array([0, 2, 1])), 0.5, 1)
    with pytest.raises(ValueError, match="corners"):
        batch.replay_corner_replicas(dict(log, corners=np.zeros((2, 6))), 0.5, 1)
    with pytest.raises(ValueError, match="corners"):
        batch.replay_corner_replicas(dict(log, corners=np.zeros((3, 4, 2))), 0.5, 1)
    with pytest.raises(ValueError, match="poses"):
        batch.replay_corner_replicas(dict(log, poses=np.zeros((2, 6))), 0.5, 1)
    with pytest.raises(KeyError):
        batch.replay_corner_replicas({k: v for k, v in log.items() if k != "corners"}, 0.5, 1)
    no_camera = _host_batch(3, camera=False)
    with pytest.raises(ValueError, match="set_camera"):
        no_camera.replay_corner_replicas(log, 0.5, 1)
    for b in (batch, no_camera):          # (neither holds a library: reaching it would have raised AttributeError)
        assert b.calls == [] and b.landmarks == [{}, {}, {}] and b.num_landmarks == [0, 0, 0]


def test_corner_logs_are_checked_before_the_library():
    batch = _host_batch(3)
    corners = {"ids": np.array([4, 9], np.int32), "corners": np.zeros((2, 4, 2)), "offsets": np.array([0, 1, 2])}
    poses = {"ids": np.array([4, 9], np.int32), "poses": np.zeros((2, 6)), "offsets": np.array([0, 1, 2])}
    neither = {"ids": np.array([4, 9], np.int32), "offsets": np.array([0, 1, 2])}
    with pytest.raises(ValueError, match="either poses"):
        batch.process_detection_logs([poses, dict(corners, poses=np.zeros((2, 6))), None])
    with pytest.raises(ValueError, match="either poses"):
        batch.process_detection_logs([corners, None, neither])
    with pytest.raises(ValueError, match=r"member 2: corners must have shape \(2, 4, 2\)"):
        batch.process_detection_logs([corners, None, dict(corners, corners=np.zeros((2, 8)))])
    with pytest.raises(ValueError, match="member 1: .*set_camera"):
        _host_batch(3, camera=False).process_detection_logs([poses, corners, None])
    assert batch.calls == [] and batch.landmarks == [{}, {}, {}]
