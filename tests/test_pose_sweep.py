"""The pose front end on the GPU (``ekf_ippe_square_kernel``, and the corner-replica kernel that shares its device code)
against the extended-precision reference over the edge-geometry table of ``pose_sweep_util``: the conditioned bound per
camera, independence of a marker's pose from its position in the batch, degenerate detections, argument edges.  All of it
is a handful of launches of a few hundred threads."""
import ctypes

import numpy as np
import pytest

import pose_sweep_util as pu
from conftest import report
from support import lib

pytestmark = pytest.mark.gpu
CAMERAS = ("none", "calib5", "calib4", "rational8")
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def gpu_poses():
    """``estimate_poses`` on every camera's table, once."""
    from aruco_slam_amd import hip_backend
    return {cam: hip_backend.estimate_poses(pu.table(cam)["corners"], pu.MARKER, *pu.cameras()[cam]) for cam in CAMERAS}


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _device_call(lib, corners, count, k, dist, n_dist, marker_size=pu.MARKER, tail=0):
    """ekf_estimate_poses_device on the first ``count`` of ``corners``, into a sentinel-filled buffer of 6 count + tail
    doubles; returns (return code, the buffer)."""
    import torch
    dev = torch.device("cuda:0")
    with torch.cuda.device(dev):
        src = torch.from_numpy(np.ascontiguousarray(corners, dtype=np.float64)).to(dev)
        out = torch.full((6 * count + tail,), SENTINEL, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev)
        kk = np.ascontiguousarray(k, dtype=np.float64).reshape(9)
        rc = lib.ekf_estimate_poses_device(src.data_ptr(), count, float(marker_size), _dp(kk),
                                           _dp(dist) if dist is not None else None, n_dist, out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("camera", CAMERAS)
def test_sweep_is_inside_the_conditioned_bound(gpu_poses, camera):
    tab = pu.table(camera)
    got = gpu_poses[camera]
    assert got.shape == (len(tab["index"]), 6) and np.isfinite(got).all()
    r_r, r_t = pu.ratios(got, tab)
    w = pu.worst(camera, r_r, r_t)
    report("pose_sweep_gpu", **w, c_R=pu.C_BOUNDS["c_R"], c_t=pu.C_BOUNDS["c_t"])
    assert r_r.max() <= pu.C_BOUNDS["c_R"], w
    assert r_t.max() <= pu.C_BOUNDS["c_t"], w


def test_a_pose_does_not_depend_on_the_batch_around_it(lib):
    """The table's first 129 markers in batches of 1, 63, 64, 65 and 129 (64 threads per block): marker j's six outputs are
    the same bits in every batch that holds it, and nothing is written behind the last marker."""
    k, dist = pu.cameras()["rational8"]
    corners = pu.table("rational8")["corners"][:129]
    assert len(corners) == 129
    outs = {}
    for count in (1, 63, 64, 65, 129):
        rc, buf = _device_call(lib, corners[:count], count, k, dist, 8, tail=70)
        assert rc == 0
        assert np.all(buf[6 * count:] == SENTINEL), count
        outs[count] = buf[:6 * count].reshape(count, 6)
        assert np.isfinite(outs[count]).all()
    for count, got in outs.items():
        assert np.array_equal(got, outs[129][:count]), count
    rc, buf = _device_call(lib, corners[:1], 0, k, dist, 8, tail=6)
    assert rc == 0 and np.all(buf == SENTINEL)          # count = 0: OK, nothing runs


def test_degenerate_detections_give_non_finite_poses_and_leave_the_others_alone():
    """Collinear, identical or coincident corners, a NaN or Inf coordinate: the marker's pose is six NaN
    (``np.isfinite(pose).all()`` is the caller's validity test, include/ekf_slam_hip.h), the call returns OK and every other
    marker of the batch has the bits it has without them."""
    from aruco_slam_amd import hip_backend
    k, dist = pu.cameras()["calib5"]
    good = pu.table("calib5")["corners"][:70]
    alone = hip_backend.estimate_poses(good, pu.MARKER, k, dist)
    bad = pu.degenerate_detections(good[3])
    assert {"collinear", "identical", "coincident_0_1", "nan_0", "inf_7"} <= set(bad)
    names = list(bad)
    # degenerate ones in front, in between, one before each marker across the block boundary, and at the end
    before = {0: names[0], 5: names[1], 30: names[2]}
    before.update({38 + i: name for i, name in enumerate(names[3:-2])})
    assert max(before) < len(good)
    rows, is_bad = [], []
    for j, c in enumerate(good):
        if j in before:
            rows.append(bad[before[j]]); is_bad.append(True)
        rows.append(c); is_bad.append(False)
    for name in names[-2:]:
        rows.append(bad[name]); is_bad.append(True)
    is_bad = np.array(is_bad)
    assert is_bad.sum() == len(bad) and is_bad[0] and is_bad[-1] and is_bad[60:70].any()
    got = hip_backend.estimate_poses(np.stack(rows), pu.MARKER, k, dist)
    assert np.isnan(got[is_bad]).all()
    assert np.array_equal(got[~is_bad], alone) and np.isfinite(alone).all()
    # without distortion (collinear corners stay collinear there: another way through the arithmetic)
    got0 = hip_backend.estimate_poses(np.stack(rows), pu.MARKER, k, None)
    assert np.isnan(got0[is_bad]).all() and np.isfinite(got0[~is_bad]).all()


def test_argument_edges(lib, gpu_poses):
    """n_dist 0, 4, 5, 8 accepted (0 with a pointer that is then not read), 9 and -1 rejected; marker_size 0 and NaN,
    fx <= 0 rejected; each rejection before anything runs (the output buffer keeps its sentinel)."""
    from aruco_slam_amd import hip_backend
    k, d5 = pu.cameras()["calib5"]
    corners = pu.table("calib5")["corners"][:65]
    d9 = np.concatenate([np.array(pu.RATIONAL8), [0.3]])
    for n_dist, dist, camera in ((0, d9, "none"), (4, d5, "calib4"), (5, d5, "calib5"), (8, d9, "rational8")):
        rc, buf = _device_call(lib, corners, 65, k, dist, n_dist)
        assert rc == 0, n_dist
        # the same bits as the camera that has exactly these coefficients gives for these corners
        want = hip_backend.estimate_poses(corners, pu.MARKER, *pu.cameras()[camera])
        assert np.array_equal(buf.reshape(65, 6), want), n_dist
    # n_dist = 0 through a non-NULL pointer on the undistorted table: what dist = None gives
    rc, buf = _device_call(lib, pu.table("none")["corners"], len(pu.table("none")["index"]), k, d9, 0)
    assert rc == 0 and np.array_equal(buf.reshape(-1, 6), gpu_poses["none"])
    bad_fx, bad_fy = np.array(k, dtype=np.float64), np.array(k, dtype=np.float64)
    bad_fx[0, 0], bad_fy[1, 1] = 0.0, -1414.0
    for kwargs, word in ((dict(n_dist=9, dist=d9), b"distortion"), (dict(n_dist=-1, dist=d9), b"distortion"),
                         (dict(n_dist=5, dist=d5, marker_size=0.0), b"marker_size"),
                         (dict(n_dist=5, dist=d5, marker_size=float("nan")), b"marker_size"),
                         (dict(n_dist=5, dist=d5, k=bad_fx), b"focal"), (dict(n_dist=5, dist=d5, k=bad_fy), b"focal")):
        kw = dict(k=k, marker_size=pu.MARKER)
        kw.update(kwargs)
        rc, buf = _device_call(lib, corners, 65, kw["k"], kw["dist"], kw["n_dist"], marker_size=kw["marker_size"])
        assert rc == -1 and word in lib.ekf_last_error_string(), kwargs
        assert np.all(buf == SENTINEL), kwargs


@pytest.mark.parametrize("camera", ("none", "rational8"))
def test_corner_replicas_without_noise_are_estimate_poses_to_the_bit(gpu_poses, camera):
    """The replica kernel runs the same device code: with sigma_px = 0 every replica is ``estimate_poses`` bit for bit, and
    no pair is flipped -- the reference's tie cases left out (on-axis, tilt <= 1e-9: test_pose_sweep_cpu holds that cap),
    where the two candidates are the same pose to sqrt u."""
    from aruco_slam_amd.batch import replica_corner_poses
    tab = pu.table(camera)
    k, dist = pu.cameras()[camera]
    poses, flipped = replica_corner_poses(tab["corners"], 0.0, 11, k, dist, pu.MARKER, replicas=2, flipped=True)
    assert poses.shape == (2, len(tab["index"]), 6) and flipped.shape == (2, len(tab["index"]))
    for r in range(2):
        assert np.array_equal(poses[r], gpu_poses[camera]), r
    report("pose_sweep_replica_flips", camera=camera, flipped=int(flipped.sum()), flipped_at_ties=int(flipped[:, tab["tie"]].sum()),
           ties=int(tab["tie"].sum()))
    assert not flipped[:, ~tab["tie"]].any(), [pu.describe(camera, j) for j in np.nonzero(flipped[0] & ~tab["tie"])[0]]
