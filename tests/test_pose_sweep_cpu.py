"""The pose front end's sweep without a GPU: the extended reference against the projected truth, the f64 oracle against
the reference (the bound's form holds for a correct f64 implementation), what the case table reaches, and the device code
of ``ekf_ippe_square_kernel`` built for the host and run on the whole table under the bound the GPU test applies."""
import json

import numpy as np
import pytest

import pose_sweep_util as pu
import support as sp
from conftest import report
from oracle import ippe_extended as xt

CAMERAS = ("none", "calib5", "calib4", "rational8")
# the reference against the truth it was projected from: the f64 rounding of the pixel corners is all that separates them
# (relative u on coordinates up to 0.9 in normalised units, on a figure of size ell), so c of order 1
C_TRUTH = 4.0


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return sp.build_host_program("ippe_host_main", tmp_path_factory.mktemp("ippe_host"))


def test_reference_recovers_the_projected_truth():
    tab = pu.table("none")
    assert len(tab["index"]) == len(pu.views())          # (no view is dropped without distortion)
    r_r, r_t = np.empty(len(tab["index"])), np.empty(len(tab["index"]))
    for j, i in enumerate(tab["index"]):
        v = pu.views()[i]
        e_r, e_t = pu.errors(v["R"], v["t"], tab, j)
        r_r[j], r_t[j] = e_r / tab["scale"][j], e_t / tab["scale"][j]
    report("pose_sweep_reference_vs_truth", **pu.worst("none", r_r, r_t))
    assert r_r.max() <= C_TRUTH and r_t.max() <= C_TRUTH


@pytest.mark.parametrize("camera", CAMERAS)
def test_f64_oracle_is_inside_the_bound(camera):
    from oracle.ippe_numpy import estimate_pose_of_markers
    k, dist = pu.cameras()[camera]
    tab = pu.table(camera)
    r_r, r_t = pu.ratios(estimate_pose_of_markers(tab["corners"], pu.MARKER, k, dist), tab)
    report("pose_sweep_oracle", **pu.worst(camera, r_r, r_t))
    assert r_r.max() <= pu.C_BOUNDS["c_R"], pu.worst(camera, r_r, r_t)
    assert r_t.max() <= pu.C_BOUNDS["c_t"], pu.worst(camera, r_r, r_t)


@pytest.mark.parametrize("camera", CAMERAS)
def test_host_build_of_the_device_code_is_inside_the_bound(host_program, camera):
    """csrc/ekf_ippe_device.h as the kernel runs it, compiled for the host (tests/host/ippe_host_main.hip).  Before the
    rotation vector went through the quaternion this failed inside cv::Rodrigues' window: ratio_R 1.2e10 at tilt 0.3,
    phi = pi/2 - 3e-5 (7.4e-6 rad), 6e8 at tilt 1.0, phi = pi/2 + 8e-6, 1.2e9 at tilt 1e-6 rolled by pi."""
    k, dist = pu.cameras()[camera]
    tab = pu.table(camera)
    poses, _best = pu.run_host_program(host_program, tab["corners"], k, dist)
    assert np.isfinite(poses).all()
    r_r, r_t = pu.ratios(poses, tab)
    report("pose_sweep_host_build", **pu.worst(camera, r_r, r_t))
    assert r_r.max() <= pu.C_BOUNDS["c_R"], pu.worst(camera, r_r, r_t)
    assert r_t.max() <= pu.C_BOUNDS["c_t"], pu.worst(camera, r_r, r_t)


def test_host_build_gives_nan_for_degenerate_detections(host_program):
    k, dist = pu.cameras()["calib5"]
    good = pu.table("calib5")["corners"][:3]
    bad = pu.degenerate_detections(good[0])
    poses, _ = pu.run_host_program(host_program, np.concatenate([good, np.stack(list(bad.values()))]), k, dist)
    assert np.isfinite(poses[:3]).all()
    for name, p in zip(bad, poses[3:]):
        assert np.isnan(p).all(), (name, p)


def test_table_reaches_every_branch_of_the_quaternion_step():
    """The matrix -> quaternion step (ekf_ippe_device.h: ippe_rotvec; restated in ippe_extended.quat_branch) picks the
    largest of trace, R00, R11, R22: the reference rotations of the table reach all four, and in the three branches where
    w is a difference of off-diagonal entries they lie on both sides of w = 0 (rotation angle pi) within 1e-4."""
    tab = pu.table("none")
    branches, near_pi = set(), set()
    for rot in tab["R"][:, 0]:
        br = xt.quat_branch(rot)
        branches.add(br)
        if br:
            w = {1: rot[2, 1] - rot[1, 2], 2: rot[0, 2] - rot[2, 0], 3: rot[1, 0] - rot[0, 1]}[br]
            if abs(w) < 1e-4:
                near_pi.add((br, bool(w < 0)))
    assert branches == {0, 1, 2, 3}
    assert {(1, False), (1, True), (2, False), (2, True)} <= near_pi
    # the small-angle end: a reference rotation within 1e-6 of the identity that is not the identity
    angles = [float(np.sqrt(v @ v)) for v in (xt.rotvec_from_matrix_ld(r) for r in tab["R"][:, 0])]
    assert any(0.0 < a < 1e-6 for a in angles) and min(angles) < 1e-15 and max(angles) > np.pi - 1e-15


def test_table_covers_every_factor_on_and_off_the_axis():
    grid = [v for v in pu.views() if v["kind"] == "grid"]
    for key, values in (("tilt", pu.TILTS), ("phi", pu.PHIS), ("roll", pu.ROLLS)):
        for val in values:
            assert {v["on_axis"] for v in grid if v[key] == val} == {True, False}, (key, val)
    assert {tuple(v["t"]) for v in grid} == set(pu.T_ON + pu.T_OFF)
    assert sum(v["kind"] == "back" for v in pu.views()) == 2 * len(pu.BACK_FACING)
    assert sum(v["kind"] == "generic" for v in pu.views()) == pu.GENERIC
    assert len(pu.views()) <= 500
    for camera in CAMERAS:       # distortion drops views whose corners leave the image, and never a factor's value
        kept = [pu.views()[i] for i in pu.table(camera)["index"]]
        assert len(kept) >= 300
        for key, values in (("tilt", pu.TILTS), ("phi", pu.PHIS), ("roll", pu.ROLLS)):
            assert {v[key] for v in kept if v["kind"] == "grid"} == set(values)


@pytest.mark.parametrize("camera", CAMERAS)
def test_reference_ties_only_on_axis_at_tilts_up_to_1e_9(camera):
    """The rule 'the nearer of the reference's two candidates counts' is open to the on-axis cases with tilt <= 1e-9 (the
    angle between the marker's normal and the optical axis: the grid's tilt, and 0 for the back-facing view R = I) and to no
    other; checked on the reference alone (17 cases without distortion, none with: there the residual of the five
    iterations separates the two errors)."""
    tab = pu.table(camera)
    for j in np.nonzero(tab["tie"])[0]:
        v = pu.views()[tab["index"][j]]
        assert v["on_axis"] and v["normal_tilt"] <= pu.TIE_TILT_MAX * (1 + 1e-6), pu.describe(camera, j)
        assert v["kind"] == "back" or v["tilt"] <= pu.TIE_TILT_MAX
        # and there the candidates are one pose to the square root of what the f64 pixel corners carry: they differ by 2 b,
        # b^2 = 1 - |c|^2 = O(u / ell) (measured: up to 3 sqrt(u / ell), at the 5 px marker)
        d = tab["R"][j, 0] - tab["R"][j, 1]
        assert float(np.sqrt(np.sum(d * d) / 2)) <= 8 * np.sqrt(pu.U / tab["ell"][j])


def test_constants_follow_the_measured_summary():
    """profiles/pose_sweep/summary.json holds the worst ratios per camera and implementation; the asserted constants are the
    kernel's worst ratio on an MI355X with a head-room of at most 8, and stay within 8 x the f64 oracle's own worst."""
    s = json.loads(pu.SUMMARY.read_text())
    for key, c in (("ratio_R", pu.C_BOUNDS["c_R"]), ("ratio_t", pu.C_BOUNDS["c_t"])):
        gpu = max(s["gpu"][cam][key] for cam in CAMERAS)
        oracle = max(s["f64_oracle"][cam][key] for cam in CAMERAS)
        assert gpu <= c <= pu.HEADROOM_MAX * gpu, (key, gpu, c)
        assert c <= 8.0 * oracle, (key, oracle, c)
    assert set(s) >= {"reference_vs_truth", "f64_oracle", "host_build", "gpu"}
    assert all(set(s[impl]) == set(CAMERAS) for impl in ("f64_oracle", "host_build", "gpu"))
