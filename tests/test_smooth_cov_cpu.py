"""Smoothed covariances without a GPU: the covariance rule of ``smooth_cov_util`` on the oracle filter's records -- the
room under the bound, the two forms against each other, P_r - P^s_r positive semi-definite -- on every fixture of the GPU
tests, then the header, the exported symbols and the Python layer with a fake back end.  ``test_smooth_cov.py`` runs the
device against the same helpers."""
import numpy as np
import pytest

import smooth_cov_util as sc
import smooth_util as su
import support as sp
import update_sweep_util as sw
from support import lib

NEW_SYMBOLS = ("ekf_smooth_cov_workspace_bytes", "ekf_smooth_history_cov")


@pytest.fixture(scope="module")
def runs():
    """Per scene: (records of the oracle filter, the longdouble run, the f64 run of the products form, the f64 direct run)."""
    out = {}
    for name in sc.CPU_SCENES:
        log, motion, scale = sc.scene(name)
        records, _filtered, _start = su.oracle_records(log, motion, scale)
        out[name] = (records, sc.smooth_cov_records(records), sc.smooth_cov_records(records, np.float64, "products"),
                     sc.smooth_cov_records(records, np.float64, "direct"))
    return out


@pytest.mark.parametrize("name", sc.CPU_SCENES)
def test_plain_f64_runs_have_room_under_the_bound_and_the_forms_agree(runs, name):
    """Both forms of the rule in NumPy f64 stay at <= 1/8 of the bound the device is judged by (measured: products 0.004 ...
    0.022, direct 0.0009 ... 0.0032), so they agree under it; the last record's P^s is its P, bit for bit."""
    records, ref, prod, direct = runs[name]
    r_prod, r_dir = sc.worst_record_ratio(prod["Ps"], ref, records), sc.worst_record_ratio(direct["Ps"], ref, records)
    print(f"{name}: products {r_prod:.4f}, direct {r_dir:.4f} of the bound")
    assert r_prod <= 0.125 and r_dir <= 0.125
    b = sc.record_bound(ref, records)
    for r, (p, d) in enumerate(zip(prod["Ps"], direct["Ps"])):
        assert np.abs(p - d).max() <= b[r]
        assert r == len(records) - 1 or np.array_equal(p, p.T)      # (the last one is the oracle filter's own P)
    assert np.array_equal(prod["Ps"][-1], records[-1]["P"])
    assert np.array_equal(ref["Ps"][-1].astype(np.float64), records[-1]["P"])


@pytest.mark.parametrize("name", sc.CPU_SCENES)
def test_smoothing_never_adds_uncertainty_and_stays_positive_definite(runs, name):
    """On the oracle P_r - P^s_r is positive semi-definite to rounding (slack: N times the entry bound, which covers the f64
    eigenvalue routine as well), P^s_r is positive definite (smallest eigenvalue 1.9e-4 or more, far above that slack),
    and no smoothed position variance exceeds the filtered one."""
    records, ref, _prod, _direct = runs[name]
    b = sc.record_bound(ref, records)
    for r, rec in enumerate(records):
        ps = ref["Ps"][r].astype(np.float64)
        gap = np.linalg.eigvalsh(rec["P"] - ps).min()
        assert gap >= -rec["dims"] * b[r], (r, gap)
        assert np.linalg.eigvalsh(ps).min() > rec["dims"] * b[r]
        ratio = np.diag(ps)[:3] / np.diag(rec["P"])[:3]
        assert (ratio > 0.0).all() and (ratio <= 1.0 + 1e-12).all(), (r, ratio)


def test_the_growing_log_tells_smoothed_from_filtered():
    """growing_scene(17, 3): the camera block of record 0 differs from the filtered one by several per cent of its largest
    entry (7.6 % measured), orders of magnitude above the bound: returning the filtered covariance cannot pass."""
    records, _f, _s = su.oracle_records(su.growing_scene(17, 3))
    ref = sc.smooth_cov_records(records)
    assert [r["dims"] for r in records][:4] == [61, 64, 67, 70]
    cam_s, cam_f = ref["Ps"][0][:10, :10].astype(np.float64), records[0]["P"][:10, :10]
    rel = np.abs(cam_s - cam_f).max() / np.abs(cam_f).max()
    assert rel >= 0.05 and np.abs(cam_s - cam_f).max() >= 1e6 * sc.record_bound(ref, records)[0]


def test_many_right_hand_sides_solve_like_the_single_one():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(9, 9))
    a = (a @ a.T + 9 * np.eye(9)).astype(sc.LD)
    b = rng.normal(size=(9, 4)).astype(sc.LD)
    l = sc.cholesky_factor(a)
    x = sc.backward(l, sc.forward(l, b))
    for j in range(4):
        assert np.abs(x[:, j] - su.cholesky_solve(a, b[:, j])).max() <= 1e-17
    with pytest.raises(np.linalg.LinAlgError):
        sc.cholesky_factor(np.array([[1.0, 2.0], [2.0, 1.0]]))


# ---- symbols and the header -------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_refuse_a_null_handle(lib):
    from aruco_slam_amd import _build, hip_backend
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    assert "ekf_smooth_cov.hip" in _build.SOURCES
    block = header[header.index("Smoothed covariances."):header.index("int ekf_observe_log_recorded(")]
    for word in ("The covariance rule", "bitwise symmetric", "BEFORE THE FIRST RECORD", "EKF_ERR_NUMERIC", "8064",
                 "ekf_batch", "resident", "EKF_MODEL_ROTATIONS", "f32 covariance", "per-frame ekf_observe"):
        assert word in block, word
    C = hip_backend.C
    n = C.c_size_t()
    assert lib.ekf_smooth_cov_workspace_bytes(None, C.byref(n)) == -1
    assert lib.ekf_smooth_history_cov(None, None, 0, None, 0, 0, None, None, None, None) == -1
    # the launcher's new argument defaults to what it did before
    kernels = (sw.CSRC / "ekf_kernels.h").read_text()
    assert "hipStream_t s, int64_t xinv_stride = 0);" in kernels


# ---- the Python layer, with a fake back end ---------------------------------------------------------------------------------
def _ekf():
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    flt = EKF.__new__(EKF)
    flt.landmarks, flt.num_landmarks = {}, 0
    return flt


def test_get_cam_estimate_cov_returns_the_row():
    flt = _ekf()
    with pytest.raises(NotImplementedError):
        flt.get_cam_estimate_cov(0)
    flt._smoothed = np.zeros((3, 7))      # (smoothed without cov: still nothing to return)
    flt._smoothed_cov = None
    with pytest.raises(NotImplementedError):
        flt.get_cam_estimate_cov(0)
    flt._smoothed_cov = np.arange(300.0).reshape(3, 10, 10)
    assert np.array_equal(flt.get_cam_estimate_cov(np.int64(1)), np.arange(100.0, 200.0).reshape(10, 10))
    for bad in (-1, 3):
        with pytest.raises(IndexError):
            flt.get_cam_estimate_cov(bad)


def test_python_layer_has_the_covariance_interface():
    """``cov`` is a keyword-only option of ``smooth_detection_log``: the positional arguments are what they were, ``cov=True``
    reaches the replay as the covariance mode, and the refusals still come first."""
    from aruco_slam_amd import hip_backend
    assert callable(hip_backend.HipEkf.smooth_history_cov)
    seen = []

    class _Cfg:
        quat_mode, cov_dtype = 1, 0

    class _Backend:
        cfg, map_frozen = _Cfg(), False

    flt = _ekf()
    flt._hip = _Backend()
    flt._replay_detection_log = lambda *a: seen.append(a) or "out"
    assert flt.smooth_detection_log("i", "p", "o", None, "n", "s", "m", True) == "out"
    assert flt.smooth_detection_log("i", "p", "o", mahal=True, cov=True) == "out"
    assert flt.smooth_detection_log("i", "p", "o", cov=False) == "out"
    assert seen == [("i", "p", "o", None, True, "n", "s", "m", True), ("i", "p", "o", None, True, None, None, None, "cov"),
                    ("i", "p", "o", None, False, None, None, None, True)]
    with pytest.raises(TypeError):      # (keyword-only)
        flt.smooth_detection_log("i", "p", "o", None, None, None, None, False, True)
    _Backend.map_frozen = True
    with pytest.raises(ValueError, match="frozen"):
        flt.smooth_detection_log("i", "p", "o", cov=True)
    assert len(seen) == 3


def test_run_slam_smooth_cov_needs_smooth():
    from aruco_slam_amd.main import run_slam
    parse = run_slam.build_parser().parse_args
    assert parse(["--smooth-cov", "c.npz"]).smooth_cov == "c.npz" and parse([]).smooth_cov is None
    with pytest.raises(ValueError, match="--smooth"):
        run_slam.main(parse(["--smooth-cov", "c.npz", "--detections", "x.npz", "--resident"]))


def test_replay_bench_has_the_cov_mode():
    text = (sw.REPO / "tools" / "replay_bench.py").read_text()
    assert '"--cov"' in text and "smooth_history_cov" in text and "cov_summary.json" in text
