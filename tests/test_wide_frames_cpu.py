"""Wide frames (ekf_config.flags bit 3, EKF_FLAG_WIDE_FRAMES) without a GPU: the configuration check and sizes of the C ABI,
and the register budget of the wide-frame kernels (ekf_wide.hip)."""
import ctypes
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def lib():
    from aruco_slam_amd import _build, hip_backend
    _build.build()
    return hip_backend.load_library()


def _sizes(lib, model, m, flags, n=100):
    from aruco_slam_amd.hip_backend import EkfConfig
    cfg = EkfConfig()
    lib.ekf_default_config(ctypes.byref(cfg))
    cfg.max_landmarks, cfg.max_visible, cfg.model, cfg.flags = n, m, model, flags
    ld, cb, sb, wb = ctypes.c_int64(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib.ekf_query_sizes(ctypes.byref(cfg), ctypes.byref(ld), ctypes.byref(cb), ctypes.byref(sb), ctypes.byref(wb))
    return rc, wb.value


@pytest.mark.parametrize("model,ok,cap", [(0, (65, 300, 1024), 64), (1, (51, 1024), 50)])
def test_wide_flag_admits_up_to_1024_detections(lib, model, ok, cap):
    from aruco_slam_amd.hip_backend import EKF_FLAG_WIDE_FRAMES
    assert EKF_FLAG_WIDE_FRAMES == 8
    for m in ok:
        rc, _ = _sizes(lib, model, m, EKF_FLAG_WIDE_FRAMES)
        assert rc == 0, (m, lib.ekf_last_error_string())
    rc, _ = _sizes(lib, model, 1025, EKF_FLAG_WIDE_FRAMES)
    assert rc == -1 and b"max_visible" in lib.ekf_last_error_string()
    # without bit 3: the caps of the stage kernels, as before
    assert _sizes(lib, model, cap, 0)[0] == 0
    rc, _ = _sizes(lib, model, cap + 1, 0)
    assert rc == -1 and b"max_visible" in lib.ekf_last_error_string()
    # the workspace never shrinks as max_visible grows, and within the caps bit 3 changes no size
    sizes = [_sizes(lib, model, m, EKF_FLAG_WIDE_FRAMES)[1] for m in (1, 16, cap, cap + 1, 128, 300, 1024)]
    assert sizes == sorted(sizes)
    for m in (1, 16, cap):
        assert _sizes(lib, model, m, EKF_FLAG_WIDE_FRAMES)[1] == _sizes(lib, model, m, 0)[1]


def test_wide_kernels_do_not_spill(tmp_path):
    """No scratch memory and no spills in any kernel of the wide-frame translation unit."""
    from aruco_slam_amd import _build
    out = tmp_path / "wide.s"
    subprocess.run([_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    str(_build.CSRC / "ekf_wide.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    spills = re.findall(r"\.name:\s+(\S*ekf_wide_\S*)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text)
    scratch = re.findall(r"\.name:\s+(\S*ekf_wide_\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    names = {n for n, _ in spills}
    for kind in ("measure", "amat", "s_kernel", "potrf", "panel", "update", "finish"):
        assert any(kind in n for n in names), kind
    assert len(spills) >= 15 and all(int(v) == 0 for _, v in spills), spills
    assert len(scratch) == len(spills) and all(int(v) == 0 for _, v in scratch), scratch
