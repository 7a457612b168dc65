"""Wide frames (ekf_config.flags bit 3, EKF_FLAG_WIDE_FRAMES) without a GPU: the configuration check and sizes of the C ABI,
and the register budget of the wide-frame kernels (ekf_wide.hip)."""
import pytest

import support as sp
from support import lib


def _sizes(lib, model, m, flags, n=100):
    rc, _ld, _cov, _state, ws = sp.query_sizes(lib, max_landmarks=n, max_visible=m, model=model, flags=flags)
    return rc, ws


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


def test_wide_kernels_do_not_spill():
    """No scratch memory and no spills in any kernel of the wide-frame translation unit."""
    found = sp.kernel_resources("ekf_wide.hip", r"ekf_wide_")
    for kind in ("measure", "amat", "s_kernel", "potrf", "panel", "update", "finish"):
        assert any(kind in n for n in found), kind
    assert len(found) >= 15, sorted(found)
    for name, res in found.items():
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (name, res)
