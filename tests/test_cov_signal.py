"""Pipelined sequence mode: the covariance update stores "C(t) complete" itself (csrc/ekf_kernels.h: ekf_cov_arrive) --
its workgroups count themselves on a device counter, the last one re-arms the counter and stores the signal the next
front kernel's end gate waits for.  Every kernel that can signal, at launch shapes with partly empty workgroups, over
short runs with odd and even frame counts and back-to-back calls, must leave BITWISE what the serial order leaves (state,
covariance, trajectory), and the counter must come back armed across handles and after a sticky device error.
Run with ``-m gpu`` on an MI355X."""
import numpy as np
import pytest

import support as sp

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
PIPELINED = "pipelined"

# name: (n, m, cov dtype, cov kernel) -> the kernel that signals and its launch
SHAPES = {
    # N = 70: 3 x 3 tiles of 32, 6 lower tiles, one wave each: two workgroups, the second one half empty
    "f32_tile_odd": (20, 4, "float32", "auto"),
    # the same tiles, one workgroup per tile (ekf_cov_update_mfma_f64_split)
    "f64_split": (20, 4, "float64", "auto"),
    # N = 202: 2 x 2 macro tiles of 128, grid = 8 x the longest per-XCD list: most workgroups have no tile
    "f32_macro": (64, 8, "float32", "mfma_macro"),
    # N = 2110: 66 x 66 tiles of 32, 2211 > 2048 lower tiles: one wave per tile (ekf_cov_update_mfma_f64), 553 workgroups,
    # the last one with three tiles
    "f64_tile": (700, 10, "float64", "auto"),
}


def _ekf(**kw):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    return EKF(INIT, **kw)


def _filter(shape, lookahead, seed):
    """A bootstrapped filter of SHAPES[shape] and the stream it was bootstrapped from."""
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m, dtype, kernel = SHAPES[shape]
    s = SyntheticStream(n, m, seed=seed)
    flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype=dtype, cov_kernel=kernel, lookahead=lookahead)
    for ids, poses in s.bootstrap():
        flt.observe(ids, poses)
    return flt, s


def _resident(frames):
    import torch
    idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda")
    z = torch.tensor(np.stack([f[1][:, :3] for f in frames]), dtype=torch.float64, device="cuda")
    return idx, z


def _run_calls(flt, idx, z, calls, want_mode):
    """Sequence calls of calls[i] frames back to back, no sync() in between; (trajectory, state, covariance)."""
    import torch
    traj = torch.zeros((idx.shape[0], 7), dtype=torch.float64, device="cuda")
    lo = 0
    for count in calls:
        flt.backend.observe_sequence(idx[lo:lo + count], z[lo:lo + count], traj[lo:lo + count])
        assert flt.backend.last_sequence_mode() == want_mode
        lo += count
    flt.backend.sync()
    return traj.cpu().numpy(), flt.state, flt.uncertainty


@pytest.mark.parametrize("frames", [2, 3, 7])
@pytest.mark.parametrize("shape", ["f32_tile_odd", "f64_split", "f32_macro", "f64_tile"])
def test_signalling_update_is_bitwise_the_serial_order(shape, frames):
    """A run of 2, 3 or 7 frames (the last update of a run does not signal: 1, 2 and 6 signalling launches, the covariance
    ending in either buffer), then a second call on the same handle while the first may still be in flight."""
    calls = (frames, 3)
    out = []
    for lookahead in (True, False):
        flt, s = _filter(shape, lookahead, seed=5)
        idx, z = _resident(list(s.steady(sum(calls))))
        out.append(_run_calls(flt, idx, z, calls, PIPELINED if lookahead else "serial"))
    sp.assert_same(out[0], out[1], "trajectory, state, covariance")
    assert np.array_equal(out[0][2], out[0][2].T)


def test_counter_is_armed_again_when_another_handle_takes_the_token_over():
    """Handle A pipelines and is synchronised; handle B (its own workspace, the process's one pipelining token) then
    pipelines and leaves what its serial twin leaves; A once more afterwards."""
    a, sa = _filter("f32_tile_odd", True, seed=6)
    b, sb = _filter("f32_tile_odd", True, seed=7)
    ref_a, _ = _filter("f32_tile_odd", False, seed=6)
    ref_b, _ = _filter("f32_tile_odd", False, seed=7)
    ia, za = _resident(list(sa.steady(8)))
    ib, zb = _resident(list(sb.steady(5)))
    first_a = _run_calls(a, ia[:5], za[:5], (5,), PIPELINED)
    got_b = _run_calls(b, ib, zb, (5,), PIPELINED)
    again_a = _run_calls(a, ia[5:], za[5:], (3,), PIPELINED)
    sp.assert_same(first_a, _run_calls(ref_a, ia[:5], za[:5], (5,), "serial"), "trajectory, state, covariance")
    sp.assert_same(got_b, _run_calls(ref_b, ib, zb, (5,), "serial"), "trajectory, state, covariance")
    sp.assert_same(again_a, _run_calls(ref_a, ia[5:], za[5:], (3,), "serial"), "trajectory, state, covariance")


def test_pipelined_call_after_a_sticky_error_and_reset_is_bitwise_the_serial_order():
    """A pipelined call whose middle frame carries a landmark index beyond the map ends in the sticky EKF_ERR_INVALID (the
    kernels clamp the index and raise the bit; every launch of the run still runs to its end).  After reset() the handle
    pipelines again, equal to a filter that never failed."""
    import torch
    from aruco_slam_amd.hip_backend import EkfError
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m, dtype, kernel = SHAPES["f32_tile_odd"]
    bad, s = _filter("f32_tile_odd", True, seed=8)
    idx, z = _resident(list(s.steady(4)))
    idx = idx.clone()
    idx[1, 2] = 99                                   # beyond the map
    bad.backend.observe_sequence(idx, z)
    assert bad.backend.last_sequence_mode() == PIPELINED
    with pytest.raises(EkfError) as err:
        bad.backend.sync()
    assert err.value.code == -1                      # EKF_ERR_INVALID, reported by the kernels
    torch.cuda.synchronize()
    bad.reset()
    assert bad.num_landmarks == 0
    out = []
    for flt in (bad, _ekf(max_landmarks=n, max_visible=m, cov_dtype=dtype, cov_kernel=kernel, lookahead=False)):
        s2 = SyntheticStream(n, m, seed=9)
        for ids, poses in s2.bootstrap():
            flt.observe(ids, poses)
        i2, z2 = _resident(list(s2.steady(6)))
        out.append(_run_calls(flt, i2, z2, (3, 3), PIPELINED if flt is bad else "serial"))
    sp.assert_same(out[0], out[1], "trajectory, state, covariance")
