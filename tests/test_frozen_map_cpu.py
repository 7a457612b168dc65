"""Localisation mode, the parts that need no GPU: the oracle construction the GPU tests compare with, the C ABI's new
symbols, the host side of ``freeze_map`` (dropped ids, log plans, checkpoints, the app loop's arguments) and the strip
kernel's resource usage."""
import argparse
import inspect
import re
import subprocess

import numpy as np
import pytest

import frozen_util as fu
import support as sp
from conftest import REPO
from support import lib

NEW_SYMBOLS = ("ekf_set_map_frozen", "ekf_get_map_frozen")


# ---- the oracle construction ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n,m_range", [("ekf", 24, (2, 10)), ("ekf_rotations", 12, (1, 5))])
def test_schmidt_step_is_the_joseph_form_schmidt_kalman_update(model, n, m_range):
    """"The oracle's step, then landmark state and P[10:, 10:] back" against the explicit Joseph-form update with the
    landmark rows of the gain zero, over bootstrap + 20 mapping + 100 frozen frames: 1e-12 relative (measured 5e-14); P stays
    positive definite."""
    from aruco_slam_amd.synthetic import ragged_log
    log = ragged_log(n, m_range, 120, seed=21, rvec_sigma=0.05 if model == "ekf_rotations" else 0.0)
    offs, boot = log["offsets"], int(log["bootstrap_frames"])
    orc = fu.new_oracle(model)
    worst, lam = 0.0, np.inf
    for t in range(len(offs) - 1):
        ids = [int(i) for i in log["ids"][offs[t]:offs[t + 1]]]
        poses = log["poses"][offs[t]:offs[t + 1]]
        if t < boot + 20:
            orc.observe(ids, poses)
            continue
        delta, want = fu.joseph_schmidt_step(orc, ids, poses)
        cam0, lm0 = np.array(orc.state[:10], dtype=np.float64), np.array(orc.state[10:], dtype=np.float64)
        fu.schmidt_step(orc, ids, poses)
        got = np.asarray(orc.uncertainty)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
        assert np.array_equal(orc.state[10:], lm0) and not delta[10:].any()
        worst = max(worst, float(np.abs((orc.state[:3] - cam0[:3]) - delta[:3]).max()))
        lam = min(lam, float(np.linalg.eigvalsh(got)[0]))
    print(f"schmidt vs joseph [{model}]: {worst:.2e} relative, smallest eigenvalue {lam:.2e}")
    assert worst <= 1e-12, worst
    assert lam > 0.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported(lib):
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    assert "Localisation mode" in header and "does not accumulate" in header
    # no handle: EKF_ERR_INVALID, nothing touched
    assert lib.ekf_set_map_frozen(None, 1) == -1 and lib.ekf_get_map_frozen(None) == -1


def test_the_frame_argument_grows_at_its_end_only():
    text = (REPO / "aruco_slam_amd" / "csrc" / "ekf_kernels.h").read_text()
    body = text[text.index("struct EkfFrame {"):text.index("// process-noise diagonal of state dimension i as the PREVIOUS")]
    fields = re.findall(r"^\s+(?:const )?[A-Za-z_0-9 ]+[ *]+([a-z_0-9, ]+);", body, flags=re.M)
    assert fields[-2:] == ["qprev_cam, qprev_err, qprev_lm", "frozen"]


# ---- the Python layer --------------------------------------------------------------------------------------------------------
class _Backend:
    """What BaseFilter needs of HipEkf on a frozen map, recording the calls."""
    can_gate = can_row_noise = False
    can_frame_scale = can_motion = True
    gate = None
    rows_per_detection = 3
    pending_scale = 0.0

    def __init__(self):
        self.map_frozen, self.calls = False, []

    def set_map_frozen(self, frozen):
        self.map_frozen = bool(frozen)

    def observe(self, index, z, rows=None, scale=None):
        self.calls.append(("observe", list(index), np.array(z), scale))

    def move(self, u):
        self.calls.append(("move", np.array(u)))

    def advance(self, scale):
        self.calls.append(("advance", scale))

    def add_markers(self, *a):
        self.calls.append(("add_markers",))

    def reset(self, pose):
        self.map_frozen = False      # (ekf_reset clears the flag)
        self.calls.append(("reset",))


def _stub_ekf():
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    flt = EKF.__new__(EKF)
    flt._hip = _Backend()
    flt._initial_pose = np.zeros(10)
    flt.landmarks, flt.num_landmarks = {7: 0, 9: 1, 4: 2}, 3
    flt.last_mahal = flt.last_rejected = None
    return flt


def test_frozen_observe_drops_unknown_ids_and_reports_them():
    flt = _stub_ekf()
    assert not flt.map_frozen and flt.last_ignored == ()
    flt.freeze_map()
    assert flt.map_frozen
    poses = np.arange(30.0).reshape(5, 6)
    flt.observe([9, 33, 7, 21, 9], poses)
    assert flt.last_ignored == (33, 21) and flt.landmarks == {7: 0, 9: 1, 4: 2} and flt.num_landmarks == 3
    (kind, index, z, scale), = flt.backend.calls
    assert kind == "observe" and index == [1, 0, 1] and scale is None
    assert np.array_equal(z, poses[[0, 2, 4], 0:3])
    # nothing known: the frame is not stepped; it is still moved and its scale goes to the pending scale
    flt.backend.calls.clear()
    flt.observe([33], poses[:1], scale=2.0, motion=[0.1, 0, 0, 0, 0, 0])
    assert [c[0] for c in flt.backend.calls] == ["move", "advance"] and flt.backend.calls[1][1] == 2.0
    assert flt.last_ignored == (33,)
    # all known: nothing is reported
    flt.observe([4], poses[:1])
    assert flt.last_ignored == ()
    # unfrozen: unknown ids are first sightings again
    flt.unfreeze_map()
    flt.backend.calls.clear()
    flt.observe([33], poses[:1])
    assert flt.backend.calls[0] == ("add_markers",) and flt.landmarks[33] == 3 and flt.last_ignored == ()


def test_reset_clears_the_flag():
    flt = _stub_ekf()
    flt.freeze_map()
    flt.observe([33], np.zeros((1, 6)))
    assert flt.map_frozen and flt.last_ignored == (33,)
    flt.reset()
    assert not flt.map_frozen and flt.last_ignored == () and flt.landmarks == {}


def test_plan_detection_log_drops_unknown_ids_on_a_frozen_map():
    from aruco_slam_amd.filters.base_filter import plan_detection_log
    known = {7: 0, 9: 1, 4: 2}
    ids = np.array([9, 33, 7, 33, 21, 4, 4, 50])
    offsets = np.array([0, 3, 5, 5, 7, 8])
    has = np.array([True, True, False, True, True])
    plan = plan_detection_log(known, 3, ids, offsets, has, frozen=True)
    assert plan.keep.tolist() == [True, False, True, False, False, True, True, False]
    assert plan.ignored == (33, 33, 21, 50) and plan.new_landmarks == {} and plan.num_landmarks == 3
    assert plan.index.tolist() == [1, 0, 2, 2] and plan.offsets.tolist() == [0, 2, 2, 2, 4, 4] and plan.widest == 2
    assert known == {7: 0, 9: 1, 4: 2}
    # not frozen: the plan it always was, and nothing is reported
    plan = plan_detection_log(known, 3, ids, offsets, has)
    assert plan.ignored == () and plan.new_landmarks == {33: 3, 21: 4, 50: 5} and plan.keep.all()
    assert inspect.signature(plan_detection_log).parameters["frozen"].default is False


def test_python_layer_has_the_localisation_mode():
    from aruco_slam_amd import hip_backend
    from aruco_slam_amd.filters.base_filter import BaseFilter
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    for cls in (EKF, EKF_Rotations):
        assert cls.freeze_map is BaseFilter.freeze_map and cls.unfreeze_map is BaseFilter.unfreeze_map
        assert isinstance(inspect.getattr_static(cls, "map_frozen"), property)
    assert inspect.signature(EKF.__init__).parameters["localize"].default is False
    assert isinstance(inspect.getattr_static(hip_backend.HipEkf, "map_frozen"), property)
    assert list(inspect.signature(hip_backend.HipEkf.set_map_frozen).parameters) == ["self", "frozen"]
    with pytest.raises(ValueError, match="map_file"):
        EKF(np.zeros(10), localize=True)


class _CheckpointBackend(_Backend):
    def get_state(self):
        return self.state

    def get_cov(self):
        return self.cov

    def set_state_cov(self, state, cov):
        self.state, self.cov = np.array(state), np.array(cov)


def _checkpoint_filter():
    flt = _stub_ekf()
    flt._hip = _CheckpointBackend()
    flt._hip.can_frame_scale = flt._hip.can_motion = False
    flt._hip.state, flt._hip.cov = np.arange(19.0), np.eye(19)
    return flt


def test_checkpoint_carries_the_flag_and_an_old_one_loads_unfrozen(tmp_path):
    a = _checkpoint_filter()
    a.freeze_map()
    a.save_checkpoint(str(tmp_path / "frozen.npz"))
    assert bool(np.load(tmp_path / "frozen.npz")["map_frozen"])
    b = _checkpoint_filter()
    b.load_checkpoint(str(tmp_path / "frozen.npz"))
    assert b.map_frozen and b.landmarks == a.landmarks
    # a checkpoint from before the flag: not frozen, also into a filter that was
    with np.load(tmp_path / "frozen.npz") as ck:
        np.savez(tmp_path / "old.npz", **{k: ck[k] for k in ck.files if k != "map_frozen"})
    b.load_checkpoint(str(tmp_path / "old.npz"))
    assert not b.map_frozen
    a.unfreeze_map()
    a.save_checkpoint(str(tmp_path / "mapping.npz"))
    b.freeze_map()
    b.load_checkpoint(str(tmp_path / "mapping.npz"))
    assert not b.map_frozen


# ---- the app loop and the tools ---------------------------------------------------------------------------------------------
def test_run_slam_localize_needs_a_map():
    from aruco_slam_amd.main import run_slam
    args = run_slam.build_parser().parse_args(["--localize", "--detections", "x.npz"])
    assert args.localize and args.map is None
    with pytest.raises(ValueError, match="--map"):
        run_slam.main(args)
    args = run_slam.build_parser().parse_args(["--map", "m.txt", "--localize"])
    assert args.map == "m.txt" and not run_slam.build_parser().parse_args([]).localize
    # a Namespace from before the two arguments still runs into the old checks, not into an AttributeError
    with pytest.raises(ValueError, match="Unknown filter type"):
        run_slam.main(argparse.Namespace(video="v.mp4", filter="nope", detections=None, resident=True))


def test_replay_bench_has_the_frozen_mode():
    text = (REPO / "tools" / "replay_bench.py").read_text()
    assert '"--frozen"' in text and "freeze_map()" in text and "lookahead=False" in text


# ---- the strip kernel --------------------------------------------------------------------------------------------------------
def test_strip_kernel_resource_usage(tmp_path):
    """ekf_cov_strip_kernel<float / double> and the f32 instance with the VALU reference kernel's chain step: no scratch, the LDS copy of W[:, 0:10] for at most 384 rows (12 elements per
    row), and registers for at least 4 waves per SIMD (a launch has few waves; the budget keeps two blocks of 16 loads in
    flight without spilling)."""
    from aruco_slam_amd import _build
    out = tmp_path / "strip.s"
    subprocess.run([_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    str(_build.CSRC / "ekf_cov_strip.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()

    # one metadata entry per kernel, "  - .agpr_count: ..." first (the keys are sorted: some lie in front of .name)
    entries = re.split(r"\n  - (?=\.agpr_count:)", text[text.index("amdhsa.kernels:"):])[1:]

    def field(kernel, name):
        entry, = [e for e in entries if re.search(rf"\.name:\s+{kernel}\n", e)]
        return int(re.search(rf"\.{name}:\s+(\d+)", entry).group(1))

    names = re.findall(r"^(_Z20ekf_cov_strip_kernel\S+):", text, flags=re.M)
    f32, f32_valu, f64 = (f"_Z20ekf_cov_strip_kernelI{t}EEv8EkfFrame" for t in ("fLb0", "fLb1", "dLb0"))
    assert sorted(names) == sorted((f32, f32_valu, f64))      # (no instance that no launcher dispatches)
    for kernel, elem in ((f32, 4), (f32_valu, 4), (f64, 8)):
        assert field(kernel, "private_segment_fixed_size") == 0
        assert field(kernel, "vgpr_spill_count") == 0 and field(kernel, "sgpr_spill_count") == 0
        assert field(kernel, "group_segment_fixed_size") == 384 * 12 * elem
        assert field(kernel, "vgpr_count") + field(kernel, "agpr_count") <= 128      # 4 waves per SIMD of 512 registers
        assert field(kernel, "max_flat_workgroup_size") == 256
    # the chain step: a single-rounding fma in the covariance dtype (f32: packed or scalar fma, never through f64); the
    # VALU-step instance: the f64 fma of the widened operands, rounded to f32 (what ekf_cov_update_valu<float> runs)
    def body(kernel):
        start = text.index(kernel + ":")
        return text[start:text.index("s_endpgm", start)]

    assert re.search(r"v_(pk_)?fma(c)?_f32", body(f32)) and not re.search(r"v_fma(c)?_f64", body(f32))
    assert re.search(r"v_fma(c)?_f64", body(f32_valu)) and "v_cvt_f32_f64" in body(f32_valu)
    assert not re.search(r"v_(pk_)?fma(c)?_f32", body(f32_valu))
