"""Localisation mode of ``EKFBatch``, the parts that need no GPU: the two new C ABI symbols, the kernel argument that grows at
its end only, the Python layer on a stub library (``freeze_map`` / ``unfreeze_map`` / ``map_frozen``, ``reset``, the planning of
a frozen member's log, the replica calls' refusal of mixed flags), ``tools/batch_bench.py --frozen``, the ragged logs the GPU
tests share, and the resource usage of the twelve FROZEN kernel instances from the compiler's remarks."""
import ctypes
import re
import subprocess
import sys

import numpy as np
import pytest

import batch_frozen_util as bu
import support as sp
from conftest import GOLDEN, REPO
from support import lib

NEW_SYMBOLS = ("ekf_batch_set_map_frozen", "ekf_batch_get_map_frozen")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported(lib):
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    assert "Localisation mode of a batch" in header and "(single filter)" not in header
    # no handle: EKF_ERR_INVALID, nothing touched
    out = np.zeros(4, np.int32)
    ip = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.ekf_batch_set_map_frozen(None, ip) == -1 and lib.ekf_batch_get_map_frozen(None, ip) == -1


def test_the_window_argument_grows_at_its_end_only():
    text = (REPO / "aruco_slam_amd" / "csrc" / "ekf_kernels.h").read_text()
    body = text[text.index("struct EkfBatchWindow {"):text.index("// dynamic LDS of one launch")]
    fields = re.findall(r"^\s+(?:const )?[A-Za-z_0-9]+[ *]+([a-z_A-Z0-9, ]+);", body, flags=re.M)
    assert fields == ["P", "ld", "state", "noise", "status", "nlm", "lm_index", "frame_offsets", "member_frames", "poses", "traj",
                      "nis", "cam_cov", "quat_mode", "window_first, window_frames", "kmax, lda", "gate", "mahal", "row_noise",
                      "pending", "scale", "motion", "frozen"]
    assert "const int32_t* frozen;" in body


def test_the_build_compiles_the_frozen_instances_in_their_own_files():
    from aruco_slam_amd import _build
    assert {"ekf_batch_frozen.hip", "ekf_batch_wide_frozen.hip"} <= set(_build.SOURCES)
    frozen = (_build.CSRC / "ekf_batch_frozen.hip").read_text() + (_build.CSRC / "ekf_batch_wide.hip").read_text()
    assert len(re.findall(r"ekf_batch_window<[01], (?:true|false), true>", frozen)) == 4
    assert len(re.findall(r"^EKF_WIDE_FROZEN_KERNEL\(", frozen, flags=re.M)) == 8


# ---- the Python layer on a stub library ---------------------------------------------------------------------------------------
class _StubLib:
    """What EKFBatch asks of the library around the frozen flags, recording the calls."""

    def __init__(self, members, counts):
        self.flags, self.counts, self.calls = np.zeros(members, np.int32), np.asarray(counts, np.int32), []

    def ekf_batch_get_map_frozen(self, h, out):
        for i, v in enumerate(self.flags):
            out[i] = int(v)
        return 0

    def ekf_batch_set_map_frozen(self, h, flags):
        self.flags = np.array([flags[i] for i in range(len(self.flags))], np.int32)
        self.calls.append(("set_map_frozen", self.flags.tolist()))
        return 0

    def ekf_batch_reset(self, h, member, poses):
        self.calls.append(("reset", member))
        if member < 0:
            self.flags[:] = 0
            self.counts[:] = 0
        else:
            self.flags[member] = 0
            self.counts[member] = 0
        return 0

    def ekf_batch_num_landmarks(self, h, out):
        for i, v in enumerate(self.counts):
            out[i] = int(v)
        return 0

    def ekf_last_error_string(self):
        return b""


def _stub_batch(members=4):
    from aruco_slam_amd.batch import EKFBatch
    b = EKFBatch.__new__(EKFBatch)
    b.members, b.model, b.lm_dims = members, "ekf", 3
    b.row_noise = b.frame_scale = b.motion = False
    b.gate = b.camera = None
    b.lib, b.h = _StubLib(members, [3] * members), ctypes.c_void_p(1)
    b.landmarks = [{7: 0, 9: 1, 4: 2} for _ in range(members)]
    b.num_landmarks = [3] * members
    b.last_ignored = [()] * members
    b._initial_poses = np.tile(bu.INIT, (members, 1))
    b.seen = []

    def observe_indexed(index, offsets, frames, poses, **kw):
        b.seen.append((np.array(index), np.array(offsets), np.array(frames), np.array(poses)))
        return np.zeros((int(frames[-1]), 7))
    b.observe_indexed = observe_indexed
    return b


def test_freeze_unfreeze_and_the_flag_array():
    b = _stub_batch()
    assert b.map_frozen.dtype == bool and b.map_frozen.tolist() == [False] * 4
    b.freeze_map(2)
    assert b.map_frozen.tolist() == [False, False, True, False]
    b.freeze_map()
    assert b.map_frozen.all()
    b.unfreeze_map(0)
    assert b.map_frozen.tolist() == [False, True, True, True]
    b.unfreeze_map()
    assert not b.map_frozen.any()
    assert [c[1] for c in b.lib.calls] == [[0, 0, 1, 0], [1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0]]
    with pytest.raises(IndexError):
        b.freeze_map(4)


def test_reset_clears_the_flag_of_the_members_it_resets():
    b = _stub_batch()
    b.freeze_map()
    b.last_ignored = [(33,)] * 4
    b.reset(1)
    assert b.map_frozen.tolist() == [True, False, True, True] and b.last_ignored == [(33,), (), (33,), (33,)]
    assert b.landmarks[1] == {} and b.num_landmarks == [3, 0, 3, 3]
    b.reset()
    assert not b.map_frozen.any() and b.last_ignored == [()] * 4


def test_a_frozen_members_log_drops_unknown_ids_and_reports_them():
    b = _stub_batch()
    b.freeze_map(1)
    b.freeze_map(3)
    log = {"ids": np.array([9, 33, 7, 21, 4]), "poses": np.arange(30.0).reshape(5, 6), "offsets": np.array([0, 3, 4, 5])}
    b.lib.counts[:] = [5, 3, 5, 3]      # (what the device reports: the mapping members added 33 and 21)
    b.process_detection_logs([log, log, log, None])
    assert b.last_ignored == [(), (33, 21), (), ()]
    index, offsets, frames, poses = b.seen[0]
    # mapping members: five rows, two first sightings; the frozen member: rows 0, 2 and 4, and frame 1 left with nothing
    assert index.tolist() == [1, 3, 0, 4, 2] + [1, 0, 2] + [1, 3, 0, 4, 2]
    assert offsets.tolist() == [0, 3, 4, 5, 7, 7, 8, 11, 12, 13] and frames.tolist() == [0, 3, 6, 9, 9]
    assert np.array_equal(poses[5:8], log["poses"][[0, 2, 4]])
    assert b.landmarks[1] == {7: 0, 9: 1, 4: 2} and b.landmarks[0] == {7: 0, 9: 1, 4: 2, 33: 3, 21: 4}
    assert b.num_landmarks == [5, 3, 5, 3]


def test_replica_calls_refuse_mixed_flags_and_plan_frozen():
    b = _stub_batch()
    log = {"ids": np.array([9, 33, 7]), "poses": np.zeros((3, 6)), "corners": np.zeros((3, 4, 2)), "offsets": np.array([0, 3])}
    b.freeze_map(2)
    with pytest.raises(ValueError, match="frozen"):
        b.replay_replicas(log, 0.01, 1)
    b.camera = (np.eye(3).reshape(9), np.zeros(0), 0.16)
    with pytest.raises(ValueError, match="frozen"):
        b.replay_corner_replicas({k: v for k, v in log.items() if k != "poses"}, 0.5, 1)
    b.freeze_map()
    plan, poses, idx, fo = b._plan_replica_log(log, "poses", (6,), "replay_replicas")
    assert plan.ignored == (33,) and idx.tolist() == [1, 0] and fo.tolist() == [0, 2] and poses.shape == (2, 6)
    b.unfreeze_map()
    plan, _p, idx, _f = b._plan_replica_log(log, "poses", (6,), "replay_replicas")
    assert plan.ignored == () and idx.tolist() == [1, 3, 0]


def test_python_layer_has_the_batch_localisation_mode():
    import inspect
    from aruco_slam_amd.batch import EKFBatch
    assert isinstance(inspect.getattr_static(EKFBatch, "map_frozen"), property)
    for name in ("freeze_map", "unfreeze_map"):
        assert list(inspect.signature(getattr(EKFBatch, name)).parameters) == ["self", "b"]
        assert inspect.signature(getattr(EKFBatch, name)).parameters["b"].default is None
    assert "last_ignored" in EKFBatch.process_detection_logs.__doc__
    assert "map_frozen" in EKFBatch.load_filter.__doc__ and "map_frozen" in EKFBatch.to_filter.__doc__


# ---- the tools and the shared inputs ---------------------------------------------------------------------------------------------
def test_batch_bench_has_the_frozen_mode():
    text = (REPO / "tools" / "batch_bench.py").read_text()
    assert '"--frozen"' in text and "freeze_map()" in text and "set_member" in text and "frozen_frames_per_s" in text
    done = subprocess.run([sys.executable, str(REPO / "tools" / "batch_bench.py"), "--help"], capture_output=True, text=True, check=True)
    assert "--frozen" in done.stdout


def test_ragged_logs_map_everything_before_the_freeze():
    plan = bu.ragged_plan()
    assert len(plan) == 60 and plan[0] == [] and plan[20] == [] and plan[30:33] == [[], [], []] and plan[25] == [4, 1, 4]
    assert set().union(*plan[:bu.MAP_FRAMES]) == set(range(8))
    for model in bu.MODELS:
        logs = bu.ragged_logs(model)
        assert len(logs) == bu.MEMBERS and all(log["motion"].shape == (60, 6) for log in logs)
        assert not np.array_equal(logs[0]["poses"], logs[1]["poses"])
        head = bu.part(logs[0], 0, bu.MAP_FRAMES)
        assert len(set(head["ids"].tolist())) == 8 and head["offsets"][0] == 0 and len(head["offsets"]) == 21


def test_the_parent_golden_is_small_and_complete():
    path = GOLDEN / "batch_frozen_parent.npz"
    assert path.stat().st_size < (GOLDEN / "frozen_c1_parent.npz").stat().st_size * 2 // 3
    with np.load(path, allow_pickle=False) as g:
        assert sorted(g.files) == sorted(bu.parent_key(m, mv, n) for m in bu.MODELS for mv in (False, True)
                                         for n in ("traj", "nis", "state", "cov"))
        assert g["ekf_plain_traj"].shape == (4, 60, 7) and g["ekf_rotations_moved_cov"].shape == (90, 90)
        assert all(np.isfinite(g[k]).all() for k in g.files)


# ---- resource usage of the FROZEN instances ------------------------------------------------------------------------------------
# kernel -> (VGPRs, AGPRs) of the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950): upper bounds.  Every
# instance: no scratch, no static LDS (the dynamic LDS is the unfrozen sibling's: the strip stages into the R region).
ONE_COLUMN = {"ekf_batch_frozen_window_kernel": (167, 0), "ekf_batch_frozen_rot_window_kernel": (242, 0),
              "ekf_batch_frozen_moved_window_kernel": (256, 176), "ekf_batch_frozen_moved_rot_window_kernel": (256, 180)}
WIDE = {"ekf_batch_frozen_wide_window_kernel": (256, 84), "ekf_batch_frozen_wide_rot_window_kernel": (256, 120),
        "ekf_batch_frozen_one_block_window_kernel": (252, 0), "ekf_batch_frozen_one_block_rot_window_kernel": (256, 8),
        "ekf_batch_frozen_moved_wide_window_kernel": (256, 202), "ekf_batch_frozen_moved_wide_rot_window_kernel": (256, 204),
        "ekf_batch_frozen_moved_one_block_window_kernel": (256, 184),
        "ekf_batch_frozen_moved_one_block_rot_window_kernel": (256, 184)}


def _remarks(src):
    from aruco_slam_amd import _build
    done = subprocess.run([_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                           "-Rpass-analysis=kernel-resource-usage", str(_build.CSRC / src), "-o", "/dev/null"],
                          check=True, capture_output=True, text=True)
    out = {}
    for blk in re.split(r"remark: Function Name: ", done.stderr)[1:]:
        mangled = blk.split()[0]
        name = re.match(r"_Z\d+([a-z_0-9]+?)\d+EkfBatch", mangled).group(1)

        def num(key):
            return int(re.search(key + r": (\d+)", blk).group(1))
        out[name] = {"vgpr": num("VGPRs"), "agpr": num("AGPRs"), "scratch": num(r"ScratchSize \[bytes/lane\]"),
                     "lds": num(r"LDS Size \[bytes/block\]"), "occupancy": num(r"Occupancy \[waves/SIMD\]")}
    return out


@pytest.mark.parametrize("src,pins", [("ekf_batch_frozen.hip", ONE_COLUMN), ("ekf_batch_wide_frozen.hip", WIDE)])
def test_frozen_kernel_resource_usage(src, pins):
    """Every FROZEN instance, and no other kernel, is in its translation unit; none uses scratch or static LDS; registers stay
    within the recorded remarks (the workgroup's dynamic LDS admits one workgroup per CU anyway, so an occupancy of one wave
    per SIMD is what every instance runs at)."""
    got = _remarks(src)
    assert sorted(got) == sorted(pins)
    for name, (vgpr, agpr) in pins.items():
        r = got[name]
        assert r["scratch"] == 0 and r["lds"] == 0, (name, r)
        assert r["vgpr"] <= vgpr and r["agpr"] <= agpr and r["occupancy"] >= 1, (name, r)
