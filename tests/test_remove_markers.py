"""Landmark removal on the device (``ekf_remove_markers``, ``ekf_batch_remove_markers``; semantics in
``include/ekf_slam_hip.h``).  The yardstick is the restore path that existed before it (``remove_util.twin_of``): state and
P read back, rows and columns deleted with ``np.delete`` on the host, a fresh filter of the same configuration restored with
``set_state_cov``; the two filters are compared with ``np.array_equal``, the raw device tensors with their capacity padding
included."""
import ctypes as C

import numpy as np
import pytest

import remove_util as ru
from conftest import rel_err

pytestmark = pytest.mark.gpu

MODELS = ("ekf", "ekf_rotations")
DTYPES = ("float64", "float32")
STEP_TOL_F64 = 1e-10      # one f64 step against the oracle: test_hip_parity.STEP_TOL["float64"]


def _traj_frames(flt, frames):
    out = []
    for ids, poses in frames:
        _, cam, _, _ = flt.process_detections(np.asarray(ids), poses)
        out.append(np.array(cam[:7], dtype=np.float64))
    return np.stack(out)


# ---- bit rule and padding -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("removed", [(2,), (0,), (4,), (0, 4), (3, 1), (0, 1, 2, 3, 4)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_removal_is_the_host_deletion_bit_for_bit_and_pads_with_zeros(model, dtype, removed):
    flt, _scene = ru.dense_filter(model, 5, 3, cov_dtype=dtype)
    dense = np.count_nonzero(flt.backend.get_cov())      # (P is dense: EKF_Rotations' landmark error states stay uncoupled)
    assert dense == flt.backend.dims ** 2 if model == "ekf" else dense >= flt.backend.dims ** 2 // 2
    twin = ru.twin_of(model, flt, removed)
    ru.remove_into_nan(flt, removed)
    assert flt.num_landmarks == 5 - len(removed) == flt.backend.num_landmarks
    assert list(flt.landmarks) == [k for k in range(5) if k not in removed]
    assert list(flt.landmarks.values()) == list(range(5 - len(removed)))
    ru.assert_zero_padding(flt)
    ru.assert_same(flt, twin)
    # the boundary getters follow
    cam, lms = flt.get_poses()
    assert cam.shape == (10,) and lms.shape == (5 - len(removed), ru.LMD[model])
    assert np.array_equal(flt.get_lm_uncertainties(), twin.get_lm_uncertainties())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model,n,m,removals", [
    ("ekf", 82, 16, ((40,), tuple(range(1, 82, 2)) + (0, 80))),          # N = 256 = cap -> N' = 253, N' = 127
    ("ekf_rotations", 63, 8, ((0,), (62,))),                             # N = 640 = cap
])
def test_removal_from_a_filter_filled_to_capacity(model, n, m, removals, dtype):
    for removed in removals:
        flt, _scene = ru.dense_filter(model, n, m, steady=2, cov_dtype=dtype)
        assert flt.backend.dims == flt.backend.ld
        twin = ru.twin_of(model, flt, removed)
        ru.remove_into_nan(flt, removed)
        assert flt.backend.dims == flt.backend.ld - ru.LMD[model] * len(removed)
        ru.assert_zero_padding(flt)
        ru.assert_same(flt, twin)
    assert flt.backend.dims == (127 if model == "ekf" else 630)


# ---- continuation ---------------------------------------------------------------------------------------------------------
def test_every_kind_of_call_continues_as_on_the_twin_ekf_f32():
    import torch
    n, m, removed = 40, 8, (5, 17, 39)
    flt, scene = ru.dense_filter("ekf", n, m, cov_dtype="float32", lookahead=True)
    twin = ru.twin_of("ekf", flt, removed, lookahead=True)
    flt.remove_markers(removed)
    ru.assert_same(flt, twin)
    kept = [k for k in range(n) if k not in removed]
    # 12 per-frame observe calls
    frames = scene.frames(12, kept)
    assert np.array_equal(_traj_frames(flt, frames), _traj_frames(twin, frames))
    ru.assert_same(flt, twin)
    # a 12-frame observe_sequence, pipelined where the process allows it (one handle at a time: first one, then the other)
    frames = scene.frames(12, kept)
    trajs = []
    for f in (flt, twin):
        be = f.backend
        idx = torch.tensor([[f.landmarks[k] for k in ids] for ids, _ in frames], dtype=torch.int32, device=be.device)
        z = torch.tensor(np.stack([p[:, :3] for _, p in frames]), dtype=torch.float64, device=be.device)
        traj = torch.empty((12, 7), dtype=torch.float64, device=be.device)
        torch.cuda.synchronize(be.device)
        be.observe_sequence(idx, z, traj)
        be.sync()
        trajs.append(traj.cpu().numpy())
    assert np.array_equal(trajs[0], trajs[1])
    ru.assert_same(flt, twin)
    # a log that sees a removed id again: a first sighting, the new landmark is the last one
    log = ru.as_log(scene.frames(3, kept) + [scene.frame(sorted(kept[:7] + [17]))] + scene.frames(4, kept + [17]))
    ta = flt.process_detection_log(log["ids"], log["poses"], log["offsets"])
    tb = twin.process_detection_log(log["ids"], log["poses"], log["offsets"])
    assert np.array_equal(ta, tb)
    assert flt.landmarks[17] == n - len(removed) == flt.num_landmarks - 1
    ru.assert_same(flt, twin)


def test_per_frame_calls_continue_as_on_the_twin_rotations_f64():
    n, m, removed = 12, 4, (0, 6, 11)
    flt, scene = ru.dense_filter("ekf_rotations", n, m, cov_dtype="float64")
    twin = ru.twin_of("ekf_rotations", flt, removed)
    flt.remove_markers(removed)
    kept = [k for k in range(n) if k not in removed]
    frames = scene.frames(6, kept) + [scene.frame([1, 2, 6, 3])] + scene.frames(5, kept + [6])
    assert np.array_equal(_traj_frames(flt, frames), _traj_frames(twin, frames))
    assert flt.landmarks[6] == n - len(removed) == flt.num_landmarks - 1
    ru.assert_same(flt, twin)


# ---- against the oracle, independent of the restore path ------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_removal_against_the_numpy_oracle(model):
    """The oracle runs a log; the filter is restored from it, removes on the device while the oracle's arrays lose the same
    rows and columns on the host; five more frames on both."""
    from oracle.ekf_numpy import OracleEKF, OracleEKFRotations
    n, m, removed = 10, 4, (7, 2, 3)
    scene = ru.Scene(model, n, m, seed=3)
    orc = OracleEKFRotations(ru.INIT, mode="fast") if model == "ekf_rotations" else \
        OracleEKF(ru.INIT, mode="fast", quat_mode="scalar_first")
    for ids, poses in scene.bootstrap() + scene.frames(5, np.arange(n)):
        orc.observe(ids, poses)
    flt = ru.make_filter(model, max_landmarks=n, max_visible=m, cov_dtype="float64")
    flt.backend.set_state_cov(np.asarray(orc.state, dtype=np.float64), orc.uncertainty)
    flt.landmarks, flt.num_landmarks = dict(orc.landmarks), orc.num_landmarks
    flt.remove_markers(removed)
    index = [orc.landmarks[k] for k in removed]
    orc.state, orc.uncertainty = ru.deleted(model, np.asarray(orc.state, dtype=np.float64), np.asarray(orc.uncertainty), index)
    kept = [k for k in range(n) if k not in removed]
    orc.landmarks = {k: i for i, k in enumerate(kept)}
    orc.num_landmarks = len(kept)
    assert flt.landmarks == orc.landmarks
    for ids, poses in scene.frames(5, kept):
        orc.observe(ids, poses)
        flt.observe(ids, poses)
    es, ep = rel_err(flt.state, orc.state), rel_err(flt.uncertainty, orc.uncertainty)
    print(f"oracle[{model}]: state {es:.3e} cov {ep:.3e}")
    assert es <= STEP_TOL_F64 and ep <= STEP_TOL_F64, (es, ep)


# ---- one large shape ------------------------------------------------------------------------------------------------------
def test_removal_at_n1024_f32():
    n, m, removed = 1024, 32, (3, 517, 1023)
    flt, _scene = ru.dense_filter("ekf", n, m, steady=2, cov_dtype="float32")
    twin = ru.twin_of("ekf", flt, removed)
    ru.remove_into_nan(flt, removed)
    assert flt.backend.dims == 3 * 1021 + 10
    ru.assert_zero_padding(flt)
    ru.assert_same(flt, twin)


# ---- gate interplay -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_gated_frame_after_a_removal_is_the_twins(model):
    n, m, removed = 8, 4, (1, 6)
    flt, scene = ru.dense_filter(model, n, m, cov_dtype="float64", gate=ru.GATES[model])
    twin = ru.twin_of(model, flt, removed, gate=ru.GATES[model])
    flt.remove_markers(removed)
    assert flt.gate == ru.GATES[model]
    ids, poses = scene.frame([0, 2, 3, 7])
    poses = poses.copy()
    poses[2, :3] += 150.0                               # a gross outlier
    for f in (flt, twin):
        f.observe(ids, poses)
    assert flt.last_rejected.tolist() == [False, False, True, False]
    assert np.array_equal(flt.last_mahal, twin.last_mahal) and np.array_equal(flt.last_rejected, twin.last_rejected)
    assert flt.backend.last_gate_stats() == twin.backend.last_gate_stats() == {"tested": 4, "rejected": 1}
    ru.assert_same(flt, twin)


# ---- errors (rule 1) ------------------------------------------------------------------------------------------------------
def test_bad_calls_change_nothing_and_an_empty_list_writes_nothing():
    import torch
    from aruco_slam_amd.hip_backend import EkfError
    flt, _scene = ru.dense_filter("ekf", 5, 3, cov_dtype="float32")
    be, lib = flt.backend, flt.backend.lib
    before = (be.get_state(), be.get_cov(), be.cov_t.data_ptr(), be.state_t.data_ptr(), be.cov_t.cpu().numpy(), dict(flt.landmarks))
    nbytes = C.c_size_t()
    assert lib.ekf_remove_workspace_bytes(be.h, 1, C.byref(nbytes)) == 0 and nbytes.value >= 4 * be.ld
    cov_new = torch.full_like(be.cov_t, float("nan"))
    state_new = torch.full_like(be.state_t, float("nan"))
    ws = torch.zeros((nbytes.value + 256,), dtype=torch.uint8, device=be.device)
    torch.cuda.synchronize(be.device)

    def call(index, count=None, cov=cov_new, ld=be.ld, state=state_new, wsp=ws.data_ptr(), wsb=nbytes.value):
        idx = np.asarray(index, dtype=np.int32)
        return lib.ekf_remove_markers(be.h, idx.ctypes.data_as(C.POINTER(C.c_int32)), len(index) if count is None else count,
                                      cov.data_ptr() if cov is not None else None, ld,
                                      state.data_ptr() if state is not None else None, wsp, wsb)

    assert call([1, 3, 1]) == -1                        # duplicate
    assert call([5]) == -1 and call([-1]) == -1         # out of range
    assert call([1], count=-1) == -1                    # negative count
    assert call([1], ld=be.ld + 128) == -1              # wrong ld
    assert call([1], cov=None) == -1 and call([1], state=None) == -1 and call([1], wsp=None) == -1
    assert call([1], wsp=ws.data_ptr() + 8) == -1       # misaligned
    assert call([1], cov=be.cov_t) == -1                # the current buffer is read: it cannot be the new one
    assert call([1], wsb=nbytes.value - 1) == -2        # EKF_ERR_CAPACITY
    assert call([]) == 0                                # nothing to do: no rebinding, nothing written
    with pytest.raises(EkfError):
        be.remove_markers([7])
    with pytest.raises(KeyError):
        flt.remove_markers([2, 99])
    with pytest.raises(ValueError):
        flt.remove_markers([2, 2])
    flt.remove_markers([])
    torch.cuda.synchronize(be.device)
    assert torch.isnan(cov_new).all() and torch.isnan(state_new).all()
    assert (be.cov_t.data_ptr(), be.state_t.data_ptr()) == before[2:4] and flt.landmarks == before[5]
    assert np.array_equal(be.get_state(), before[0]) and np.array_equal(be.get_cov(), before[1])
    assert np.array_equal(be.cov_t.cpu().numpy(), before[4])
    assert flt.num_landmarks == 5 == be.num_landmarks
    # ... and the filter goes on: the same call, valid, works
    assert call([1]) == 0
    be.sync()
    assert be.num_landmarks == 4 and not torch.isnan(cov_new).any()


# ---- the policy, end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [None, 11.345])
def test_confirm_policy_prunes_the_spurious_ids_like_removals_by_hand(gate):
    from aruco_slam_amd.synthetic import ragged_log
    log = ragged_log(6, (5, 6), 16, seed=4, bootstrap_m=3)
    offs = log["offsets"]
    frames = [(log["ids"][offs[t]:offs[t + 1]].tolist(), log["poses"][offs[t]:offs[t + 1]]) for t in range(len(offs) - 1)]
    spurious = {4: 31, 9: 47}                           # frame -> a mis-decoded id, seen once
    for t, marker in spurious.items():
        ids, poses = frames[t]
        frames[t] = (ids + [marker], np.vstack((poses, poses[0] + np.array([0.4, -0.3, 0.2, 0, 0, 0]))))
    kw = dict(max_landmarks=8, max_visible=8, cov_dtype="float64", gate=gate)
    auto = ru.make_filter("ekf", confirm=(2, 5), **kw)
    hand = ru.make_filter("ekf", **kw)
    traj_a, traj_h, sizes = [], [], []
    for t, (ids, poses) in enumerate(frames):
        _, cam, _, _ = auto.process_detections(np.asarray(ids), poses)
        traj_a.append(np.array(cam))
        _, cam, _, _ = hand.process_detections(np.asarray(ids), poses)
        for t0, marker in spurious.items():
            if t == t0 + 4:                             # the end of the window: t - t0 + 1 = 5
                hand.remove_marker(marker)
        traj_h.append(np.array(cam))
        sizes.append(auto.num_landmarks)
    assert sorted(auto.landmarks) == [0, 1, 2, 3, 4, 5]
    assert sizes[4] == sizes[3] + 1 and sizes[8] == sizes[7] - 1 and 31 not in auto.landmarks
    assert np.array_equal(np.stack(traj_a), np.stack(traj_h))
    ru.assert_same(auto, hand)


def test_landmarks_a_log_replay_adds_are_confirmed():
    """The policy sees per-frame calls only: what ``process_detection_log`` adds is never pruned, whenever it is seen next."""
    scene = ru.Scene("ekf", 6, 3, seed=2)
    flt = ru.make_filter("ekf", max_landmarks=8, max_visible=4, confirm=(2, 3))
    log = ru.as_log(scene.bootstrap() + scene.frames(3, np.arange(6)))
    flt.process_detection_log(log["ids"], log["poses"], log["offsets"])
    for ids, poses in scene.frames(2, [0, 1, 2]) + [scene.frame([5, 0, 1])] + scene.frames(6, [0, 1, 2]):
        flt.process_detections(np.asarray(ids), poses)      # 3, 4 never again, 5 once
    assert sorted(flt.landmarks) == [0, 1, 2, 3, 4, 5]
    ids, poses = scene.frame([0, 1, 2])
    flt.process_detections(np.asarray(ids + [33]), np.vstack((poses, poses[0] + 0.3)))      # a new id in a per-frame call
    for ids, poses in scene.frames(2, [0, 1, 2]):
        flt.process_detections(np.asarray(ids), poses)
    assert sorted(flt.landmarks) == [0, 1, 2, 3, 4, 5]       # ... is tentative, and goes after its window


# ---- batch ----------------------------------------------------------------------------------------------------------------
def _batch_case(model, n, kw, B, lists, seed0):
    from aruco_slam_amd.batch import EKFBatch
    from aruco_slam_amd.filters.map_management import renumber_landmarks
    from aruco_slam_amd.synthetic import ragged_log
    rs = 0.05 if model == "ekf_rotations" else 0.0
    m_range = (2, 4)
    logs = [ragged_log(n, m_range, 5, seed=seed0 + b, rvec_sigma=rs) for b in range(B)]
    more = [ragged_log(n, m_range, 4, seed=seed0 + 50 + b, rvec_sigma=rs) for b in range(B)]
    batch = EKFBatch(B, ru.INIT, model=model, **kw)
    twin = EKFBatch(B, ru.INIT, model=model, **kw)
    batch.process_detection_logs(logs)
    assert batch.num_landmarks == [n] * B
    for b in range(B):                                   # the twins, by the restore path
        index = [batch.landmarks[b][k] for k in lists[b]]
        state, cov = ru.deleted(model, batch.get_state(b), batch.get_cov(b), index)
        table = renumber_landmarks(batch.landmarks[b], index)
        twin.set_member(b, state, cov, [k for k, _ in sorted(table.items(), key=lambda kv: kv[1])])
    batch.remove_markers(lists)
    counts = batch._num_landmarks_device().tolist()
    assert counts == batch.num_landmarks == [n - len(ids) for ids in lists]
    assert batch.landmarks == twin.landmarks
    for b in range(B):
        assert np.array_equal(batch.get_state(b), twin.get_state(b)) and np.array_equal(batch.get_cov(b), twin.get_cov(b))
    assert np.array_equal(batch.state_t.cpu().numpy(), twin.state_t.cpu().numpy())
    assert np.array_equal(batch.cov_t.cpu().numpy(), twin.cov_t.cpu().numpy())
    ta, tb = batch.process_detection_logs(more), twin.process_detection_logs(more)
    for b in range(B):
        assert np.array_equal(ta[b], tb[b])
        assert np.array_equal(batch.get_state(b), twin.get_state(b)) and np.array_equal(batch.get_cov(b), twin.get_cov(b))
    assert batch.landmarks == twin.landmarks and batch.status() == twin.status() == [0] * B
    return batch


@pytest.mark.parametrize("model,n", [("ekf", 6), ("ekf_rotations", 5)])
def test_batch_removal_is_every_members_set_member_twin(model, n):
    lists = [[], [0], [n - 1, 1], list(range(n)), [2]]
    batch = _batch_case(model, n, {"max_landmarks": 8, "max_visible": 4}, 5, lists, seed0=10)
    with pytest.raises(KeyError):
        batch.remove_markers({0: [999]})
    before = batch.cov_t.data_ptr()
    batch.remove_markers([[], [], [], [], []])           # nothing to do: no rebinding
    assert batch.cov_t.data_ptr() == before
    batch.remove_markers({4: [0]})                       # the dict form
    assert 0 not in batch.landmarks[4] and batch._num_landmarks_device()[4] == batch.num_landmarks[4]


def test_batch_removal_with_large_maps():
    batch = _batch_case("ekf", 12, {"max_landmarks": 338, "max_visible": 4, "large_maps": True}, 2, [[11, 0, 5], [3]],
                        seed0=20)
    assert batch.ld == 1024
