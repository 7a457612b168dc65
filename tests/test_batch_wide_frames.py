"""Wide batch frames (``EKFBatch(wide_frames=True)``, kernel ekf_batch_wide.hip) on an MI355X: the same bits as without the
flag where both run, the extended-precision step up to 64 / 50 detections, the single filter at m ~ U[1, 64] / U[1, 50], a
pivot that fails in a later block, the covariance invariants, composition and window independence, capacity errors and
interop with ``EKF``."""
import numpy as np
import pytest

import support as sp
import update_sweep_util as sw
from conftest import rel_err, report

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
# (c_P, c_x) of the wide-frame kernels against the extended-precision step: 4x the worst ratio measured on an MI355X
# (EKF: r_P 0.248 at n = 30, m = 17, r_x 0.200 at n = 338, m = 16; EKF_Rotations: r_P 0.186 at n = 50, m = 19, r_x 0.139 at
# n = 101, m = 8), rounded up to two digits: inside the large-map kernels' (15, 3.1) / (5.3, 1.9)
C_WIDE = {"ekf": (1.0, 0.8), "ekf_rotations": (0.75, 0.56)}
BLOCK = {"ekf": 16, "ekf_rotations": 8}          # detections per factorisation block
WIDE = {"ekf": 64, "ekf_rotations": 50}          # max_visible with the flag
RD = {"ekf": 3, "ekf_rotations": 7}
LMD = {"ekf": 3, "ekf_rotations": 10}


def _batch(members, model="ekf", **kw):
    from aruco_slam_amd.batch import EKFBatch
    kw.setdefault("max_visible", WIDE[model])
    return EKFBatch(members, INIT, model=model, **kw)


def _ragged(model, n, m_range, steady, seed, **kw):
    from aruco_slam_amd.synthetic import ragged_log
    return ragged_log(n, m_range, steady, seed=seed, rvec_sigma=0.05 if model == "ekf_rotations" else 0.0, **kw)


def _frame_log(ids, poses):
    ids = np.asarray(ids, dtype=np.int32)
    return {"ids": ids, "poses": np.asarray(poses, dtype=np.float64), "offsets": np.array([0, len(ids)], dtype=np.int64)}


def _snapshot(batch, b):
    return batch.get_state(b), batch.get_cov(b)


def _mixed_logs(model, n, seed):
    """Ragged logs up to n landmarks with at most BLOCK detections per frame: bootstrap first sightings, more than 64
    frames, empty frames that reach the kernel, one member without a log and one with a non-finite pose in a bootstrap
    frame."""
    hi = BLOCK[model]
    logs = []
    for j, nj in enumerate((n, max(1, n // 3), n, max(2, n // 2), n)):
        lg = _ragged(model, nj, (0 if j % 2 else 1, min(nj, hi)), 100, seed=seed + j)
        if j % 2:
            lg = {k: v for k, v in lg.items() if k != "has_detections"}
        logs.append(lg)
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in logs[3].items()}
    bad["poses"][int(bad["offsets"][1]), 0] = np.nan
    logs[3] = bad
    logs.append(None)
    return logs


def _assert_same(one, t_one, two, t_two):
    assert one.status() == two.status()
    for b in range(one.members):
        assert np.array_equal(t_one[b], t_two[b], equal_nan=True), b
        for x, y in zip(_snapshot(one, b), _snapshot(two, b)):
            assert np.array_equal(x, y, equal_nan=True), b
        assert one.landmarks[b] == two.landmarks[b] and one.num_landmarks[b] == two.num_landmarks[b]


@pytest.mark.parametrize("model,n,quat", [("ekf", 50, "as_written"), ("ekf", 250, "as_written"),
                                          ("ekf", 250, "scalar_first"), ("ekf_rotations", 24, None),
                                          ("ekf_rotations", 100, None)])
def test_same_bits_as_without_the_flag(model, n, quat):
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    logs = _mixed_logs(model, n, seed=11 * n + (quat == "scalar_first"))
    assert max(len(lg["offsets"]) - 1 for lg in logs if lg is not None) > 64
    runs = []
    for wide in (False, True):
        batch = _batch(len(logs), model, max_landmarks=n, quat_update=quat, wide_frames=wide,
                       max_visible=WIDE[model] if wide else BLOCK[model])
        assert batch.wide_frames is wide
        runs.append((batch, batch.process_detection_logs(logs)))
    (one, t_one), (wide, t_wide) = runs
    assert one.status()[3] == EKF_ERR_NUMERIC and one.status().count(0) == 5
    _assert_same(one, t_one, wide, t_wide)


def _keys(tag, quat, sizes, ms):
    return [sw.RefKey(tag, sizes[j % len(sizes)], m, "float64", quat) for j, m in enumerate(ms)]


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_members_against_the_extended_reference(model):
    """One call: member j takes one frame of m detections from its own dense prior.  m covers 17..64 (EKF) / 9..50
    (EKF_Rotations) once over the map sizes, and every block boundary at every map size; m > n repeats landmarks, so
    some duplicate ids fall into two blocks."""
    if model == "ekf":
        tag, quat, sizes, top, vis = "ekf", "as_written", (30, 82, 170, 338), 338, 64
        bounds = (16, 17, 32, 33, 48, 49, 64)
    else:
        tag, quat, sizes, top, vis = "rot", "scalar_first", (50, 101), 101, 50
        bounds = (8, 9, 16, 17, 48, 49, 50)
    lo = BLOCK[model] + 1
    keys = _keys(tag, quat, sizes, range(lo, vis + 1))
    keys += [sw.RefKey(tag, n, m, "float64", quat) for n in sizes for m in bounds]
    keys.append(sw.RefKey(tag, 12, 2 * BLOCK[model] + 4, "float64", quat))      # m > n: repeated ids in later blocks
    keys = list(dict.fromkeys(keys))
    got = sw.references(keys)
    batch = _batch(len(keys), model, max_landmarks=top, quat_update=quat)
    assert batch.wide_frames and batch.ld == 1024
    logs, split = [], 0
    blk = BLOCK[model]
    for b, key in enumerate(keys):
        state, p, lm_ids, ids, poses = got[key][0]
        batch.set_member(b, state, p, lm_ids)
        logs.append(_frame_log(ids, poses))
        blocks = [set(ids[i:i + blk]) for i in range(0, len(ids), blk)]
        split += sum(len(x & y) for i, x in enumerate(blocks) for y in blocks[i + 1:]) > 0
    assert split > 0                 # (members whose frame has a duplicate id in two blocks)
    batch.process_detection_logs(logs)
    assert batch.status() == [0] * len(keys)
    worst, at = np.zeros(2), [None, None]
    for b, key in enumerate(keys):
        ref = got[key][1]
        assert ref["kappa"] <= sw.KAPPA_MAX
        p = batch.get_cov(b)
        assert np.array_equal(p, p.T)
        r = sw.ratios(ref, p, batch.get_state(b), "float64")
        for i in range(2):
            if r[i] > worst[i]:
                worst[i], at[i] = r[i], f"n={key.n},m={key.m}"
    c_p, c_x = C_WIDE[model]
    report(f"update_sweep[batch_wide_{model},float64]", members=len(keys), ratio_P=worst[0], ratio_x=worst[1],
           worst_P_at=at[0], worst_x_at=at[1], c_P=c_p, c_x=c_x)
    assert worst[0] <= c_p and worst[1] <= c_x, worst


def _horizon(a, b, envelope=1e-8):
    d = np.abs(a - b).max(axis=1)
    bad = np.nonzero(d > envelope)[0]
    return int(bad[0]) - 1 if len(bad) else len(d) - 1


@pytest.mark.parametrize("model,n", [("ekf", 200), ("ekf_rotations", 100)])
def test_against_the_single_filter_path(model, n):
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    hi = WIDE[model]
    log = _ragged(model, n, (1, hi), 120, seed=41)
    assert (np.diff(log["offsets"]) > BLOCK[model]).mean() > 0.5
    cls = EKF_Rotations if model == "ekf_rotations" else EKF

    def single(poses):
        flt = cls(INIT, max_landmarks=n, max_visible=hi, cov_dtype="float64")
        return flt.process_detection_log(log["ids"], poses, log["offsets"], log["has_detections"]), flt.landmarks

    want, table = single(log["poses"])
    rng = np.random.default_rng(41)
    pert, _ = single(log["poses"] * (1.0 + 1e-15 * rng.standard_normal(log["poses"].shape)))
    hz = _horizon(want, pert)
    batch = _batch(3, model, max_landmarks=n)
    assert batch.wide_frames
    got = batch.process_detection_logs([None, log, _ragged(model, 10, (1, 10), 30, seed=2)])[1]
    err = float(np.abs(got[:hz + 1] - want[:hz + 1]).max())
    report(f"batch_wide_vs_single[{model},n={n},m=(1,{hi})]", horizon=hz, frames=len(want), max_abs=err)
    assert hz >= 50, hz
    assert err <= 1e-6, err
    assert batch.landmarks[1] == table
    assert batch.status() == [0, 0, 0]


def _later_block_prior(model, n):
    """(state, P, ids, frame ids, frame poses): a diagonal P that is positive everywhere but on landmark BLOCK, which is
    -10; the frame sees landmarks 0 .. BLOCK - 1 (the first block) and then landmark BLOCK (the second)."""
    lmd, blk = LMD[model], BLOCK[model]
    rng = np.random.default_rng(5)
    dims = lmd * n + 10
    state = np.zeros(dims)
    state[:10] = INIT
    for i in range(n):
        c0 = 10 + lmd * i
        state[c0:c0 + 3] = [rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(1.5, 2.5)]
        if lmd == 10:
            state[c0 + 3] = 1.0
    d = np.full(dims, 0.05)
    d[:10] = 0.01
    d[10 + lmd * blk:10 + lmd * (blk + 1)] = -10.0
    ids = list(range(blk + 1))
    poses = np.zeros((blk + 1, 6))
    for j, i in enumerate(ids):
        c0 = 10 + lmd * i
        poses[j, :3] = state[c0:c0 + 3] + rng.normal(0.0, 0.01, 3)
        poses[j, 3:] = rng.normal(0.0, 0.01, 3)
    return state, np.diag(d), list(range(n)), ids, poses


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_a_pivot_failing_in_a_later_block_leaves_the_member_as_it_was(model):
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    n, blk = 40, BLOCK[model]
    state, p, lm_ids, ids, poses = _later_block_prior(model, n)
    frame = _frame_log(ids, poses)
    first_block = _frame_log(ids[:blk], poses[:blk])
    more = _ragged(model, n, (1, 30), 10, seed=8)
    more = sp.sub_log(more, more["bootstrap_frames"], len(more["offsets"]) - 1)
    bad = {"ids": np.concatenate([frame["ids"], more["ids"]]), "poses": np.concatenate([frame["poses"], more["poses"]]),
           "offsets": np.concatenate([[0], len(ids) + more["offsets"]]).astype(np.int64)}
    others = [_ragged(model, 60, (1, min(60, WIDE[model])), 40, seed=9), _ragged(model, 30, (1, 20), 40, seed=10)]
    runs = []
    for member1 in (bad, None):
        batch = _batch(4, model, max_landmarks=n + 60)
        batch.set_member(1, state, p, lm_ids)
        batch.set_member(3, state, p, lm_ids)
        before = _snapshot(batch, 1)
        trajs = batch.process_detection_logs([others[0], member1, others[1], first_block])
        runs.append((batch, trajs, before))
    (failed, t_failed, before), (clean, t_clean, _) = runs
    st = failed.status()
    assert st[1] == EKF_ERR_NUMERIC and st[3] == 0 and st[0] == st[2] == 0       # block 1 alone passes
    assert np.isnan(t_failed[1]).all() and t_failed[1].shape[0] == len(bad["offsets"]) - 1
    for x, y in zip(before, _snapshot(failed, 1)):
        assert np.array_equal(x, y)
    assert failed.num_landmarks[1] == n
    for b in (0, 2, 3):
        assert np.array_equal(t_failed[b], t_clean[b]), b
        for x, y in zip(_snapshot(failed, b), _snapshot(clean, b)):
            assert np.array_equal(x, y), b


@pytest.mark.parametrize("model,n", [("ekf", 338), ("ekf", 330), ("ekf_rotations", 101)])
def test_covariance_symmetric_and_padding_zero(model, n):
    lmd = LMD[model]
    logs = [_ragged(model, n, (1, WIDE[model]), 12, seed=n), _ragged(model, n // 2, (1, WIDE[model]), 12, seed=n + 1)]
    batch = _batch(2, model, max_landmarks=n)
    batch.process_detection_logs(logs)
    assert batch.status() == [0, 0] and batch.ld == 1024
    P = batch.cov_t.cpu().numpy()
    S = batch.state_t.cpu().numpy()
    for b in range(2):
        N = lmd * batch.num_landmarks[b] + 10
        assert np.array_equal(P[b], P[b].T)
        assert not P[b, N:, :].any() and not P[b, :, N:].any() and not S[b, N:].any()
        assert np.isfinite(P[b, :N, :N]).all()
    assert batch.num_landmarks[0] == n


def test_composition_independence_bitwise():
    """A member's bits do not depend on its neighbours' frame widths (the call's kmax and window) or on their number."""
    log = _ragged("ekf", 200, (1, 20), 60, seed=3)
    others = [_ragged("ekf", n, (1, min(n, 64)), 20, seed=s) for s, n in enumerate((40, 200, 120))] + [None]
    runs = []
    for B, slots in ((1, (0,)), (7, (3,)), (70, (5, 69))):
        logs = [others[i % len(others)] for i in range(B)]
        for s in slots:
            logs[s] = log
        batch = _batch(B, max_landmarks=200)
        traj = batch.process_detection_logs(logs)
        for s in slots:
            runs.append((traj[s], *_snapshot(batch, s)))
        del batch
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("model,n", [("ekf", 250), ("ekf_rotations", 100)])
def test_continuation_across_calls_and_windows_is_bitwise(model, n):
    log = _ragged(model, n, (1, WIDE[model]), 60, seed=5)
    frames = len(log["offsets"]) - 1
    one = _batch(2, model, max_landmarks=n)
    t_one = one.process_detection_logs([log, None])[0]
    two = _batch(2, model, max_landmarks=n)
    cut = 37                                      # inside a window of the wide batch (16 / 9 frames)
    t_a = two.process_detection_logs([sp.sub_log(log, 0, cut), None])[0]
    t_b = two.process_detection_logs([sp.sub_log(log, cut, frames), None])[0]
    assert one.status() == [0, 0]
    assert np.array_equal(t_one, np.concatenate([t_a, t_b]))
    for a, b in zip(_snapshot(one, 0), _snapshot(two, 0)):
        assert np.array_equal(a, b)
    assert one.landmarks[0] == two.landmarks[0]


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_a_frame_beyond_max_visible_raises_before_anything_runs(model):
    from aruco_slam_amd.hip_backend import EkfError
    n, vis = 80, WIDE[model]
    batch = _batch(3, model, max_landmarks=n)
    logs = [_ragged(model, n, (1, vis), 5, seed=1), _ragged(model, 60, (1, min(60, vis)), 5, seed=2), None]
    batch.process_detection_logs(logs)
    before = [_snapshot(batch, b) for b in range(3)]
    tables = [dict(t) for t in batch.landmarks]
    known = sorted(batch.landmarks[0])[:vis + 1]
    wide = _frame_log(known, np.ones((vis + 1, 6)))                  # one detection too many, all of known markers
    with pytest.raises(EkfError) as info:
        batch.process_detection_logs([wide, _ragged(model, 60, (1, min(60, vis)), 3, seed=4), None])
    assert info.value.code == -2
    assert batch.landmarks == tables and batch.status() == [0, 0, 0]
    for b in range(3):
        for a, c in zip(before[b], _snapshot(batch, b)):
            assert np.array_equal(a, c)


def test_to_filter_continues_as_an_ordinary_ekf():
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    n = 200
    batch = _batch(2, max_landmarks=n)
    log = _ragged("ekf", n, (17, 64), 10, seed=21)
    batch.process_detection_logs([log, None])
    flt = batch.to_filter(0)
    assert isinstance(flt, EKF) and flt.num_landmarks == n
    assert np.array_equal(np.asarray(flt.state), batch.get_state(0)) and np.array_equal(flt.uncertainty, batch.get_cov(0))
    more = _ragged("ekf", n, (40, 64), 3, seed=22)
    frames = len(more["offsets"]) - 1
    nxt = sp.sub_log(more, frames - 1, frames)                            # one steady wide frame of known markers
    assert len(nxt["ids"]) > 16
    flt.observe(nxt["ids"], nxt["poses"])
    got = batch.process_detection_logs([nxt, None])[0][-1]
    assert rel_err(got, np.asarray(flt.state)[:7]) <= 1e-10
    assert rel_err(batch.get_state(0), np.asarray(flt.state)) <= 1e-10
    assert rel_err(batch.get_cov(0), flt.uncertainty) <= 1e-10
    batch.load_filter(1, flt)
    assert np.array_equal(batch.get_state(1), np.asarray(flt.state)) and np.array_equal(batch.get_cov(1), flt.uncertainty)
    assert batch.landmarks[1] == flt.landmarks
