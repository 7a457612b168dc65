"""Dictionary-sized batch maps (``EKFBatch(large_maps=True)``, the one-block instances of the kernels of ekf_batch_wide.hip)
on an MI355X: the same bits as the one-column kernels where both run and pinned bits just above them, the extended-precision
step up to N = 1024, the single-filter path at n = 250 / 100, the covariance invariants, composition and window independence,
capacity errors and interop with ``EKF``."""
import hashlib

import numpy as np
import pytest

import gating_util as gu
import support as sp
import update_sweep_util as sw
from conftest import rel_err, report

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
# (c_P, c_x) of the large-map kernels against the extended-precision step: 4x the worst ratio measured on an MI355X
# (EKF: r_P 3.68 at n = 83, m = 1, r_x 0.76 at n = 83, m = 5; EKF_Rotations: r_P 1.30 at n = 25, m = 1, r_x 0.46 at n = 101,
# m = 3), rounded up to two digits
C_LARGE = {"ekf": (15, 3.1), "ekf_rotations": (5.3, 1.9)}
VISIBLE = {"ekf": 16, "ekf_rotations": 8}


def _batch(members, model="ekf", **kw):
    from aruco_slam_amd.batch import EKFBatch
    kw.setdefault("max_visible", VISIBLE[model])
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
    """Ragged logs up to n landmarks: bootstrap first sightings, more than 64 frames, empty frames that reach the kernel
    (no has_detections: every frame is stepped or repeated there), one member without a log and one with a non-finite
    pose in a bootstrap frame."""
    hi = VISIBLE[model] if model == "ekf" else 8
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


@pytest.mark.parametrize("model,n,quat", [("ekf", 82, "as_written"), ("ekf", 82, "scalar_first"), ("ekf", 50, "as_written"),
                                          ("ekf_rotations", 24, None)])
def test_same_bits_as_the_one_column_kernel(model, n, quat):
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    logs = _mixed_logs(model, n, seed=7 * n + (quat == "scalar_first"))
    assert max(len(lg["offsets"]) - 1 for lg in logs if lg is not None) > 64
    runs = []
    for large in (False, True):
        batch = _batch(len(logs), model, max_landmarks=n, quat_update=quat, large_maps=large)
        assert batch.large_maps is large
        trajs = batch.process_detection_logs(logs)
        runs.append((batch, trajs))
    (one, t_one), (big, t_big) = runs
    assert one.status() == big.status() and one.status()[3] == EKF_ERR_NUMERIC and one.status().count(0) == 5
    for b in range(len(logs)):
        assert np.array_equal(t_one[b], t_big[b], equal_nan=True), b
        for x, y in zip(_snapshot(one, b), _snapshot(big, b)):
            assert np.array_equal(x, y, equal_nan=True), b      # (the failed member keeps its NaN first sighting)
        assert one.landmarks[b] == big.landmarks[b] and one.num_landmarks[b] == big.num_landmarks[b]
    assert np.array_equal(one.cov_t.cpu().numpy(), big.cov_t.cpu().numpy(), equal_nan=True)


# Above 82 / 24 landmarks no second kernel computes the same frames, so the bits are pinned: sha256[:16] of
# test_bits_just_past_one_column_block's two runs, taken on an MI355X with the library of the last commit that had the
# large-map kernels in a file of their own (ekf_batch_large.hip); the kernels of ekf_batch_wide.hip give the same
PINNED_MAPS = {"ekf": 86, "ekf_rotations": 26}        # N = 268 / 270: two column blocks, two row panels per sweep
PINNED_DIGESTS = {
    ("ekf", "plain"): "f6dc9b8398a35b36",
    ("ekf", "gated"): "48871a8c83b8a545",
    ("ekf_rotations", "plain"): "0c4c85672220a5be",
    ("ekf_rotations", "gated"): "ffd82db6d36be9be",
}


def _pinned_logs(model):
    """Four short logs: bootstrap frames of 16 / 8 first sightings, six steady frames; member 1 with gating_util's gross
    outliers (frames of up to 16 / 8 detections) and an empty frame that reaches the kernel, member 3 on half the map."""
    n, hi = PINNED_MAPS[model], VISIBLE[model]
    logs = [_ragged(model, n if j < 3 else n // 2, (1, hi - 2), 6, seed=40 + j, bootstrap_m=hi) for j in range(4)]
    logs[1] = gu.dirty_log(model, logs[1], seed=1)[0]
    assert max(int(np.diff(lg["offsets"]).max()) for lg in logs) == hi and (np.diff(logs[1]["offsets"]) == 0).sum() == 1
    return [{k: v for k, v in lg.items() if k != "has_detections"} for lg in logs]


def _pinned_digest(batch, *fields):
    h = hashlib.sha256()
    for field in fields:
        for x in field:
            h.update(np.ascontiguousarray(x, dtype=np.float64).tobytes())
    for b in range(batch.members):
        for x in _snapshot(batch, b):
            h.update(x.tobytes())
    return h.hexdigest()[:16]


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_bits_just_past_one_column_block(model):
    logs = _pinned_logs(model)
    kw = {"max_landmarks": PINNED_MAPS[model], "quat_update": "scalar_first" if model == "ekf" else None}
    plain = _batch(4, model, **kw)
    assert plain.large_maps and plain.ld > 256
    digest = _pinned_digest(plain, plain.process_detection_logs(logs))
    gated = _batch(4, model, gate=np.array([np.inf, gu.GATES[model], np.inf, np.inf]), **kw)
    out = gated.process_detection_logs(logs, nis=True, cam_cov=True, mahal=True)
    digest_gated = _pinned_digest(gated, out.trajectory, out.nis, out.cam_cov, out.mahal)
    report(f"batch_large_pinned[{model}]", plain=digest, gated=digest_gated)
    assert plain.status() == gated.status() == [0] * 4 and plain.num_landmarks[0] == PINNED_MAPS[model]
    assert out.rejected[1].any() and not out.rejected[1].all() and not any(out.rejected[b].any() for b in (0, 2, 3))
    assert digest == PINNED_DIGESTS[(model, "plain")]
    assert digest_gated == PINNED_DIGESTS[(model, "gated")]


@pytest.mark.parametrize("model,sizes,top", [("ekf", (83, 167, 253, 338), 338), ("ekf_rotations", (25, 60, 101), 101)])
def test_members_against_the_extended_reference(model, sizes, top):
    """One call: member j sees m = 1..max_visible detections from its own dense prior, cycling through the map sizes."""
    tag, quat = ("rot", "scalar_first") if model == "ekf_rotations" else ("ekf", "as_written")
    vis = VISIBLE[model]
    keys = [sw.RefKey(tag, sizes[j % len(sizes)], j % vis + 1, "float64", quat) for j in range(max(vis, 2 * len(sizes)))]
    got = sw.references(keys)
    batch = _batch(len(keys), model, max_landmarks=top, quat_update=quat)
    assert batch.large_maps and batch.ld == 1024
    logs = []
    for b, key in enumerate(keys):
        state, p, lm_ids, ids, poses = got[key][0]
        batch.set_member(b, state, p, lm_ids)
        logs.append(_frame_log(ids, poses))
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
    c_p, c_x = C_LARGE[model]
    report(f"update_sweep[batch_large_{model},float64]", members=len(keys), ratio_P=worst[0], ratio_x=worst[1],
           worst_P_at=at[0], worst_x_at=at[1], c_P=c_p, c_x=c_x)
    assert worst[0] <= c_p and worst[1] <= c_x, worst


def _horizon(a, b, envelope=1e-8):
    d = np.abs(a - b).max(axis=1)
    bad = np.nonzero(d > envelope)[0]
    return int(bad[0]) - 1 if len(bad) else len(d) - 1


@pytest.mark.parametrize("model,n,hi", [("ekf", 250, 10), ("ekf_rotations", 100, 8)])
def test_against_the_single_filter_path(model, n, hi):
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    log = _ragged(model, n, (1, hi), 200, seed=31)
    cls = EKF_Rotations if model == "ekf_rotations" else EKF

    def single(poses):
        flt = cls(INIT, max_landmarks=n, max_visible=VISIBLE[model], cov_dtype="float64")
        return flt.process_detection_log(log["ids"], poses, log["offsets"], log["has_detections"]), flt.landmarks

    want, table = single(log["poses"])
    rng = np.random.default_rng(31)
    pert, _ = single(log["poses"] * (1.0 + 1e-15 * rng.standard_normal(log["poses"].shape)))
    hz = _horizon(want, pert)
    batch = _batch(3, model, max_landmarks=n)
    assert batch.large_maps
    got = batch.process_detection_logs([None, log, _ragged(model, 10, (1, hi), 30, seed=2)])[1]
    err = float(np.abs(got[:hz + 1] - want[:hz + 1]).max())
    report(f"batch_large_vs_single[{model},n={n},m=(1,{hi})]", horizon=hz, frames=len(want), max_abs=err)
    assert hz >= 50, hz
    assert err <= 1e-6, err
    assert batch.landmarks[1] == table


@pytest.mark.parametrize("n", [338, 330])
def test_covariance_symmetric_and_padding_zero(n):
    logs = [_ragged("ekf", n, (1, 16), 20, seed=n), _ragged("ekf", n // 2, (1, 16), 20, seed=n + 1)]
    batch = _batch(2, max_landmarks=n)
    batch.process_detection_logs(logs)
    assert batch.status() == [0, 0] and batch.ld == 1024
    P = batch.cov_t.cpu().numpy()
    S = batch.state_t.cpu().numpy()
    for b in range(2):
        N = 3 * batch.num_landmarks[b] + 10
        assert np.array_equal(P[b], P[b].T)
        assert not P[b, N:, :].any() and not P[b, :, N:].any() and not S[b, N:].any()
        assert np.isfinite(P[b, :N, :N]).all()
    assert 3 * batch.num_landmarks[0] + 10 == 3 * n + 10


def test_composition_independence_bitwise():
    log = _ragged("ekf", 200, (1, 16), 80, seed=3)
    others = [_ragged("ekf", n, (1, 16), 20, seed=s) for s, n in enumerate((40, 200, 120))] + [None]
    runs = []
    for B, slots in ((1, (0,)), (7, (3,)), (300, (5, 299))):
        logs = [others[i % len(others)] for i in range(B)]
        for s in slots:
            logs[s] = log
        batch = _batch(B, max_landmarks=200, large_maps=True)
        traj = batch.process_detection_logs(logs)
        for s in slots:
            runs.append((traj[s], *_snapshot(batch, s)))
        del batch
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("model,n", [("ekf", 250), ("ekf_rotations", 100)])
def test_continuation_across_calls_and_windows_is_bitwise(model, n):
    log = _ragged(model, n, (1, 8), 150, seed=5)
    frames = len(log["offsets"]) - 1
    assert frames > 2 * 64
    one = _batch(2, model, max_landmarks=n)
    t_one = one.process_detection_logs([log, None])[0]
    two = _batch(2, model, max_landmarks=n)
    cut = 100                                     # inside the second window
    t_a = two.process_detection_logs([sp.sub_log(log, 0, cut), None])[0]
    t_b = two.process_detection_logs([sp.sub_log(log, cut, frames), None])[0]
    assert np.array_equal(t_one, np.concatenate([t_a, t_b]))
    for a, b in zip(_snapshot(one, 0), _snapshot(two, 0)):
        assert np.array_equal(a, b)
    assert one.landmarks[0] == two.landmarks[0]


def test_a_log_beyond_capacity_raises_before_anything_runs():
    from aruco_slam_amd.hip_backend import EkfError
    n = 338
    batch = _batch(3, max_landmarks=n)
    logs = [_ragged("ekf", n, (1, 16), 5, seed=1), _ragged("ekf", 100, (1, 16), 5, seed=2), None]
    batch.process_detection_logs(logs)
    before = [_snapshot(batch, b) for b in range(3)]
    tables = [dict(t) for t in batch.landmarks]
    extra = _frame_log([10 ** 6], np.ones((1, 6)))                  # a new marker: landmark n + 1 of member 0
    with pytest.raises(EkfError) as info:
        batch.process_detection_logs([extra, _ragged("ekf", 100, (1, 16), 3, seed=4), None])
    assert info.value.code == -2
    assert batch.landmarks == tables and batch.status() == [0, 0, 0]
    for b in range(3):
        for a, c in zip(before[b], _snapshot(batch, b)):
            assert np.array_equal(a, c)


def test_to_filter_continues_as_an_ordinary_ekf():
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    n = 250
    batch = _batch(2, max_landmarks=n)
    log = _ragged("ekf", n, (1, 10), 20, seed=21)
    batch.process_detection_logs([log, None])
    flt = batch.to_filter(0)
    assert isinstance(flt, EKF) and flt.num_landmarks == n
    assert np.array_equal(np.asarray(flt.state), batch.get_state(0)) and np.array_equal(flt.uncertainty, batch.get_cov(0))
    more = _ragged("ekf", n, (1, 10), 3, seed=22)
    frames = len(more["offsets"]) - 1
    nxt = sp.sub_log(more, frames - 1, frames)                            # one steady frame of known markers
    flt.observe(nxt["ids"], nxt["poses"])
    got = batch.process_detection_logs([nxt, None])[0][-1]
    assert rel_err(got, np.asarray(flt.state)[:7]) <= 1e-10
    assert rel_err(batch.get_state(0), np.asarray(flt.state)) <= 1e-10
    assert rel_err(batch.get_cov(0), flt.uncertainty) <= 1e-10
    # load_filter round trip into the other member
    batch.load_filter(1, flt)
    assert np.array_equal(batch.get_state(1), np.asarray(flt.state)) and np.array_equal(batch.get_cov(1), flt.uncertainty)
    assert batch.landmarks[1] == flt.landmarks
