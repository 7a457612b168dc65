"""The per-detection chi-square gate and the Mahalanobis distance output of ``EKFBatch`` on an MI355X, in every window
kernel: off is off, the gated replay is the gate-off replay of the log without the rejected detections (bit for bit),
distances and decisions against the oracle, outliers go and inliers stay, neighbours do not matter, ``mahal`` is the same
bits in every kernel, replicas, failing members and bad gates."""
import ctypes
import hashlib

import numpy as np
import pytest

import gating_util as gu
import support as sp
from conftest import report

pytestmark = pytest.mark.gpu

INIT = gu.INIT
ALL = list(gu.FAMILIES)


def _same_outputs(got, want, what):
    for name in ("trajectory", "nis", "cam_cov", "dof"):
        for b, (u, v) in enumerate(zip(getattr(got, name), getattr(want, name))):
            assert np.array_equal(u, v, equal_nan=True), (what, name, b)


def _digest(batch, out):
    h = hashlib.sha256()
    for t in out:
        h.update(np.ascontiguousarray(t).tobytes())
    for s, p in sp.snap_batch(batch):
        h.update(s.tobytes())
        h.update(p.tobytes())
    return h.hexdigest()[:16]


# sha256[:16] over every member's trajectory, state and covariance of the 256-member gate-off batches of
# test_a_256_member_batch_hashes_as_before_the_gate, taken with the library built from the commit before the gate
PARENT_DIGESTS = {
    ("ekf", "column"): "4215dfbcb75f6d51",
    ("ekf_rotations", "column"): "c8322f9c33dce959",
    ("ekf", "large"): "4215dfbcb75f6d51",
    ("ekf_rotations", "large"): "c8322f9c33dce959",
    ("ekf", "wide"): "4a42e0fa72abd759",
    ("ekf_rotations", "wide"): "9b17142e2c7eb81a",
}


@pytest.mark.parametrize("model,family", ALL)
def test_off_is_off(model, family):
    logs = [gu.dirty_log(model, gu.clean_log(model, family, seed=s), seed=s)[0] for s in range(3)] + [None]
    plain = sp.family_batch(4, model, family)
    want = plain.process_detection_logs(logs, nis=True, cam_cov=True)
    for name, kw, call in (("gate=None", {"gate": None}, {}), ("gate=inf", {"gate": np.inf}, {}),
                           ("mahal only", {}, {"mahal": True})):
        batch = sp.family_batch(4, model, family, **kw)
        got = batch.process_detection_logs(logs, nis=True, cam_cov=True, **call)
        _same_outputs(got, want, name)
        sp.assert_same(sp.snap_batch(batch), sp.snap_batch(plain), name, equal_nan=True)
        assert batch.status() == plain.status() and batch.landmarks == plain.landmarks, name
        if name != "gate=None":
            assert not any(r.any() for r in got.rejected), name
            for b in range(3):      # exactly 0 where the log first shows an id (exempt), a tested distance elsewhere
                first = np.zeros(len(logs[b]["ids"]), dtype=bool)
                first[np.unique(logs[b]["ids"], return_index=True)[1]] = True
                assert np.isfinite(got.mahal[b]).all() and (got.mahal[b][first] == 0).all(), (name, b)
                assert (got.mahal[b][~first] > 0).all(), (name, b)


@pytest.mark.parametrize("model,family", ALL)
def test_only_the_first_occurrence_of_a_new_landmark_is_exempt(model, family):
    """A landmark first sighted twice in one frame: the first occurrence reports exactly 0, the second one is tested
    against the landmark the first one placed (z differs from h by the offset between the two poses)."""
    log = gu.clean_log(model, family, seed=4)
    n0 = int(log["offsets"][1])
    ids = np.concatenate((log["ids"][:n0], log["ids"][:2]))
    poses = np.vstack((log["poses"][:n0], log["poses"][:2] + np.array([0.3, -0.2, 0.1, 0, 0, 0])))
    frame = {"ids": ids.astype(np.int32), "poses": poses, "offsets": np.array([0, n0 + 2], np.int64)}
    for gate, rejected in ((None, False), (1e-6, True)):
        out = sp.family_batch(1, model, family, gate=gate).process_detection_logs([frame], mahal=True)
        assert (out.mahal[0][:n0] == 0).all() and not out.rejected[0][:n0].any()
        assert np.isfinite(out.mahal[0][n0:]).all() and (out.mahal[0][n0:] > 1e-6).all()
        assert out.rejected[0][n0:].all() == rejected and out.dof[0][0] == gu.RD[model] * (n0 if rejected else n0 + 2)


@pytest.mark.parametrize("model,family", ALL)
def test_a_256_member_batch_hashes_as_before_the_gate(model, family):
    """The digest of trajectories, states and covariances of 256 members, gate off, is the one the library of the commit
    before the gate gave on an MI355X for the same logs (PARENT_DIGESTS, also in DESIGN 4.7.5)."""
    logs = [gu.clean_log(model, family, seed=s % 8) for s in range(256)]
    batch = sp.family_batch(256, model, family)
    digest = _digest(batch, batch.process_detection_logs(logs))
    report(f"gating_hash_{model}_{family}", digest=digest)
    assert digest == PARENT_DIGESTS[(model, family)]
    gated = sp.family_batch(256, model, family, gate=np.inf)
    assert _digest(gated, gated.process_detection_logs(logs).trajectory) == digest


@pytest.mark.parametrize("model,family", ALL)
def test_gated_replay_is_the_replay_of_the_log_without_the_rejected(model, family):
    gate = gu.GATES[model]
    logs, marks = zip(*(gu.dirty_log(model, gu.clean_log(model, family, seed=s), seed=s) for s in range(3)))
    # member 3: a tight gate that also rejects ordinary detections, so what is deleted is the device's own choice
    logs, gates = list(logs) + [logs[0]], np.array([gate, gate, gate, 1e-3])
    gated = sp.family_batch(4, model, family, gate=gates)
    got = gated.process_detection_logs(logs, nis=True, cam_cov=True)
    assert gated.status() == [0] * 4
    for b in range(3):
        assert np.array_equal(got.rejected[b], marks[b]), b
    assert got.rejected[3].sum() > marks[0].sum() and not got.rejected[3].all()
    if family == "wide":        # the deletions shift block boundaries
        block = 16 if model == "ekf" else 8
        offs = logs[0]["offsets"]
        assert any(offs[t + 1] - offs[t] > block and got.rejected[0][offs[t]:offs[t] + block].any()
                   for t in range(len(offs) - 1))
    plain = sp.family_batch(4, model, family)
    want = plain.process_detection_logs([gu.delete(lg, rj) for lg, rj in zip(logs, got.rejected)], nis=True, cam_cov=True)
    _same_outputs(got, want, "deleted log")
    sp.assert_same(sp.snap_batch(gated), sp.snap_batch(plain), "state / P", equal_nan=True)
    assert gated.landmarks == plain.landmarks and gated.num_landmarks == plain.num_landmarks
    # frames without a survivor are not stepped
    offs = logs[0]["offsets"]
    none = [t for t in range(len(offs) - 1) if offs[t + 1] > offs[t] and got.rejected[0][offs[t]:offs[t + 1]].all()]
    assert none
    for t in none:
        assert got.nis[0][t] == 0 and got.dof[0][t] == 0 and np.array_equal(got.trajectory[0][t], got.trajectory[0][t - 1])


@pytest.mark.parametrize("family", ["column", "large", "wide"])
@pytest.mark.parametrize("case", ["c1", "g5"])
def test_distances_and_decisions_against_the_oracle_teacher_forced(case, family):
    """|d^2 - want| / want <= max(1e-9, 100 kappa(S_d) 2^-52) for every detection of the C1 / G5 frames, and the oracle's
    decisions (test_batch_gating_cpu.py: none is within that margin of the gate).  Measured on an MI355X: worst
    ratio to the tolerance 3.6e-5 (C1, 773 detections) and 2.4e-6 (G5, 29 detections), the same in all three kernels."""
    from aruco_slam_amd.batch import EKFBatch
    model, frames = gu.teacher_frames(case)
    gate = gu.GATES[model]
    extra = {"column": {}, "large": {"large_maps": True}, "wide": {"wide_frames": True}}[family]
    batch = EKFBatch(len(frames), INIT, model=model, max_landmarks=16 if case == "c1" else 8,
                     max_visible=max(len(f[3]) for f in frames), gate=gate, **extra)
    for b, (s0, p0, lm, _ids, _poses) in enumerate(frames):
        batch.set_member(b, s0, p0, lm)
    logs = [{"ids": np.asarray(f[3], np.int32), "poses": np.asarray(f[4], np.float64),
             "offsets": np.array([0, len(f[3])], np.int64)} for f in frames]
    out = batch.process_detection_logs(logs)
    assert batch.status() == [0] * len(frames)
    worst, checked, rejected = 0.0, 0, 0
    for b, (s0, p0, lm, ids, poses) in enumerate(frames):
        want, kappa = gu.teacher_distances(model, s0, p0, lm, ids, poses)
        for j in range(len(ids)):
            rel, tol = abs(out.mahal[b][j] - want[j]) / want[j], gu.tolerance(kappa[j])
            print(f"{case} {family} member {b} detection {j}: d2 {out.mahal[b][j]:.17g} want {want[j]:.17g} rel/tol {rel / tol:.3g}")
            assert rel <= tol, (b, j, rel, tol)
            worst = max(worst, rel / tol)
            checked += 1
        assert np.array_equal(out.rejected[b], want > gate), b
        rejected += int(out.rejected[b].sum())
    report(f"gating_oracle_{case}_{family}", detections=checked, rejected=rejected, worst_over_tol=worst)
    assert checked >= 9 and rejected >= 1


@pytest.mark.parametrize("model,family", ALL)
def test_outliers_go_and_inliers_stay(model, family):
    clean = gu.clean_log(model, family, seed=0)
    dirty, marks = gu.dirty_log(model, clean, seed=0)
    empty = gu.extra_frames(dirty, marks)          # (the frames the dirty log has more: they are not stepped)
    gated, loose, ref = (sp.family_batch(1, model, family, gate=gu.GATES[model]), sp.family_batch(1, model, family),
                         sp.family_batch(1, model, family))
    got = gated.process_detection_logs([dirty], nis=True, cam_cov=True)
    bent = loose.process_detection_logs([dirty], nis=True, cam_cov=True)
    want = ref.process_detection_logs([clean], nis=True, cam_cov=True)
    assert np.array_equal(got.rejected[0], marks)
    for name in ("trajectory", "nis", "cam_cov", "dof"):
        assert np.array_equal(getattr(got, name)[0][~empty], getattr(want, name)[0]), name
    sp.assert_same(sp.snap_batch(gated), sp.snap_batch(ref), "gated(dirty) = ungated(clean)", equal_nan=True)
    assert not np.array_equal(bent.trajectory[0][~empty], want.trajectory[0])


def test_neighbours_do_not_matter():
    model, family = "ekf", "column"
    log = gu.dirty_log(model, gu.clean_log(model, family, seed=1), seed=1)[0]
    gates = np.array([gu.GATES[model], np.inf, 1e-3, 50.0])
    whole = sp.family_batch(4, model, family, gate=gates)
    got = whole.process_detection_logs([log] * 4, nis=True, cam_cov=True)
    snap = sp.snap_batch(whole)
    for b in range(4):
        alone = sp.family_batch(1, model, family, gate=gates[b])
        one = alone.process_detection_logs([log], nis=True, cam_cov=True)
        for name in ("trajectory", "nis", "cam_cov", "dof", "mahal", "rejected"):
            assert np.array_equal(getattr(one, name)[0], getattr(got, name)[b], equal_nan=True), (b, name)
        sp.assert_same(sp.snap_batch(alone), snap[b:b + 1], b, equal_nan=True)
    assert len({r.sum() for r in got.rejected}) >= 3


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_mahal_is_bitwise_equal_across_kernels(model):
    log = gu.dirty_log(model, gu.clean_log(model, "column", seed=2), seed=2)[0]
    outs = []
    for family in ("column", "large", "wide"):
        kw = dict(gu.FAMILIES[(model, "column")][0], gate=gu.GATES[model])
        kw.update({"column": {}, "large": {"large_maps": True}, "wide": {"wide_frames": True}}[family])
        from aruco_slam_amd.batch import EKFBatch
        outs.append(EKFBatch(2, INIT, model=model, **kw).process_detection_logs([log, None], nis=True))
    ref, offs = outs[0], log["offsets"]
    for family, other in zip(("large", "wide"), outs[1:]):
        # frames whose prior agrees: the first one, and every frame behind a frame with equal rows
        same = (ref.trajectory[0] == other.trajectory[0]).all(axis=1)
        prior = np.concatenate(([True], same[:-1]))
        prior = np.logical_and.accumulate(prior)
        report(f"gating_mahal_across_kernels_{model}_{family}", frames=len(prior), agreeing=int(prior.sum()))
        assert prior.sum() > 10
        dets = np.repeat(prior, np.diff(offs))
        assert np.array_equal(ref.mahal[0][dets], other.mahal[0][dets], equal_nan=True)


@pytest.mark.parametrize("case", ["c1", "g5"])
def test_mahal_is_bitwise_equal_across_kernels_teacher_forced(case):
    """The same prior in all three kernels (set_member on the C1 / G5 frames): every detection's d^2 is the same bits."""
    from aruco_slam_amd.batch import EKFBatch
    model, frames = gu.teacher_frames(case)
    logs = [{"ids": np.asarray(f[3], np.int32), "poses": np.asarray(f[4], np.float64),
             "offsets": np.array([0, len(f[3])], np.int64)} for f in frames]
    outs = []
    for extra in ({}, {"large_maps": True}, {"wide_frames": True}):
        batch = EKFBatch(len(frames), INIT, model=model, max_landmarks=16 if case == "c1" else 8,
                         max_visible=max(len(f[3]) for f in frames), **extra)
        for b, (s0, p0, lm, _ids, _poses) in enumerate(frames):
            batch.set_member(b, s0, p0, lm)
        outs.append(np.concatenate(batch.process_detection_logs(logs, mahal=True).mahal))
    assert np.isfinite(outs[0]).all() and (outs[0] > 0).all() and len(outs[0]) >= 9
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize("model,family", [("ekf", "column"), ("ekf_rotations", "large"), ("ekf", "wide")])
def test_replicas_with_a_gate_equal_explicit_logs(model, family):
    from aruco_slam_amd.batch import GatedReplicaReplay, replica_poses
    B, seed = 4, 77
    log = gu.dirty_log(model, gu.clean_log(model, family, seed=3), seed=3)[0]
    gates = np.array([gu.GATES[model], 2.0, np.inf, gu.GATES[model]])
    sigma = np.random.default_rng(2).uniform(0.002, 0.02, (B, 6))
    batch = sp.family_batch(B, model, family, gate=gates)
    got = batch.replay_replicas(log, sigma, seed, nis=True, cam_cov=True)
    assert isinstance(got, GatedReplicaReplay)
    poses = replica_poses(log["poses"], sigma, seed)
    explicit = sp.family_batch(B, model, family, gate=gates)
    want = explicit.process_detection_logs([dict(log, poses=poses[b]) for b in range(B)], nis=True, cam_cov=True)
    for name in ("trajectory", "nis", "cam_cov", "dof", "mahal", "rejected"):
        assert np.array_equal(getattr(got, name), np.stack(getattr(want, name)), equal_nan=True), name
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(explicit), "state / P", equal_nan=True)
    assert got.rejected.any() and not got.rejected[2].any()


def test_failing_member_and_bad_gates():
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    from aruco_slam_amd.hip_backend import EkfError
    model, family = "ekf", "column"
    logs = [gu.dirty_log(model, gu.clean_log(model, family, seed=s), seed=s)[0] for s in range(3)]
    boot = [{"ids": lg["ids"][:lg["offsets"][8]], "poses": lg["poses"][:lg["offsets"][8]],
             "offsets": lg["offsets"][:9]} for lg in logs]
    rest = [{"ids": lg["ids"][lg["offsets"][8]:], "poses": lg["poses"][lg["offsets"][8]:],
             "offsets": lg["offsets"][8:] - lg["offsets"][8]} for lg in logs]
    ref, bad = sp.family_batch(3, model, family, gate=gu.GATES[model]), sp.family_batch(3, model, family, gate=gu.GATES[model])
    for batch in (ref, bad):
        batch.process_detection_logs(boot)
    ids = [k for k, _ in sorted(bad.landmarks[1].items(), key=lambda kv: kv[1])]
    s0 = bad.get_state(1)
    bad.set_member(1, s0, -np.eye(s0.shape[0]), ids)          # (no S_d and no S can be positive definite)
    want = ref.process_detection_logs(rest, nis=True)
    got = bad.process_detection_logs(rest, nis=True)
    assert bad.status() == [0, EKF_ERR_NUMERIC, 0]
    offs = rest[1]["offsets"]
    first = int(np.nonzero(np.diff(offs))[0][0])          # the failing frame: its distances are the pivot failures' NaN
    assert np.isnan(got.mahal[1]).all() and not got.rejected[1].any()
    assert np.isnan(got.trajectory[1][first:]).all()
    for b in (0, 2):
        for name in ("trajectory", "nis", "dof", "mahal", "rejected"):
            assert np.array_equal(getattr(got, name)[b], getattr(want, name)[b], equal_nan=True), (b, name)
    # a joint S that is not positive definite under S_d that are: the failing frame keeps its distances, later ones NaN
    late = sp.family_batch(1, model, family)
    late.process_detection_logs(boot[:1])
    ids = [k for k, _ in sorted(late.landmarks[0].items(), key=lambda kv: kv[1])]
    s0 = late.get_state(0)
    p0 = np.eye(s0.shape[0])
    p0[10, 13] = p0[13, 10] = 5000.0          # (landmarks 0 and 1: each block is fine, the pair is not)
    late.set_member(0, s0, p0, ids)
    two = {"ids": np.array(ids[:2] * 2, np.int32), "poses": np.zeros((4, 6)), "offsets": np.array([0, 2, 4])}
    out = late.process_detection_logs([two], mahal=True)
    assert late.status() == [EKF_ERR_NUMERIC]
    assert np.isfinite(out.mahal[0][:2]).all() and (out.mahal[0][:2] > 0).all() and np.isnan(out.mahal[0][2:]).all()
    # bad gates raise before anything runs, and no member changes
    before, gate0 = sp.snap_batch(ref), ref.gate.copy()
    for g in (np.nan, 0.0, -3.0, -np.inf, [1.0, 2.0], [1.0, np.nan, 3.0]):
        with pytest.raises(ValueError):
            ref.set_gate(g)
        with pytest.raises(ValueError):
            sp.family_batch(3, model, family, gate=g)
    nan = np.full(3, np.nan)
    assert ref.lib.ekf_batch_set_gate(ref.h, nan.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert np.array_equal(ref.gate, gate0)
    sp.assert_same(before, sp.snap_batch(ref), "bad gates", equal_nan=True)
    assert isinstance(EkfError, type)
    ref.set_gate(gate0)
