"""Per-detection measurement noise in ``EKFBatch`` (``row_noise=True``; ``"noise"`` in a log, ``observe_indexed(noise=)``)
on an MI355X, for the three window kernels (``gating_util.FAMILIES``) and both models: rows equal to a constant are that
member's ``r_uncertainty`` bit for bit, one teacher-forced step against the extended-precision step with the same rows,
large-map and wide-frame kernels are bitwise the one-column kernel, a one-member batch and its ``to_filter`` give the same
d^2 bits, ``nis`` / ``cam_cov`` stay available; and ``batch.corner_row_noise``."""
import numpy as np
import pytest

import gating_util as gu
import row_noise_util as rn
import support as sp
import update_sweep_util as sw
from conftest import load_npz, report

pytestmark = pytest.mark.gpu

INIT = gu.INIT
ALL = list(gu.FAMILIES)
MODELS = ["ekf", "ekf_rotations"]
QM = {"ekf": "ekf", "ekf_rotations": "rot"}
EXTRA = {"column": {}, "large": {"large_maps": True}, "wide": {"wide_frames": True}}
# teacher-forced members (n, m): one detection, odd widths, a full one-column frame; the wide family adds frames of more
# than one block of 16 / 8 detections
STEP_MEMBERS = {"ekf": [(1, 1), (39, 3), (82, 8), (39, 16)], "ekf_rotations": [(1, 1), (12, 2), (24, 5), (12, 8)]}
STEP_WIDE = {"ekf": [(40, 17), (40, 36)], "ekf_rotations": [(20, 9), (20, 18)]}


def _same_outputs(got, want, what, names=("trajectory", "nis", "cam_cov", "dof", "mahal", "rejected")):
    for name in names:
        for b, (u, v) in enumerate(zip(getattr(got, name), getattr(want, name))):
            assert np.array_equal(u, v, equal_nan=True), (what, name, b)


def _with_rows(model, log, seed):
    return dict(log, noise=rn.log_rows(model, log, seed))


@pytest.mark.parametrize("model,family", ALL)
def test_uniform_rows_are_the_members_constant_bit_for_bit(model, family):
    """Member b's log carries rows all equal to c_b (as [D] or [D, RD]) on a batch of default constants; the twin has
    r_uncertainty = c_b per member and no rows: every output and every member's state and P agree in every bit.  The last
    member has no noise in its log and keeps its own constant."""
    consts = np.array([0.37, 0.6, 1.5, 0.9])
    logs = [gu.clean_log(model, family, seed=s) for s in range(4)]
    rd = gu.RD[model]
    noisy = [dict(lg, noise=np.full(len(lg["ids"]), c) if b % 2 else np.full((len(lg["ids"]), rd), c))
             for b, (lg, c) in enumerate(zip(logs[:3], consts))] + [logs[3]]
    rows = sp.family_batch(4, model, family, row_noise=True)
    got = rows.process_detection_logs(noisy, nis=True, cam_cov=True, mahal=True)
    twin = sp.family_batch(4, model, family, noise={"r_uncertainty": consts})
    want = twin.process_detection_logs(logs, nis=True, cam_cov=True, mahal=True)
    assert rows.status() == twin.status() == [0] * 4
    _same_outputs(got, want, "rows = c")
    sp.assert_same(sp.snap_batch(rows), sp.snap_batch(twin), "rows = c", equal_nan=True)
    plain = sp.family_batch(4, model, family)      # (the rows are not ignored)
    assert not np.array_equal(plain.process_detection_logs(logs)[0], got.trajectory[0])


@pytest.mark.parametrize("model,family", ALL)
def test_one_teacher_forced_step_against_the_extended_reference(model, family):
    """Every member one step from its own dense prior (set_member) with log-uniform rows in [0.3, 3], against
    row_noise_util.extended_step_rows under update_sweep_util.C_BOUNDS["batch"] (kappa(S) <= 1e3 asserted)."""
    from aruco_slam_amd.batch import EKFBatch
    members = STEP_MEMBERS[model] + (STEP_WIDE[model] if family == "wide" else [])
    kw = dict(gu.FAMILIES[(model, family)][0])
    kw.update(max_landmarks=max(n for n, _ in members), max_visible=max(kw["max_visible"], max(m for _, m in members)))
    kw.pop("quat_update", None)
    batch = EKFBatch(len(members), INIT, model=model, row_noise=True, **kw)
    logs, refs = [], []
    for b, (n, m) in enumerate(members):
        key = sw.RefKey(QM[model], n, m, "float64", "as_written")
        state, p, lm_ids, ids, poses = sw.dense_prior(key.model, n, m, sw.prior_seed(key))
        rows = rn.case_rows(key, *rn.WIDE)
        refs.append(rn.extended_step_rows(sw.oracle_at(key.model, state, p, lm_ids), ids, poses, rows))
        batch.set_member(b, state, p, lm_ids)
        logs.append({"ids": np.asarray(ids, np.int32), "poses": poses, "offsets": np.array([0, m], np.int64), "noise": rows})
    batch.process_detection_logs(logs)
    assert batch.status() == [0] * len(members)
    worst = np.zeros(2)
    for b, ref in enumerate(refs):
        assert ref["kappa"] <= sw.KAPPA_MAX, (members[b], ref["kappa"])
        p = batch.get_cov(b)
        assert np.array_equal(p, p.T)
        worst = np.maximum(worst, sw.ratios(ref, p, batch.get_state(b), "float64"))
    c_p, c_x = sw.C_BOUNDS["batch"]["float64"]
    report(f"row_noise_batch[{model},{family}]", members=len(members), ratio_P=worst[0], ratio_x=worst[1], c_P=c_p, c_x=c_x)
    assert worst[0] <= c_p and worst[1] <= c_x, worst


@pytest.mark.parametrize("model", MODELS)
def test_large_and_wide_kernels_are_bitwise_the_one_column_kernel_with_rows(model):
    """A dirty log with rows and a gate that the one-column kernel can run, in all three kernels: the same bits in every
    output, state and P."""
    from aruco_slam_amd.batch import EKFBatch
    logs = [_with_rows(model, gu.dirty_log(model, gu.clean_log(model, "column", seed=s), seed=s)[0], s) for s in range(2)]
    outs = []
    for family in ("column", "large", "wide"):
        kw = dict(gu.FAMILIES[(model, "column")][0], gate=gu.GATES[model], row_noise=True)
        kw.update(EXTRA[family])
        batch = EKFBatch(2, INIT, model=model, **kw)
        outs.append((batch.process_detection_logs(logs, nis=True, cam_cov=True), sp.snap_batch(batch)))
        assert batch.status() == [0, 0]
    assert any(r.any() for r in outs[0][0].rejected)
    for family, (out, snap) in zip(("large", "wide"), outs[1:]):
        _same_outputs(out, outs[0][0], family)
        sp.assert_same(snap, outs[0][1], family, equal_nan=True)


@pytest.mark.parametrize("model,family", ALL)
def test_a_one_member_batch_and_its_to_filter_give_the_same_distances(model, family):
    """From the prior a one-member batch leaves (handed over by to_filter, which carries the capability), one further
    frame with rows: d^2 of the batch and of the filter's replay are the same bits (the one gate core both run; the
    updates behind it are different kernels)."""
    clean = gu.clean_log(model, family, seed=1)
    boot_frames = int(clean["bootstrap_frames"]) + 3
    end = int(clean["offsets"][boot_frames])
    head = {"ids": clean["ids"][:end], "poses": clean["poses"][:end], "offsets": clean["offsets"][:boot_frames + 1]}
    batch = sp.family_batch(1, model, family, row_noise=True, gate=np.inf)
    batch.process_detection_logs([_with_rows(model, head, 1)])
    flt, const = batch.to_filter(0), batch.to_filter(0)
    assert flt.backend.can_row_noise and flt.gate == np.inf
    d1 = int(clean["offsets"][boot_frames + 1])
    ids, poses = clean["ids"][end:d1], clean["poses"][end:d1] + np.array([0.05, -0.03, 0.04, 0, 0, 0])
    rows = np.exp(np.random.default_rng(3).uniform(np.log(0.05), np.log(20.0), (len(ids), gu.RD[model])))
    offsets = np.array([0, len(ids)], np.int64)
    out = batch.process_detection_logs([{"ids": ids, "poses": poses, "offsets": offsets, "noise": rows}], mahal=True)
    _traj, d2 = flt.process_detection_log(ids, poses, offsets, mahal=True, noise=rows)
    assert (out.mahal[0] > 0).all() and np.array_equal(d2, out.mahal[0])
    _t, d2_const = const.process_detection_log(ids, poses, offsets, mahal=True)      # (the rows are not ignored)
    assert d2_const.shape == d2.shape and (d2_const != d2).all()


@pytest.mark.parametrize("model,family", ALL)
def test_nis_and_cam_cov_come_with_rows_and_change_nothing_else(model, family):
    logs = [_with_rows(model, gu.clean_log(model, family, seed=s), s) for s in range(2)]
    bare = sp.family_batch(2, model, family, row_noise=True)
    traj = bare.process_detection_logs(logs)
    full = sp.family_batch(2, model, family, row_noise=True)
    out = full.process_detection_logs(logs, nis=True, cam_cov=True, mahal=True)
    for b in range(2):
        assert np.array_equal(traj[b], out.trajectory[b])
        stepped, boot = out.dof[b] > 0, int(logs[b]["bootstrap_frames"])
        # (a bootstrap frame holds first sightings only: z = h, NIS exactly 0)
        assert np.isfinite(out.nis[b]).all() and (out.nis[b] >= 0).all() and (out.nis[b][~stepped] == 0).all()
        assert (out.nis[b][boot:][stepped[boot:]] > 0).all()
        assert out.cam_cov[b].shape == (len(traj[b]), 10, 10) and np.isfinite(out.cam_cov[b]).all()
        assert np.array_equal(out.cam_cov[b][-1], full.get_cov(b)[:10, :10])
        assert np.isfinite(out.mahal[b]).all()
    sp.assert_same(sp.snap_batch(bare), sp.snap_batch(full), "asking for outputs", equal_nan=True)
    # the rows matter: with rows ten times larger the steady frames' NIS per row is smaller
    big = sp.family_batch(2, model, family, row_noise=True)
    out_big = big.process_detection_logs([dict(lg, noise=10.0 * lg["noise"]) for lg in logs], nis=True)
    t = int(logs[0]["bootstrap_frames"])
    assert 0 < out_big.nis[0][t:].sum() < out.nis[0][t:].sum()


def test_noise_arguments_of_the_batch_are_validated():
    model, family = "ekf", "column"
    log = gu.clean_log(model, family, seed=0)
    plain = sp.family_batch(1, model, family)
    with pytest.raises(ValueError, match="row_noise=True"):
        plain.process_detection_logs([dict(log, noise=np.full(len(log["ids"]), 0.9))])
    batch = sp.family_batch(1, model, family, row_noise=True)
    for bad in (np.full(len(log["ids"]) - 1, 0.9), np.full((len(log["ids"]), 2), 0.9), np.zeros(len(log["ids"])),
                np.full(len(log["ids"]), np.nan)):
        with pytest.raises(ValueError, match="noise"):
            batch.process_detection_logs([dict(log, noise=bad)])
    assert batch.num_landmarks == [0]
    with pytest.raises(ValueError, match="row_noise=True"):
        plain.observe_indexed(np.zeros(1, np.int32), [0, 1], [0, 1], np.zeros((1, 6)), noise=[0.9])
    assert plain.to_filter(0).backend.can_row_noise is False and batch.to_filter(0).backend.can_row_noise is True
    with pytest.raises(ValueError, match="row_noise=True"):
        plain.load_filter(0, batch.to_filter(0))


@pytest.mark.parametrize("model", MODELS)
def test_corner_row_noise_is_the_variance_of_the_replica_z(model):
    from aruco_slam_amd.batch import corner_row_noise, replica_corner_poses, replica_z
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    from aruco_slam_amd.synthetic import corner_log
    cal = load_npz("calibration.npz")
    k, dist = cal["camera_matrix"], cal["dist_coeffs"].reshape(-1)
    log = corner_log(8, (2, 5), 6, 3, k, dist)
    sigma_px, seed, replicas = 1.0, 11, 32
    rows = corner_row_noise(log, sigma_px, seed, replicas, k, dist, 0.16, model)
    d, rd = len(log["ids"]), gu.RD[model]
    assert rows.shape == (d, rd) and np.isfinite(rows).all() and (rows > 0).all()
    poses = replica_corner_poses(log["corners"], sigma_px, seed, k, dist, 0.16, replicas=replicas)
    assert poses.shape == (replicas, d, 6)
    if model == "ekf":
        z = poses[:, :, :3]
    else:
        z = np.concatenate((poses[:, :, :3], euler_xyz_to_quat(poses[:, :, 3:6].reshape(-1, 3)).reshape(replicas, d, 4)), axis=2)
    assert np.array_equal(replica_z(poses, model), z)
    assert np.array_equal(rows, np.var(z, axis=0))
    # depth is the noisy direction, and it grows with distance
    assert (rows[:, 2] > rows[:, 0]).mean() > 0.9
    depth = log["poses_clean"][:, 2]
    far = depth > np.median(depth)
    assert np.median(rows[far, 2]) > np.median(rows[~far, 2])
    # ... and the table is what a batch log and a filter take
    with pytest.raises(ValueError, match="replicas"):
        corner_row_noise(log, sigma_px, seed, 1, k, dist, 0.16, model)
