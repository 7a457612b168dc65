"""Every update-kernel instance against an extended-precision step (``oracle/ekf_extended.py``), componentwise.

Each case is one production step (no debug copies) from a dense random prior restored with ``set_state_cov``: the
case table and the dispatch restatement are in ``update_sweep_util.py`` (``test_update_sweep_cpu.py`` checks that the
table reaches every compiled instance).  One filter per configuration, a fresh prior per case, one reference per
(prior, m) shared by every kernel and path that runs it; an f32 filter starts from its own f32-rounded prior.

Bounds: |P'_gpu - P'_ref| <= c_P (k+1) u M_P and |x'_gpu - x'_ref| <= c_x tau_x M_x (update_sweep_util's docstring
derives them).  The constants (update_sweep_util.C_BOUNDS) are the worst ratios measured per path on an MI355X
(profiles/update_sweep/) times a head-room of at most 8; every ratio goes to ``report``.
"""
import numpy as np
import pytest

import support as sp
import update_sweep_util as sw
from conftest import report

pytestmark = pytest.mark.gpu

C = sw.C_BOUNDS
CASES = sw.sweep_cases()
GROUPS = list(dict.fromkeys(c.group for c in CASES))


@pytest.fixture(scope="module")
def refs():
    return sw.references(sw.ref_key(c) for c in CASES)


def _filter(case):
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    kw = dict(max_landmarks=case.n, max_visible=case.max_visible, cov_dtype=case.dtype, cov_kernel=case.kernel,
              fused=case.fused, lookahead=False)
    if case.model == "rot":
        return EKF_Rotations(sw.INIT, **kw)
    return EKF(sw.INIT, quat_update=case.quat, **kw)


def _step(flt, prior):
    """One production step from the prior; returns (state, P) and checks the capacity padding of cov_t."""
    sp.restore(flt, prior)
    flt.observe(prior[3], prior[4])
    x, p = flt.state, flt.uncertainty
    cov = flt.backend.cov_t.cpu().numpy()
    dims = p.shape[0]
    assert not cov[dims:].any() and not cov[:, dims:].any(), "capacity padding of cov_t is not zero"
    return x, p


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_against_the_extended_reference(group, refs):
    cases = [c for c in CASES if c.group == group]
    filters, worst = {}, {}
    failures = []
    for case in cases:
        key = sw.filter_key(case)
        if key not in filters:
            filters[key] = _filter(case)
        prior, ref = refs[sw.ref_key(case)]
        assert ref["kappa"] <= sw.KAPPA_MAX, (case, ref["kappa"])
        x, p = _step(filters[key], prior)
        assert np.array_equal(p, p.T), case
        r_p, r_x = sw.ratios(ref, p, x, case.dtype)
        w = worst.setdefault(case.dtype, [0.0, 0.0, 0.0, None, None])
        if r_p > w[0]:
            w[0], w[3] = r_p, (case.n, case.m, case.kernel)
        if r_x > w[1]:
            w[1], w[4] = r_x, (case.n, case.m, case.kernel)
        w[2] = max(w[2], ref["kappa"])
        c_p, c_x = C[group][case.dtype]
        if r_p > c_p or r_x > c_x:
            failures.append((case, r_p, r_x))
    for dt, (r_p, r_x, kap, at_p, at_x) in worst.items():
        c_p, c_x = C[group][dt]
        report(f"update_sweep[{group},{dt}]", cases=sum(c.dtype == dt for c in cases), ratio_P=r_p, ratio_x=r_x,
               ratio_P_to_tau=r_p / c_p, ratio_x_to_tau=r_x / c_x, c_P=c_p, c_x=c_x, kappa_max=kap,
               worst_P_at=str(at_p), worst_x_at=str(at_x))
    assert not failures, failures[:5]


def test_intermediates_at_the_nb_boundaries(refs):
    """The NB-boundary cases once more with the debug copies on: L and W against the reference S and A
    (componentwise backward errors, update_sweep_util.backward_ratios), and the step itself bitwise the production run."""
    cases = [c for c in CASES if c.group in ("ekf_fused", "ekf_stage") and c.m in sw.EKF_NB_BOUNDS]
    keys = [sw.ref_key(c) for c in cases]
    fac = sw.references(keys, factors=True)
    filters, worst, mismatch = {}, {}, []
    for case in cases:
        key = sw.filter_key(case)
        if key not in filters:
            prod, dbg = _filter(case), _filter(case)
            dbg.backend.debug_enable_w()
            filters[key] = (prod, dbg)
        prod, dbg = filters[key]
        prior, ref = fac[sw.ref_key(case)]
        x0, p0 = _step(prod, prior)
        x1, p1 = _step(dbg, prior)
        if not (np.array_equal(x0, x1) and np.array_equal(p0, p1)):
            mismatch.append(case)
        r_s, r_w = sw.backward_ratios(ref, dbg.backend.debug_fetch("L", case.m), dbg.backend.debug_fetch("W", case.m),
                                      case.dtype)
        w = worst.setdefault(case.dtype, [0.0, 0.0])
        w[0], w[1] = max(w[0], r_s), max(w[1], r_w)
    for dt, (r_s, r_w) in worst.items():
        c_s, c_w = C["intermediates"][dt]
        report(f"update_sweep[intermediates,{dt}]", ratio_LLt_S=r_s, ratio_LW_A=r_w, ratio_LLt_to_tau=r_s / c_s,
               ratio_LW_to_tau=r_w / c_w)
    assert not mismatch, f"debug run differs from the production run: {mismatch[:4]}"
    for dt, (r_s, r_w) in worst.items():
        c_s, c_w = C["intermediates"][dt]
        assert r_s <= c_s and r_w <= c_w, (dt, r_s, r_w)


@pytest.mark.parametrize("model,ms", [("ekf", sw.EKF_NB_LARGEST), ("rot", sw.ROT_NB_ONE)])
def test_pipelined_sequence_mode_at_every_nb_is_bitwise_the_serial_calls(model, ms):
    """Three frames through observe_sequence (lookahead=True: the pipelined mode) from a dense prior, bitwise the
    per-frame calls of a serial filter, for one m per NB 1..12."""
    import torch
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations, euler_xyz_to_quat
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    make = EKF_Rotations if model == "rot" else EKF
    n = 125 if model == "ekf" else 63
    mv = max(ms)
    for dt in sw.DTYPES:
        pip = make(sw.INIT, max_landmarks=n, max_visible=mv, cov_dtype=dt, lookahead=True)
        ser = make(sw.INIT, max_landmarks=n, max_visible=mv, cov_dtype=dt, lookahead=False)
        for m in ms:
            state, p, lm_ids, ids, poses = sw.dense_prior(model, n, m, 77 + m, dt)
            rng = np.random.default_rng(m)
            frames = [poses + np.hstack((rng.normal(0.0, 0.01, (m, 3)), np.zeros((m, 3)))) for _ in range(3)]
            for flt in (pip, ser):
                sp.restore(flt, (state, p, lm_ids))
            for z in frames:
                ser.observe(ids, z)
            idx = torch.tensor(np.array([ids] * 3), dtype=torch.int32, device="cuda:0")
            if model == "rot":
                zz = np.stack([np.hstack((z[:, :3], euler_xyz_to_quat(z[:, 3:6]))) for z in frames])
            else:
                zz = np.stack([z[:, :3] for z in frames])
            pip.backend.observe_sequence(idx, torch.tensor(zz, dtype=torch.float64, device="cuda:0"))
            assert pip.backend.last_sequence_mode() == "pipelined", (model, dt, m)
            assert np.array_equal(pip.state, ser.state), (model, dt, m)
            assert np.array_equal(pip.uncertainty, ser.uncertainty), (model, dt, m)


def test_batch_members_against_the_extended_reference():
    """One EKFBatch call, 16 members: member j sees m = j detections from its own dense prior, at n = 1, 39 and 82."""
    from aruco_slam_amd.batch import EKFBatch
    keys = [sw.RefKey("ekf", (1, 39, 82)[j % 3], j, "float64", "as_written") for j in range(1, 17)]
    got = sw.references(keys)
    batch = EKFBatch(len(keys), sw.INIT, max_landmarks=82, max_visible=16)
    logs = []
    for b, key in enumerate(keys):
        state, p, lm_ids, ids, poses = got[key][0]
        batch.set_member(b, state, p, lm_ids)
        logs.append({"ids": np.asarray(ids, dtype=np.int32), "poses": poses,
                     "offsets": np.array([0, len(ids)], dtype=np.int64)})
    batch.process_detection_logs(logs)
    worst = np.zeros(2)
    for b, key in enumerate(keys):
        ref = got[key][1]
        assert ref["kappa"] <= sw.KAPPA_MAX
        p = batch.get_cov(b)
        assert np.array_equal(p, p.T)
        worst = np.maximum(worst, sw.ratios(ref, p, batch.get_state(b), "float64"))
    c_p, c_x = C["batch"]["float64"]
    report("update_sweep[batch,float64]", members=len(keys), ratio_P=worst[0], ratio_x=worst[1],
           ratio_P_to_tau=worst[0] / c_p, ratio_x_to_tau=worst[1] / c_x, c_P=c_p, c_x=c_x)
    assert worst[0] <= c_p and worst[1] <= c_x, worst


# ---------------------------------------------------------------------------------------------------------------------
# set_fused + growth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start_fused", [False, True])
@pytest.mark.parametrize("grow_by", ["add_markers", "observe", "set_state_cov"])
def test_set_fused_then_growth_equals_a_filter_built_that_way_and_large(start_fused, grow_by):
    """A filter created with one front-kernel setting, switched with set_fused, then grown past its capacity: the new
    workspace must be sized for the live setting (the second covariance buffer of the pipelined mode exists only for a
    fused filter), and the run bitwise that of a filter built with the final setting and a large capacity."""
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    state, p, lm_ids, ids, poses = sw.dense_prior("ekf", 20, 6, 5)
    big_state, big_p, big_ids, _, big_poses = sw.dense_prior("ekf", 40, 12, 6)
    out = []
    for small in (True, False):
        flt = EKF(sw.INIT, max_landmarks=20 if small else 64, max_visible=6 if small else 16,
                  fused=start_fused if small else not start_fused)
        if small:
            flt.backend.set_fused(not start_fused)
        sp.restore(flt, (state, p, lm_ids))
        flt.observe(ids, poses)
        if grow_by == "add_markers":
            flt.add_marker(1000, np.array([0.3, -0.2, 1.5]))
            flt.observe(ids + [1000], np.vstack((poses, [[0.1, 0.2, 1.4, 0, 0, 0]])))
        elif grow_by == "observe":
            more = list(range(6)) * 2
            flt.observe(more, np.vstack((poses, poses)))
        else:
            sp.restore(flt, (big_state, big_p, big_ids))
            flt.observe(ids + [30, 31], np.vstack((poses, big_poses[:2])))
        out.append((flt.state, flt.uncertainty))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])
