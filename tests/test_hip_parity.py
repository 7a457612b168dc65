"""GPU parity tests: the HIP path (through the C ABI) against the pinned CPU
oracle and the reference's golden fixtures.  Run with ``-m gpu`` on an MI355X.

Tolerances (relative = max|a-b| / max(1, max|b|)):
  fp64 covariance : 1e-10 per teacher-forced step
  fp32 covariance : 2e-5  per teacher-forced step (P stored/updated in fp32,
                    everything else fp64)
  free-run        : <= 1e-4 (north_star) inside the reference's own chaos
                    horizon (see conftest.chaos_horizon)
"""
import numpy as np
import pytest

import support as sp
from conftest import chaos_horizon, load_npz, rel_err, rel_err_elem, report

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
# Both bounds are set from what was MEASURED on MI355X (profiles/r02_parity_metrics.jsonl), with a
# factor of ~4 of head-room, not from the 1e-4 of north_star:
#   norm-wise  rel_err      = max|a-b| / max(1, max|b|)      (an absolute bound on entries < 1)
#   element-wise rel_err_elem = max_i |a_i-b_i| / max(|b_i|, 1e-3)
# measured per teacher-forced step: fp64 4e-15 / 6e-12; fp32 covariance 1e-7 / 1.3e-5 on (state, P)
# (G2, G5), 6e-7 / 5.4e-5 on the n=1024 variances (G4), 6e-7 / 6e-6 at n=4096 (C5).
STEP_TOL = {"float64": 1e-10, "float32": 2e-6}
ELEM_TOL = {"float64": 1e-9, "float32": 2e-4}


def _ekf(**kw):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    return EKF(INIT, **kw)


def _oracle(**kw):
    from oracle.ekf_numpy import OracleEKF
    return OracleEKF(INIT, **kw)


def _restore_hip(flt, state, cov, lm_ids):
    flt.landmarks = {int(k): i for i, k in enumerate(lm_ids)}
    flt.num_landmarks = len(lm_ids)
    flt.backend.set_state_cov(state, cov)


def _restore_oracle(flt, state, cov, lm_ids):
    flt.state = np.array(state, dtype=np.float64)
    flt.uncertainty = np.array(cov, dtype=np.float64)
    flt.landmarks = {int(k): i for i, k in enumerate(lm_ids)}
    flt.num_landmarks = len(lm_ids)


# ---------------------------------------------------------------------------
def test_loaded_library_is_the_in_tree_one():
    from aruco_slam_amd import hip_backend
    hip_backend.load_library()
    with open("/proc/self/maps") as fh:
        assert "aruco_slam_amd/lib/libekf_slam_hip.so" in fh.read()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_intermediates_one_step(dtype):
    """Jacobian rows, residual, A = H(P+Q), Cholesky factor, whitened panel."""
    g = load_npz("g2_teacher_forced.npz")
    f = 150
    state0, p0, lm_ids = g[f"f{f}_state0"], g[f"f{f}_P0"], g[f"f{f}_lm_ids"]
    ids, poses = list(g[f"f{f}_ids"]), g[f"f{f}_poses"]
    flt = _ekf(max_landmarks=16, max_visible=8, cov_dtype=dtype)
    flt.backend.debug_enable_w()
    _restore_hip(flt, state0, p0, lm_ids)
    p0s = 0.5 * (p0 + p0.T)
    if dtype == "float32":
        p0s = p0s.astype(np.float32).astype(np.float64)
    orc = _oracle(mode="fast")
    _restore_oracle(orc, state0, p0s, lm_ids)
    z, hv, jac, col = orc.measurement_blocks(ids, poses)
    dh = orc.dense_jacobian(jac, col)
    flt.observe(ids, poses)
    m = len(ids)
    k = 3 * m
    assert rel_err(flt.backend.debug_fetch("jac", m), jac.reshape(k, 13)) <= 1e-13
    assert rel_err(flt.backend.debug_fetch("resid", m), z - hv) <= 1e-13
    pq = p0s + np.diag(orc.process_noise_diag())
    a_ref = dh @ pq
    assert rel_err(flt.backend.debug_fetch("A", m), a_ref) <= 1e-13
    s = a_ref @ dh.T + 0.9 * np.eye(k)
    chol = np.linalg.cholesky(0.5 * (s + s.T))
    lfac = flt.backend.debug_fetch("L", m)
    assert rel_err(lfac[:k, :k], chol) <= 1e-12
    assert np.array_equal(lfac[k:, k:], np.eye(lfac.shape[0] - k))
    w_ref = np.linalg.solve(chol, a_ref)
    w = flt.backend.debug_fetch("W", m)
    assert rel_err(w[:k], w_ref) <= 1e-11
    assert np.all(w[k:] == 0.0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_g2_teacher_forced_vs_reference(dtype):
    g = load_npz("g2_teacher_forced.npz")
    worst = np.zeros(4)
    for f in g["frames"]:
        flt = _ekf(max_landmarks=16, max_visible=8, cov_dtype=dtype)
        _restore_hip(flt, g[f"f{f}_state0"], g[f"f{f}_P0"], g[f"f{f}_lm_ids"])
        flt.observe(list(g[f"f{f}_ids"]), g[f"f{f}_poses"])
        assert flt.state.shape == g[f"f{f}_state1"].shape
        p1 = flt.uncertainty
        worst = np.maximum(worst, [rel_err(flt.state, g[f"f{f}_state1"]), rel_err(p1, g[f"f{f}_P1"]),
                                   rel_err_elem(flt.state, g[f"f{f}_state1"]), rel_err_elem(p1, g[f"f{f}_P1"])])
    report(f"g2_teacher_forced[{dtype}]", state_norm=worst[0], cov_norm=worst[1], state_elem=worst[2], cov_elem=worst[3])
    assert worst[0] <= STEP_TOL[dtype] and worst[1] <= STEP_TOL[dtype], worst
    assert worst[2] <= ELEM_TOL[dtype] and worst[3] <= ELEM_TOL[dtype], worst


@pytest.mark.parametrize("dtype,kernel", [("float64", "mfma"), ("float64", "valu"),
                                          ("float32", "mfma"), ("float32", "valu")])
def test_c1_teacher_forced_chain_all_200_frames(dtype, kernel):
    """Every frame of the C1 replay as a single step from the oracle's prior:
    no chaos amplification, so the per-step bound holds on all 200 frames."""
    det = load_npz("c1_detections.npz")
    offs = det["offsets"]
    orc = _oracle(mode="fast")
    flt = _ekf(max_landmarks=16, max_visible=8, cov_dtype=dtype, cov_kernel=kernel)
    worst_s = worst_p = worst_e = 0.0
    for f in range(len(det["timestamps_ms"])):
        if not det["has_detections"][f]:
            continue
        sl = slice(offs[f], offs[f + 1])
        ids, poses = list(det["ids"][sl]), det["poses"][sl]
        if orc.num_landmarks:
            lm_ids = [k for k, _ in sorted(orc.landmarks.items(), key=lambda kv: kv[1])]
            _restore_hip(flt, np.asarray(orc.state, dtype=np.float64), orc.uncertainty, lm_ids)
        orc.observe(ids, poses)
        flt.observe(ids, poses)
        worst_s = max(worst_s, rel_err(flt.state, orc.state))
        worst_p = max(worst_p, rel_err(flt.uncertainty, orc.uncertainty))
        worst_e = max(worst_e, rel_err_elem(flt.state, orc.state), rel_err_elem(flt.uncertainty, orc.uncertainty))
    report(f"c1_teacher_forced_chain[{dtype},{kernel}]", state_norm=worst_s, cov_norm=worst_p, elem=worst_e)
    assert worst_s <= STEP_TOL[dtype] and worst_p <= STEP_TOL[dtype], (worst_s, worst_p)
    assert worst_e <= ELEM_TOL[dtype], worst_e


def _replay_c1(flt):
    det = load_npz("c1_detections.npz")
    offs = det["offsets"]
    cams = []
    for f in range(len(det["timestamps_ms"])):
        ids = det["ids"][offs[f]:offs[f + 1]] if det["has_detections"][f] else None
        _, cam, _, _ = flt.process_detections(ids, det["poses"][offs[f]:offs[f + 1]])
        cams.append(np.asarray(cam[:7], dtype=np.float64).copy())
    return np.stack(cams)


def test_g3_free_run_fp64_within_1e4_inside_chaos_horizon():
    g = load_npz("g3_free_run.npz")
    flt = _ekf(max_landmarks=16, max_visible=8, cov_dtype="float64")
    cams = _replay_c1(flt)
    hz = chaos_horizon(g)
    assert hz >= 120
    err = rel_err(cams[:hz + 1], g["cam"][:hz + 1])
    print(f"fp64 free-run: horizon {hz} frames, rel err {err:.2e}")
    assert err <= 1e-4
    assert np.isfinite(cams).all() and np.abs(cams).max() < 50.0
    assert list(flt.landmarks.keys()) == list(g["lm_ids"])


def test_g3_free_run_fp32_cov_horizon():
    """fp32-stored P: 6e-8 relative rounding per step, amplified by the
    reference's chaos -> the 1e-4 bound holds for a shorter run."""
    g = load_npz("g3_free_run.npz")
    flt = _ekf(max_landmarks=16, max_visible=8, cov_dtype="float32")
    cams = _replay_c1(flt)
    d = np.abs(cams - g["cam"]).max(axis=1)
    first_bad = int(np.argmax(d > 1e-4)) if (d > 1e-4).any() else len(d)
    print(f"fp32-cov free-run: first frame beyond 1e-4 = {first_bad}")
    assert first_bad >= 60
    assert np.isfinite(cams).all()


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 1e-4)])
def test_free_run_200_frames_scalar_first_convention(dtype, tol):
    """With the consistent quaternion convention the filter is not chaotic:
    200 free-running frames agree with the oracle end to end."""
    flt = _ekf(max_landmarks=16, max_visible=8, cov_dtype=dtype, quat_update="scalar_first")
    orc = _oracle(mode="fast", quat_mode="scalar_first")
    cams = _replay_c1(flt)
    det = load_npz("c1_detections.npz")
    offs = det["offsets"]
    ref = []
    for f in range(len(det["timestamps_ms"])):
        if det["has_detections"][f]:
            sl = slice(offs[f], offs[f + 1])
            orc.observe(list(det["ids"][sl]), det["poses"][sl])
        ref.append(np.asarray(orc.state[:7], dtype=np.float64).copy())
    assert rel_err(cams, np.stack(ref)) <= tol
    assert rel_err(flt.state, orc.state) <= tol
    assert rel_err(flt.uncertainty, orc.uncertainty) <= tol


@pytest.mark.parametrize("name,dtype,tol", [("g4_scale_n256.npz", "float64", 1e-8),
                                            ("g4_scale_n1024.npz", "float64", 1e-8),
                                            ("g4_scale_n1024.npz", "float32", 5e-6)])
def test_g4_scale_vs_reference(name, dtype, tol):
    g = load_npz(name)
    n, m = int(g["n"]), int(g["m"])
    flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype=dtype)
    boot = int(g["boot_frames"])
    poses = np.zeros((m, 6))
    for f in range(boot):
        poses[:, :3] = g["z"][f]
        flt.observe(g["ids"][f], poses)
    assert rel_err(flt.state, g["boot_state"]) <= tol
    assert rel_err(flt.backend.get_cov_diag(), g["boot_diag"]) <= tol
    worst = np.zeros(6)
    for j in range(g["states"].shape[0]):
        poses[:, :3] = g["z"][boot + j]
        flt.observe(g["ids"][boot + j], poses)
        st, dg = flt.state, flt.backend.get_cov_diag()
        worst[:4] = np.maximum(worst[:4], [rel_err(st, g["states"][j]), rel_err(dg, g["diags"][j]),
                                           rel_err_elem(st, g["states"][j]), rel_err_elem(dg, g["diags"][j])])
    p = flt.uncertainty
    assert abs(np.linalg.norm(p) - g["fro"][-1]) <= tol * g["fro"][-1]
    for (r, c), blk in zip(g["block_corners"], g["blocks"][-1]):
        worst[4:] = np.maximum(worst[4:], [rel_err(p[r:r + 16, c:c + 16], blk), rel_err_elem(p[r:r + 16, c:c + 16], blk)])
    report(f"g4_scale[{name},{dtype}]", state_norm=worst[0], diag_norm=worst[1], state_elem=worst[2], diag_elem=worst[3],
           blocks_norm=worst[4], blocks_elem=worst[5])
    assert worst[0] <= tol and worst[1] <= tol and worst[4] <= tol, worst
    # element-wise: state and variances (all well above the 1e-3 floor) to the same bound; sampled
    # off-diagonal blocks hold entries down to 1e-6, i.e. mostly the absolute floor
    etol = {"float64": 1e-8, "float32": 2e-4}[dtype]
    assert worst[2] <= etol and worst[3] <= etol and worst[5] <= etol, worst
    assert np.array_equal(p, p.T)          # bitwise symmetric


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mfma_and_valu_kernels_agree_bitwise(dtype):
    """Both covariance kernels run the same k-ordered fma chain (the symmetric
    MFMA kernel computes the lower triangle and mirrors it; the VALU kernel
    computes every element)."""
    from aruco_slam_amd.synthetic import SyntheticStream
    res = []
    for kernel in ("valu", "mfma"):
        s = SyntheticStream(96, 12, seed=5)
        flt = _ekf(max_landmarks=96, max_visible=12, cov_dtype=dtype, cov_kernel=kernel)
        for ids, poses in list(s.bootstrap()) + list(s.steady(3)):
            flt.observe(ids, poses)
        res.append((flt.state, flt.uncertainty))
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])


@pytest.mark.parametrize("n,m", [(300, 5), (300, 16), (520, 37), (700, 64)])
def test_macro_tile_cov_kernel_is_bitwise_the_other_kernels(n, m):
    """f32, large problems: one workgroup per 128 x 128 macro tile, W staged through LDS by LDS-DMA, launch order from a
    host-built table (csrc/ekf_cov_macro.hip; chosen from 1024 macro tiles on, forced here).  Same k-ascending fma chain
    per element and v = (P + q) + acc as the wave-per-tile MFMA kernel and the VALU reference kernel: same bits.  The
    shapes cover whole and half last chunks of W (k = 16, 48, 112, 192 rows) and several per-XCD list lengths."""
    from aruco_slam_amd.synthetic import SyntheticStream
    res = []
    for kernel in ("valu", "mfma_tile", "mfma_macro"):
        s = SyntheticStream(n, m, seed=7)
        flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32", cov_kernel=kernel)
        for ids, poses in list(s.bootstrap()) + list(s.steady(3)):
            flt.observe(ids, poses)
        res.append((flt.state, flt.uncertainty))
    for other in res[1:]:
        assert np.array_equal(res[0][0], other[0])
        assert np.array_equal(res[0][1], other[1])
    assert np.array_equal(res[2][1], res[2][1].T)


def test_macro_tile_cov_kernel_in_the_pipelined_sequence_mode_is_bitwise_the_serial_order():
    """The macro-tile kernel out of place (ping-pong covariance) beside the next frame's front kernel."""
    import torch
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m = 400, 24
    out = []
    for kernel, la in (("mfma_tile", False), ("mfma_macro", True)):
        s = SyntheticStream(n, m, seed=11)
        flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32", cov_kernel=kernel, lookahead=la)
        for ids, poses in s.bootstrap():
            flt.observe(ids, poses)
        frames = list(s.steady(7))
        idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda:0")
        z = torch.tensor(np.stack([f[1][:, :3] for f in frames]), dtype=torch.float64, device="cuda:0")
        flt.backend.observe_sequence(idx, z)
        out.append((flt.state, flt.uncertainty))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


def test_full_size_properties_n1024_fp32():
    """BASELINE headline size: properties that need no oracle run."""
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m = 1024, 32
    s = SyntheticStream(n, m, seed=1)
    flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32")
    flt.backend.debug_enable_w()
    for ids, poses in s.bootstrap():
        flt.observe(ids, poses)
    for ids, poses in s.steady(4):
        flt.observe(ids, poses)
    p_before = flt.uncertainty
    ids, poses = next(iter(s.steady(1)))
    flt.observe(ids, poses)
    p_after = flt.uncertainty
    w = flt.backend.debug_fetch("W", m)[:3 * m]
    # downdate identity: P' + W^T W == P + Q  (fp32 rounding only)
    q = np.full(3 * n + 10, 0.01)
    q[0:3], q[3:7], q[7:10] = 0.3, 0.0, 0.5
    lhs = p_after + w.T @ w
    assert rel_err(lhs, p_before + np.diag(q)) <= 5e-6
    assert np.array_equal(p_after, p_after.T)
    assert (np.diagonal(p_after) > 0).all()
    assert (np.diagonal(p_after) <= np.diagonal(p_before) + q + 1e-6).all()
    # capacity padding stays exactly zero
    cov_t = flt.backend.cov_t
    dims = 3 * n + 10
    assert float(cov_t[dims:, :].abs().max()) == 0.0 and float(cov_t[:, dims:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype,kernel", [("float64", "mfma"), ("float32", "mfma"), ("float32", "valu")])
def test_resident_sequence_entry_matches_per_frame_calls(dtype, kernel):
    """ekf_observe_sequence_device (pipelined mode: the front kernel of frame t+1 beside the covariance
    update of frame t, support entries of P completed inside the front kernel) must give BITWISE the results
    of per-frame observe() calls, also with a landmark detected twice in a frame and with the mode switched off."""
    import torch
    from aruco_slam_amd.synthetic import SyntheticStream
    outs = []
    for mode in ("per_frame", "sequence", "sequence_no_lookahead"):
        s = SyntheticStream(64, 8, seed=2)
        flt = _ekf(max_landmarks=64, max_visible=8, cov_dtype=dtype, cov_kernel=kernel,
                   lookahead=(mode != "sequence_no_lookahead"))   # True forces it on at this size
        for ids, poses in s.bootstrap():
            flt.observe(ids, poses)
        frames = [(ids.copy(), poses.copy()) for ids, poses in s.steady(9)]
        frames[3][0][5] = frames[3][0][1]            # duplicate detection in frame 3
        frames[4][0][:] = frames[4][0][0]            # one landmark seen 8 times (> 4 slot list)
        if mode == "per_frame":
            tr = []
            for ids, poses in frames:
                flt.observe(ids, poses)
                tr.append(flt.state[:7].copy())
            tr = np.stack(tr)
        else:
            idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda")
            z = torch.tensor(np.stack([f[1][:, :3] for f in frames]), dtype=torch.float64,
                             device="cuda")
            traj = torch.zeros((len(frames), 7), dtype=torch.float64, device="cuda")
            flt.backend.observe_sequence(idx[:5], z[:5], traj[:5])     # two calls back to back:
            flt.backend.observe_sequence(idx[5:], z[5:], traj[5:])     # the join must hold
            # (the test must not pass vacuously: the VALU kernel has no pipelined mode, the others must have used it)
            want = "pipelined" if (mode == "sequence" and kernel != "valu") else "serial"
            assert flt.backend.last_sequence_mode() == want
            flt.backend.sync()
            tr = traj.cpu().numpy()
        outs.append((tr, flt.state, flt.uncertainty))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("n,m,dtype", [(160, 40, "float32"), (96, 48, "float64"), (48, 16, "float32")])
def test_pipelined_sequence_mode_beyond_96_rows_is_bitwise_the_serial_order(n, m, dtype):
    """k = 120 / 144: every row of the factorisation publishes its own blocks (no free wave beyond 6 block columns),
    two rows per wave; k = 48: the publishing-wave arrangement with three block columns.  Pipelined mode forced on,
    two calls (odd and even frame counts: the covariance ends in either buffer), one duplicate detection."""
    import torch
    from aruco_slam_amd.synthetic import SyntheticStream
    s = SyntheticStream(n, m, seed=4)
    boot = list(s.bootstrap())
    frames = [(ids.copy(), poses.copy()) for ids, poses in s.steady(13)]
    frames[6][0][3] = frames[6][0][0]
    idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda")
    z = torch.tensor(np.stack([f[1][:, :3] for f in frames]), dtype=torch.float64, device="cuda")
    outs = []
    for mode in (True, False):
        flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype=dtype, lookahead=mode)
        for ids, poses in boot:
            flt.observe(ids, poses)
        traj = torch.zeros((len(frames), 7), dtype=torch.float64, device="cuda")
        for lo, hi in ((0, 5), (5, 13)):
            flt.backend.observe_sequence(idx[lo:hi], z[lo:hi], traj[lo:hi])
        flt.backend.sync()
        outs.append((traj.cpu().numpy(), flt.state, flt.uncertainty))
        del flt
    assert np.isfinite(outs[0][2]).all()
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("m,want", [(6, "pipelined"), (16, "serial")])
def test_sequence_mode_chosen_by_size_for_ekf_rotations(m, want):
    """The size rule (profiles/r03_mode_select.txt): EKF_Rotations pipelines up to k = 64 rows, serial order beyond (its
    pipelined form is slower there); either way the results are those of per-frame calls, bit for bit."""
    import torch
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    from aruco_slam_amd.synthetic import SyntheticStream
    n = 40
    s = SyntheticStream(n, m, seed=4, rvec_sigma=0.05)
    boot = list(s.bootstrap())
    frames = [(ids.copy(), poses.copy()) for ids, poses in s.steady(8)]
    outs = []
    for seq in (True, False):
        flt = _rot(max_landmarks=n, max_visible=m, cov_dtype="float32")
        for ids, poses in boot:
            flt.observe(ids, poses)
        if seq:
            idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda")
            z = np.stack([np.hstack((f[1][:, :3], euler_xyz_to_quat(f[1][:, 3:6]))) for f in frames])
            flt.backend.observe_sequence(idx, torch.tensor(z, dtype=torch.float64, device="cuda"), None)
            assert flt.backend.last_sequence_mode() == want
            flt.backend.sync()
        else:
            for ids, poses in frames:
                flt.observe(ids, poses)
        outs.append((flt.state, flt.uncertainty))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])


def test_pipelined_sequence_mode_at_headline_size_is_bitwise_the_serial_order():
    """n=1024, m=32, f32 covariance: the sequence entry point picks the pipelined mode by itself here (front kernel
    of frame t+1 beside the covariance update of frame t on a second covariance buffer, support entries of P completed
    on the matrix cores from the compact support columns, device-side gates between the two streams).  Three calls back to back (join / restart of the pipeline), a
    duplicate detection and a frame that sees one landmark in every slot; state, covariance and trajectory must be
    the bits of the serial order, and no status bit may be set."""
    import torch
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m = 1024, 32
    s = SyntheticStream(n, m, seed=9)
    boot = list(s.bootstrap())
    frames = [(ids.copy(), poses.copy()) for ids, poses in s.steady(70)]
    frames[11][0][5] = frames[11][0][1]
    frames[40][0][:] = frames[40][0][0]
    idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda")
    z = torch.tensor(np.stack([f[1][:, :3] for f in frames]), dtype=torch.float64, device="cuda")
    outs = []
    for mode in (None, False, True):                 # by size (= pipelined here), never, always
        flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32", lookahead=mode)
        for ids, poses in boot:
            flt.observe(ids, poses)
        traj = torch.zeros((len(frames), 7), dtype=torch.float64, device="cuda")
        for lo, hi in ((0, 30), (30, 31), (31, 70)):
            flt.backend.observe_sequence(idx[lo:hi], z[lo:hi], traj[lo:hi])
        assert flt.backend.last_sequence_mode() == ("serial" if mode is False else "pipelined")
        flt.backend.sync()
        outs.append((traj.cpu().numpy(), flt.state, flt.uncertainty))
        del flt
    assert np.isfinite(outs[0][2]).all()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


def test_error_behaviour():
    """Errors at the boundary: Python exceptions, as in the reference; the C ABI's capacity errors are still there for a caller
    that does not grow (the Python classes do: test_filter_that_outgrows_its_buffers_equals_one_built_large)."""
    import ctypes as C
    from aruco_slam_amd.hip_backend import EkfError
    flt = _ekf(max_landmarks=4, max_visible=2)
    with pytest.raises(ValueError):
        flt.observe([], np.zeros((0, 6)))
    poses = np.tile(np.array([0.1, 0.2, 5.0, 0, 0, 0]), (3, 1))
    hip = flt.backend
    flt.observe([1, 2], poses[:2])
    idx = np.array([0, 1, 1], dtype=np.int32)
    z = np.ascontiguousarray(poses[:, :3])
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = hip.lib.ekf_observe(hip.h, idx.ctypes.data_as(ip), z.ctypes.data_as(dp), 3)      # 3 detections > max_visible
    assert rc == -2 and b"max_visible" in hip.lib.ekf_last_error_string()
    xyz = np.ascontiguousarray(np.tile(poses[:1, :3], (3, 1)))
    rc = hip.lib.ekf_add_markers(hip.h, xyz.ctypes.data_as(dp), None, 3)                    # 2 + 3 landmarks > max_landmarks
    assert rc == -2 and b"max_landmarks" in hip.lib.ekf_last_error_string()
    with pytest.raises(EkfError) as e:
        hip.observe([5], poses[:1, :3])          # index out of range
    assert e.value.code == -1
    flt.observe([1, 2, 3], poses)                # through the class: the filter grows instead
    assert flt.num_landmarks == 3 and hip.max_visible >= 3


def test_add_marker_with_uncertainty_and_duplicates():
    """Restore hook (add_marker with a variance vector) and duplicate ids in
    one frame (two row blocks for one landmark) against the oracle."""
    flt = _ekf(max_landmarks=8, max_visible=6)
    orc = _oracle(mode="fast")
    for obj in (flt, orc):
        obj.add_marker(7, np.array([0.5, -0.2, 4.0, 0, 0, 0]), np.array([0.2, 0.3, 0.4]))
        obj.add_marker(9, np.array([-1.0, 0.4, 6.0, 0, 0, 0]))
    ids = [7, 9, 7, 11]
    poses = np.array([[0.51, -0.2, 4.02, 0, 0, 0], [-1.0, 0.41, 6.0, 0, 0, 0],
                      [0.49, -0.21, 3.99, 0, 0, 0], [2.0, 1.0, 7.0, 0, 0, 0]])
    for _ in range(3):
        flt.observe(ids, poses)
        orc.observe(ids, poses)
    assert rel_err(flt.state, orc.state) <= 1e-10
    assert rel_err(flt.uncertainty, orc.uncertainty) <= 1e-10
    assert rel_err(flt.get_lm_uncertainties(), orc.get_lm_uncertainties()) <= 1e-10


def test_c1_run_slam_outputs_vs_reference_files(tmp_path, golden_dir):
    """C1: `run_slam --filter ekf` on the 200-frame replay; outputs/trajectory.txt and
    outputs/map.txt against the files the reference wrote for the same frames."""
    import argparse
    from aruco_slam_amd.main import run_slam
    args = argparse.Namespace(video="input_video.mp4", filter="ekf",
                              detections=str(golden_dir / "c1_detections.npz"),
                              output_dir=str(tmp_path),
                              filter_kwargs={"max_landmarks": 16, "max_visible": 8})
    run_slam.main(args)
    got_t = (tmp_path / "trajectory.txt").read_text()
    ref_t = (golden_dir / "g3_trajectory.txt").read_text()
    # format: same line count, timestamps and token counts; integer pose before the first marker
    assert got_t.splitlines()[0] == ref_t.splitlines()[0] == "0.0333 0 0 0 1 0 0 0"
    assert [ln.split()[0] for ln in got_t.splitlines()] == [ln.split()[0] for ln in ref_t.splitlines()]
    a, b = sp.parse_trajectory(got_t), sp.parse_trajectory(ref_t)
    assert a.shape == b.shape == (200, 8)
    hz = chaos_horizon(load_npz("g3_free_run.npz"))
    err = rel_err(a[:hz + 1], b[:hz + 1])
    l2 = float(np.sqrt(((a[:hz + 1, 1:4] - b[:hz + 1, 1:4]) ** 2).sum(axis=1)).max())
    print(f"trajectory.txt: {hz + 1} frames inside the reference's chaos horizon, "
          f"rel err {err:.2e}, max position L2 {l2:.2e}")
    assert err <= 1e-4
    # map.txt: same header, ids in the same order; numbers are end-of-run values, i.e.
    # beyond the horizon -> format and ids only, values must be finite
    got_m, ref_m = (tmp_path / "map.txt").read_text(), (golden_dir / "g3_map.txt").read_text()
    assert got_m.splitlines()[:4] == ref_m.splitlines()[:4]
    gi, gx, gu = sp.parse_map(got_m)
    ri, rx, ru = sp.parse_map(ref_m)
    assert gi == ri and gx.shape == rx.shape and gu.shape == ru.shape
    assert np.isfinite(gx).all() and (gu > 0).all()


def test_run_slam_ekf_rotations_outputs_vs_reference_files(tmp_path, golden_dir):
    """f2 end to end: ``run_slam --filter ekf_rotations`` (main/run_slam.py:69-79, 110-143) on the
    120-frame replay; trajectory.txt and map.txt against the files the reference's EKF_Rotations wrote for
    the same frames (tests/golden/make_golden.py g5txt).  This filter uses the consistent quaternion
    convention, so it is not chaotic and the WHOLE run is compared, map values included."""
    import argparse
    from aruco_slam_amd.main import run_slam
    args = argparse.Namespace(video="input_video.mp4", filter="ekf_rotations",
                              detections=str(golden_dir / "g5_detections.npz"), output_dir=str(tmp_path),
                              filter_kwargs={"max_landmarks": 8, "max_visible": 6})
    run_slam.main(args)
    got_t, ref_t = (tmp_path / "trajectory.txt").read_text(), (golden_dir / "g5_trajectory.txt").read_text()
    assert got_t.splitlines()[0] == ref_t.splitlines()[0] == "0.0333 0 0 0 1 0 0 0"
    assert [ln.split()[0] for ln in got_t.splitlines()] == [ln.split()[0] for ln in ref_t.splitlines()]
    a, b = sp.parse_trajectory(got_t), sp.parse_trajectory(ref_t)
    assert a.shape == b.shape == (120, 8)
    got_m, ref_m = (tmp_path / "map.txt").read_text(), (golden_dir / "g5_map.txt").read_text()
    assert got_m.splitlines()[:4] == ref_m.splitlines()[:4]
    lines_g, lines_r = got_m.splitlines()[4:], ref_m.splitlines()[4:]
    assert len(lines_g) == len(lines_r)
    ids_g = [int(lines_g[i]) for i in range(0, len(lines_g) - 2, 4)]
    assert ids_g == [int(lines_r[i]) for i in range(0, len(lines_r) - 2, 4)]
    num = lambda lines, off: np.array([[float(t) for t in lines[i + off].split(", ")]       # noqa: E731
                                       for i in range(0, len(lines) - 2, 4)])
    pose_g, pose_r, unc_g, unc_r = num(lines_g, 1), num(lines_r, 1), num(lines_g, 2), num(lines_r, 2)
    assert pose_g.shape == pose_r.shape == (len(ids_g), 10) and unc_g.shape == unc_r.shape == (len(ids_g), 10)
    errs = dict(traj_norm=rel_err(a, b), traj_elem=rel_err_elem(a, b), map_norm=rel_err(pose_g, pose_r),
                map_elem=rel_err_elem(pose_g, pose_r), unc_norm=rel_err(unc_g, unc_r), unc_elem=rel_err_elem(unc_g, unc_r))
    report("run_slam_ekf_rotations", **errs)
    assert max(errs["traj_norm"], errs["map_norm"], errs["unc_norm"]) <= 1e-9, errs
    assert max(errs["traj_elem"], errs["map_elem"], errs["unc_elem"]) <= 1e-6, errs


def test_c1_map_txt_matches_reference_at_the_horizon(tmp_path, golden_dir):
    """map.txt numbers: stop the replay at the chaos horizon, where the reference still
    reproduces itself, and compare against the oracle's map at that frame (the oracle is
    pinned to the reference on this very run, test_oracle_golden.py)."""
    from aruco_slam_amd.main import run_slam
    hz = chaos_horizon(load_npz("g3_free_run.npz"))
    flt = _ekf(max_landmarks=16, max_visible=8)
    orc = _oracle(mode="fast")
    for f, (ts, ids, poses) in enumerate(run_slam.detection_frames(str(golden_dir / "c1_detections.npz"))):
        if f > hz:
            break
        flt.process_detections(ids, poses)
        if ids is not None:
            orc.observe(list(ids), poses)
    flt.save_map(str(tmp_path / "map.txt"))
    gi, gx, gu = sp.parse_map((tmp_path / "map.txt").read_text())
    assert gi == [k for k, _ in sorted(orc.landmarks.items(), key=lambda kv: kv[1])]
    assert rel_err(gx, orc.state[10:].reshape(-1, 3)) <= 1e-4
    assert rel_err(gu, orc.get_lm_uncertainties()) <= 1e-4


# ---------------------------------------------------------------------------
# EKF_Rotations (ekf_with_rotations.py) on the same kernels: 7 rows / detection, 10-dim landmarks
# ---------------------------------------------------------------------------
def _rot(**kw):
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    return EKF_Rotations(INIT, **kw)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_g5_rotations_teacher_forced_vs_reference(dtype):
    g = load_npz("g5_rotations.npz")
    offs = g["offsets"]
    worst = np.zeros(4)
    for f in g["frames"]:
        flt = _rot(max_landmarks=8, max_visible=6, cov_dtype=dtype)
        _restore_hip(flt, g[f"f{f}_state0"], g[f"f{f}_P0"], g[f"f{f}_lm_ids"])
        sl = slice(offs[f], offs[f + 1])
        flt.observe(list(g["ids"][sl]), g["poses"][sl])
        assert flt.state.shape == g[f"f{f}_state1"].shape
        p1 = flt.uncertainty
        worst = np.maximum(worst, [rel_err(flt.state, g[f"f{f}_state1"]), rel_err(p1, g[f"f{f}_P1"]),
                                   rel_err_elem(flt.state, g[f"f{f}_state1"]), rel_err_elem(p1, g[f"f{f}_P1"])])
    report(f"g5_rotations_teacher_forced[{dtype}]", state_norm=worst[0], cov_norm=worst[1], state_elem=worst[2],
           cov_elem=worst[3])
    assert worst[0] <= STEP_TOL[dtype] and worst[1] <= STEP_TOL[dtype], worst
    assert worst[2] <= ELEM_TOL[dtype] and worst[3] <= ELEM_TOL[dtype], worst


def test_g5_rotations_intermediates():
    from oracle.ekf_numpy import OracleEKFRotations
    g = load_npz("g5_rotations.npz")
    f, offs = 90, g["offsets"]
    flt = _rot(max_landmarks=8, max_visible=6)
    flt.backend.debug_enable_w()
    _restore_hip(flt, g[f"f{f}_state0"], g[f"f{f}_P0"], g[f"f{f}_lm_ids"])
    orc = OracleEKFRotations(INIT, mode="fast")
    p0 = g[f"f{f}_P0"]
    _restore_oracle(orc, g[f"f{f}_state0"], 0.5 * (p0 + p0.T), g[f"f{f}_lm_ids"])
    sl = slice(offs[f], offs[f + 1])
    ids, poses = list(g["ids"][sl]), g["poses"][sl]
    z, hv, jac, col = orc.measurement_blocks(ids, poses)
    flt.observe(ids, poses)
    m = len(ids)
    assert rel_err(flt.backend.debug_fetch("jac", m), jac.reshape(7 * m, 20)) <= 1e-13
    assert rel_err(flt.backend.debug_fetch("resid", m), z - hv) <= 1e-13
    dh = orc.dense_jacobian(jac, col)
    pq = orc.uncertainty + np.diag(orc.process_noise_diag())
    assert rel_err(flt.backend.debug_fetch("A", m), dh @ pq) <= 1e-13
    s = dh @ pq @ dh.T + 0.9 * np.eye(7 * m)
    chol = np.linalg.cholesky(0.5 * (s + s.T))
    assert rel_err(flt.backend.debug_fetch("L", m)[:7 * m, :7 * m], chol) <= 1e-12


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 2e-5)])
def test_g5_rotations_free_run_120_frames_vs_reference(dtype, tol):
    g = load_npz("g5_rotations.npz")
    offs = g["offsets"]
    flt = _rot(max_landmarks=8, max_visible=6, cov_dtype=dtype)
    cams = []
    for f in range(len(g["has_detections"])):
        sl = slice(offs[f], offs[f + 1])
        ids = g["ids"][sl] if g["has_detections"][f] else None
        _, cam, _, _ = flt.process_detections(ids, g["poses"][sl])
        cams.append(np.asarray(cam[:7], dtype=np.float64).copy())
    assert rel_err(np.stack(cams), g["cam"]) <= tol
    assert rel_err(flt.state, g["final_state"]) <= tol
    assert rel_err(flt.uncertainty, g["final_P"]) <= tol
    assert rel_err(flt.get_lm_uncertainties(), np.diagonal(g["final_P"])[10:].reshape(-1, 10)) <= tol
    assert list(flt.landmarks.keys()) == list(g["lm_ids"])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rotations_sequence_entry_matches_per_frame_calls(dtype):
    """Model 1 through ekf_observe_sequence_device, with and without the cross-frame lookahead
    (10 priority rows per next-frame landmark): bitwise the per-frame results."""
    import torch
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    from aruco_slam_amd.synthetic import SyntheticStream
    outs = []
    for mode in ("per_frame", "sequence", "sequence_no_lookahead"):
        s = SyntheticStream(40, 8, seed=4, rvec_sigma=0.05)
        flt = _rot(max_landmarks=40, max_visible=8, cov_dtype=dtype,
                   lookahead=(mode != "sequence_no_lookahead"))
        for ids, poses in s.bootstrap():
            flt.observe(ids, poses)
        frames = [(ids.copy(), poses.copy()) for ids, poses in s.steady(7)]
        frames[2][0][5] = frames[2][0][1]            # duplicate detection
        frames[3][0][:] = frames[3][0][0]            # one landmark seen 8 times
        if mode == "per_frame":
            tr = []
            for ids, poses in frames:
                flt.observe(ids, poses)
                tr.append(flt.state[:7].copy())
            tr = np.stack(tr)
        else:
            idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda")
            z = np.stack([np.hstack((f[1][:, :3], euler_xyz_to_quat(f[1][:, 3:6]))) for f in frames])
            z = torch.tensor(z, dtype=torch.float64, device="cuda")
            traj = torch.zeros((len(frames), 7), dtype=torch.float64, device="cuda")
            flt.backend.observe_sequence(idx[:4], z[:4], traj[:4])
            flt.backend.observe_sequence(idx[4:], z[4:], traj[4:])
            flt.backend.sync()
            tr = traj.cpu().numpy()
        outs.append((tr, flt.state, flt.uncertainty))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


def test_rotations_vs_oracle_n100_fp32_and_fp64():
    """Model 1 at a size the reference cannot reach in reasonable time (dims 1010, k = 112):
    20 steady frames against the NumPy restatement (pinned by G5)."""
    from oracle.ekf_numpy import OracleEKFRotations
    from aruco_slam_amd.synthetic import SyntheticStream
    for dtype, tol in (("float64", 1e-9), ("float32", 5e-5)):
        s = SyntheticStream(100, 16, seed=9, rvec_sigma=0.05)
        flt = _rot(max_landmarks=100, max_visible=16, cov_dtype=dtype)
        orc = OracleEKFRotations(INIT, mode="fast")
        frames = list(s.bootstrap()) + list(s.steady(20))
        for ids, poses in frames:
            flt.observe(ids, poses)
            orc.observe(list(ids), poses)
        assert rel_err(flt.state, orc.state) <= tol
        assert rel_err(flt.uncertainty, orc.uncertainty) <= tol
        p = flt.uncertainty
        assert np.array_equal(p, p.T)


@pytest.mark.parametrize("make,dtype", [(_ekf, "float64"), (_ekf, "float32"), (_rot, "float32")])
def test_checkpoint_resume_is_bitwise(tmp_path, make, dtype):
    """save_checkpoint / load_checkpoint: a filter restored mid-run continues
    bitwise like the one that never stopped."""
    from aruco_slam_amd.synthetic import SyntheticStream
    s = SyntheticStream(24, 6, seed=5, rvec_sigma=0.05)
    frames = list(s.bootstrap()) + list(s.steady(12))
    a = make(max_landmarks=24, max_visible=6, cov_dtype=dtype)
    for ids, poses in frames[:9]:
        a.observe(ids, poses)
    a.save_checkpoint(str(tmp_path / "ck.npz"))
    b = make(max_landmarks=24, max_visible=6, cov_dtype=dtype)
    b.load_checkpoint(str(tmp_path / "ck.npz"))
    assert b.landmarks == a.landmarks and b.num_landmarks == a.num_landmarks
    for ids, poses in frames[9:]:
        a.observe(ids, poses)
        b.observe(ids, poses)
    assert np.array_equal(a.state, b.state)
    assert np.array_equal(a.uncertainty, b.uncertainty)
    with pytest.raises(ValueError):
        other = _rot if make is _ekf else _ekf
        other(max_landmarks=24, max_visible=6).load_checkpoint(str(tmp_path / "ck.npz"))


# ---------------------------------------------------------------------------
# fused front kernel (ekf_front_impl.h) vs the three separate launches (cfg.flags bit 2)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("make,n,m,dtype", [(_ekf, 24, 8, "float64"), (_ekf, 24, 8, "float32"),
                                            (_ekf, 256, 16, "float64"), (_ekf, 1024, 32, "float32"),
                                            (_ekf, 128, 64, "float32"),      # k = 192: 12 block columns of 16, streamed factorisation
                                            (_ekf, 64, 20, "float32"),       # k = 60: 4 block columns (chain-wave factorisation, one row per worker)
                                            (_ekf, 64, 26, "float64"),       # k = 78: 5
                                            (_ekf, 96, 38, "float32"),       # k = 114: 8 (sv_factor: the chain on the row's owner)
                                            (_ekf, 96, 46, "float32"),       # k = 138: 9 block columns, the streamed factorisation
                                            (_ekf, 96, 50, "float64"),       # k = 150: 10
                                            (_ekf, 200, 57, "float32"),      # k = 171: 11
                                            (_rot, 40, 21, "float32"),       # EKF_Rotations k = 147: 10
                                            (_rot, 20, 6, "float64"), (_rot, 40, 27, "float32")])
def test_fused_front_kernel_is_bitwise_the_separate_launches(make, n, m, dtype):
    from aruco_slam_amd.synthetic import SyntheticStream
    outs = []
    for fused in (True, False):
        s = SyntheticStream(n, m, seed=1, rvec_sigma=0.05)
        flt = make(max_landmarks=n, max_visible=m, cov_dtype=dtype, fused=fused)
        for ids, poses in list(s.bootstrap()) + list(s.steady(5)):
            flt.observe(ids, poses)
        flt.observe(ids[:max(1, m // 3)], poses[:max(1, m // 3)])      # smaller k after a larger one
        flt.observe(ids, poses)
        outs.append((flt.state, flt.uncertainty))
    assert np.isfinite(outs[0][0]).all()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("make,n,m,tol", [(_ekf, 128, 64, 1e-9), (_rot, 40, 27, 1e-9)])
def test_k192_vs_oracle(make, n, m, tol):
    """Largest innovation the fused front kernel takes (k = 192 / 189: 12 block columns of 16 through the streamed
    factorisation of ekf_solve_big.h)."""
    from oracle.ekf_numpy import OracleEKF, OracleEKFRotations
    from aruco_slam_amd.synthetic import SyntheticStream
    s = SyntheticStream(n, m, seed=3, rvec_sigma=0.05)
    flt = make(max_landmarks=n, max_visible=m) if make is _rot else make(max_landmarks=n, max_visible=m,
                                                                        quat_update="scalar_first")
    orc = OracleEKFRotations(INIT, mode="fast") if make is _rot else OracleEKF(INIT, mode="fast",
                                                                             quat_mode="scalar_first")
    for ids, poses in list(s.bootstrap()) + list(s.steady(6)):
        flt.observe(ids, poses)
        orc.observe(list(ids), poses)
    assert rel_err(flt.state, orc.state) <= tol
    assert rel_err(flt.uncertainty, orc.uncertainty) <= tol


def test_large_k_runs_are_repeatable_bitwise():
    """n=512, m=64 (k = 192, the 128-register instantiation of the covariance update, the streamed
    factorisation with its chain / publisher / worker waves), f32 covariance: three independent runs of the same frames give the same bits (the
    kernels that count their own loads or poll other workgroups leave no room for timing effects)."""
    from aruco_slam_amd.synthetic import SyntheticStream
    outs = []
    for _ in range(3):
        s = SyntheticStream(512, 64, seed=11)
        flt = _ekf(max_landmarks=512, max_visible=64, cov_dtype="float32")
        for ids, poses in list(s.bootstrap()) + list(s.steady(12)):
            flt.observe(ids, poses)
        outs.append((flt.state, flt.uncertainty))
    assert np.isfinite(outs[0][1]).all()
    for other in outs[1:]:
        assert np.array_equal(outs[0][0], other[0])
        assert np.array_equal(outs[0][1], other[1])


def test_c5_size_back_to_back_frames_fused_vs_separate_launches():
    """n=4096, m=64 (C5): the front kernel has more workgroups than the GPU has CUs (late-starting
    chunks), the factorisation streams 12 block columns (history blocks re-read from the exchange buffer,
    tag-checked), every bounded wait is long; 40 frames back to back through the sequence entry
    point, one filter at a time, must give the bits of the separate launches.  ``fused=True`` IS the
    fused kernel at this size (round 1 silently fell back to the stage kernels here)."""
    import torch
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m = 4096, 64
    s = SyntheticStream(n, m, seed=0)
    boot = list(s.bootstrap())
    frames = list(s.steady(40))
    idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda")
    z = torch.tensor(np.stack([f[1][:, :3] for f in frames]), dtype=torch.float64, device="cuda")
    outs = []
    for fused in (True, False, True):
        flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32", fused=fused)
        assert flt.backend.fused is fused
        for ids, poses in boot:
            flt.observe(ids, poses)
        flt.backend.observe_sequence(idx, z, None)
        flt.backend.sync()
        outs.append((flt.state, flt.backend.get_cov_diag()))
        del flt
    for other in outs[1:]:
        assert np.array_equal(outs[0][0], other[0])
        assert np.array_equal(outs[0][1], other[1])


@pytest.mark.parametrize("quat", ["scalar_first", "as_written"])
def test_c5_full_size_properties_and_oracle_steps(quat):
    """(Both quaternion conventions: `as_written` is the reference's own, extended_kalman_filter.py:138-149; teacher-forced
    steps from a common (state, P) do not amplify its chaos.)
    BASELINE configs[4] (n=4096, m=64, N=12298, k=192, f32 covariance) through the fused front kernel:
    (i) properties of one update at full size -- downdate identity P' + W^T W = P + Q with the debug copy
    of W, bitwise symmetry, zero capacity padding, variances positive and not growing beyond P + Q;
    (ii) three steady frames against the CPU oracle (fast mode) started from the SAME (state, P): the
    bootstrap (128 frames of 32 new markers... here 64 frames of 64) runs on the GPU only -- the oracle's
    add_marker reallocates N x N per marker -- and its result is handed to the oracle, so the comparison
    covers the steady-state frames, the thing C5 is about (reference: extended_kalman_filter.py:95-156,
    2 N^3 = 3.7 TF per frame there)."""
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m = 4096, 64
    dims = 3 * n + 10
    s = SyntheticStream(n, m, seed=5)
    flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32", quat_update=quat)
    assert flt.backend.fused is True
    flt.backend.debug_enable_w()
    for ids, poses in s.bootstrap():
        flt.observe(ids, poses)
    steady = [(ids.copy(), poses.copy()) for ids, poses in s.steady(6)]
    for ids, poses in steady[:2]:
        flt.observe(ids, poses)
    state0, p0 = flt.state, flt.uncertainty
    # ---- (ii) oracle from the same prior
    orc = _oracle(mode="fast", quat_mode=quat)
    _restore_oracle(orc, state0, p0, list(range(n)))
    q = np.full(dims, 0.01)
    q[0:3], q[3:7], q[7:10] = 0.3, 0.0, 0.5
    worst = np.zeros(4)
    for t, (ids, poses) in enumerate(steady[2:5]):
        flt.observe(ids, poses)
        orc.observe(list(ids), poses)
        st, dg = flt.state, flt.backend.get_cov_diag()
        od = np.diagonal(orc.uncertainty)
        worst = np.maximum(worst, [rel_err(st, orc.state), rel_err(dg, od), rel_err_elem(st, orc.state),
                                   rel_err_elem(dg, od)])
        if t == 0:
            # ---- (i) properties of this update
            p1 = flt.uncertainty
            w = flt.backend.debug_fetch("W", m)[:3 * m]
            lhs = p1 + w.T @ w
            ident = rel_err(lhs, p0 + np.diag(q))
            del lhs
            assert ident <= 5e-6, ident
            assert np.array_equal(p1, p1.T)
            d1 = np.diagonal(p1)
            assert (d1 > 0).all() and (d1 <= np.diagonal(p0) + q + 1e-6).all()
            cov_t = flt.backend.cov_t
            assert float(cov_t[dims:, :].abs().max()) == 0.0 and float(cov_t[:, dims:].abs().max()) == 0.0
            full = rel_err(p1, orc.uncertainty)
            assert full <= 5e-6, full
            del p1
    report(f"c5_oracle_steps[float32,{quat}]", state_norm=worst[0], diag_norm=worst[1], state_elem=worst[2], diag_elem=worst[3],
           downdate_identity=ident, cov_norm_step1=full)
    assert worst[0] <= 5e-6 and worst[1] <= 5e-6, worst          # measured 3e-9 / 6e-7 (as_written: 4e-9 / 4e-7)
    # element-wise (floor 1e-3): scalar_first measured 2e-7 / 6e-6; as_written 5e-7 / 1.9e-4 (the as-written filter has
    # drifted by then -- SURVEY F5 -- and its small variances are a few f32 ulps of the large ones they are differences of)
    assert worst[2] <= 5e-5 and worst[3] <= (5e-5 if quat == "scalar_first" else 8e-4), worst


@pytest.mark.parametrize("make,n,m,dtype", [(_ekf, 300, 20, "float32"), (_ekf, 128, 64, "float64"), (_rot, 40, 12, "float32")])
def test_stage_and_fused_frames_alternate_inside_one_filter(make, n, m, dtype):
    """A filter may switch between the fused front kernel and the stage kernels between any two frames
    (ekf_set_fused).  The exchange bookkeeping (buffer parity, frame tags, chunk counter of the
    EKF_Rotations injection) advances with the FUSED frames only; round 1 advanced it with every frame, so
    an odd number of stage frames left the next fused frame on a buffer that still held an older
    frame's factor.  Alternating run == all-stage run, bit for bit, and no stale-exchange status."""
    from aruco_slam_amd.synthetic import SyntheticStream
    pattern = [True, False, True, True, False, False, False, True, False, True, True, True, False, True]
    outs = []
    for alternate in (True, False):
        s = SyntheticStream(n, m, seed=7, rvec_sigma=0.05)
        flt = make(max_landmarks=n, max_visible=m, cov_dtype=dtype, fused=False)
        for ids, poses in s.bootstrap():
            flt.observe(ids, poses)
        for fused, (ids, poses) in zip(pattern, s.steady(len(pattern))):
            flt.backend.set_fused(fused and alternate)
            mm = m if fused else max(1, m // 2)              # the visible count changes as well
            flt.observe(ids[:mm], poses[:mm])
        flt.backend.sync()
        outs.append((flt.state, flt.uncertainty))
    assert np.isfinite(outs[0][0]).all()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("make", ["_ekf", "_rot"])
def test_state_getter_after_observe_reads_the_host_mirror_of_the_device_state(make):
    """A state getter that directly follows a per-frame observe waits for the front part of the frame only and takes the
    state from the pinned host mirror the injection code writes (no device-to-host copy): it must be the device's state,
    bit for bit -- also right after new markers (slow path, then mirror again), for both filters, and the covariance
    getter behind it must see the finished update."""
    import torch
    from aruco_slam_amd.synthetic import SyntheticStream
    rot = make == "_rot"
    n, m = (40, 8)
    flt = (_rot if rot else _ekf)(max_landmarks=n, max_visible=m, cov_dtype="float32")
    s = SyntheticStream(n, m, seed=11, rvec_sigma=0.05 if rot else 0.0)
    frames = list(s.bootstrap()) + list(s.steady(6))
    for ids, poses in frames:
        flt.observe(ids, poses)
        got = flt.state                                   # (event wait + mirror, or the copy path after add_markers)
        torch.cuda.synchronize()
        dev = flt.backend.state_t[:got.size].cpu().numpy()
        assert np.array_equal(got, dev)
        cam, marks = flt.get_poses()
        assert np.array_equal(np.concatenate([cam, marks.reshape(-1)]), dev)
    p = flt.uncertainty
    assert np.array_equal(p, p.T) and np.isfinite(p).all()


def test_device_resident_bad_index_is_clamped_and_reported():
    """ekf_observe_device / ekf_observe_sequence_device cannot range-check resident indices on the host:
    the kernels clamp them (no out-of-bounds access) and the next synchronising call returns
    EKF_ERR_INVALID, for the fused and for the stage kernels; a clean filter is unaffected."""
    import torch
    from aruco_slam_amd.hip_backend import EkfError
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m = 64, 8
    for fused in (True, False):
        s = SyntheticStream(n, m, seed=2)
        flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32", fused=fused)
        for ids, poses in s.bootstrap():
            flt.observe(ids, poses)
        frames = list(s.steady(3))
        idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda")
        z = torch.tensor(np.stack([f[1][:, :3] for f in frames]), dtype=torch.float64, device="cuda")
        flt.backend.observe_sequence(idx[:1], z[:1], None)
        flt.backend.sync()                                   # clean so far
        idx[1, 3] = n + 1000                                 # far outside the state
        idx[2, 0] = -5
        flt.backend.observe_sequence(idx[1:], z[1:], None)
        with pytest.raises(EkfError) as e:
            flt.backend.sync()
        assert e.value.code == -1 and "index" in str(e.value)
        with pytest.raises(EkfError):                        # sticky until reset
            flt.backend.get_state()


def test_map_file_restore_on_the_hip_filter_vs_oracle(golden_dir):
    """f4: ``EKF(init, map_file=...)`` -> BaseFilter.load_map -> add_marker(id, pose, uncertainty) on the
    real filter (base_filter.py:249-272 as intended, extended_kalman_filter.py:279-285), against the oracle
    fed the same add_marker sequence; then a few observe steps on the restored map, one of them with
    a marker the map does not hold."""
    from aruco_slam_amd.filters.base_filter import BaseFilter
    path = str(golden_dir / "g3_map.txt")
    flt = _ekf(max_landmarks=16, max_visible=8, map_file=path)

    class _Feed(BaseFilter):                                  # load_map's parser -> oracle.add_marker
        def __init__(self, orc):
            self.orc = orc

        def add_marker(self, idx, pose, uncertainty=None):
            self.orc.add_marker(idx, pose, uncertainty)

    orc = _oracle(mode="fast")
    _Feed(orc).load_map(path)
    g = load_npz("g3_free_run.npz")
    assert list(flt.landmarks.items()) == list(orc.landmarks.items())
    assert [k for k, _ in flt.landmarks.items()] == list(g["lm_ids"])
    assert np.array_equal(flt.state, np.asarray(orc.state, dtype=np.float64))
    assert np.array_equal(flt.uncertainty, orc.uncertainty)
    det = load_npz("c1_detections.npz")
    offs = det["offsets"]
    steps = 0
    for f in range(len(det["timestamps_ms"])):
        if not det["has_detections"][f]:
            continue
        sl = slice(offs[f], offs[f + 1])
        ids, poses = list(det["ids"][sl]), det["poses"][sl].copy()
        if steps == 2:
            ids = ids + [49]                                  # a marker the map does not know
            poses = np.vstack([poses, [[0.3, -0.2, 4.0, 0, 0, 0]]])
        flt.observe(ids, poses)
        orc.observe(ids, poses)
        assert rel_err(flt.state, orc.state) <= 1e-10
        assert rel_err(flt.uncertainty, orc.uncertainty) <= 1e-10
        steps += 1
        if steps == 5:
            break
    assert flt.num_landmarks == orc.num_landmarks == len(g["lm_ids"]) + 1


@pytest.mark.gpu
def test_pose_front_end_kernel_vs_oracle_and_projected_poses():
    """f3: ekf_estimate_poses (batched IPPE-square, csrc/ekf_pose_ippe.hip) against the NumPy restatement
    (oracle/ippe_numpy.py) on the same corners, and against the poses the corners were projected from through the
    reference's calibrated camera (tests/golden/calibration.npz).  Parity unpinned: no OpenCV here, no fixture of
    the reference covers cv2.solvePnP (base_filter.py:157-165)."""
    from scipy.spatial.transform import Rotation
    from aruco_slam_amd import hip_backend
    from aruco_slam_amd.filters.base_filter import BaseFilter
    from conftest import synthetic_marker_views
    from oracle.ippe_numpy import estimate_pose_of_markers
    k, dist, corners, tvecs, rots = synthetic_marker_views(500, seed=2)
    got = hip_backend.estimate_poses(corners, 0.16, k, dist)
    want = estimate_pose_of_markers(corners, 0.16, k, dist)
    assert got.shape == (500, 6) and np.isfinite(got).all()
    assert np.abs(got[:, :3] - want[:, :3]).max() <= 1e-9
    for j in range(len(corners)):
        assert np.abs((Rotation.from_rotvec(got[j, 3:]) * Rotation.from_rotvec(want[j, 3:]).inv()).as_rotvec()).max() <= 1e-9
        assert np.abs(got[j, :3] - tvecs[j]).max() <= 5e-5 * np.linalg.norm(tvecs[j])
        assert np.abs((Rotation.from_rotvec(got[j, 3:]) * rots[j].inv()).as_rotvec()).max() <= 5e-5
    # through the filter boundary, with corners as cv2's detector returns them (one float32 [1,4,2] array per marker)
    flt = BaseFilter.__new__(BaseFilter)
    flt.calib_matrix, flt.dist_coeffs = k, dist.reshape(1, -1)
    cv_corners = [c.astype(np.float32).reshape(1, 4, 2) for c in corners[:7]]
    poses = flt.estimate_pose_of_markers(cv_corners, np.arange(7), 0.16)
    ref32 = estimate_pose_of_markers(np.stack(cv_corners).astype(np.float64), 0.16, k, dist)
    assert poses.shape == (7, 6) and np.abs(poses - ref32).max() <= 1e-8
    assert flt.estimate_pose_of_markers([], np.arange(0), 0.16).shape == (0, 6)
    with pytest.raises(hip_backend.EkfError) as e:
        hip_backend.estimate_poses(corners[:2], 0.16, k, np.zeros(9))          # 9 distortion coefficients
    assert e.value.code == -1


# ---------------------------------------------------------------------------
# capacity that follows the reference (extended_kalman_filter.py:274-290: arrays grow without limit)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("make,dtype", [("_ekf", "float64"), ("_ekf", "float32"), ("_rot", "float32")])
def test_filter_that_outgrows_its_buffers_equals_one_built_large(make, dtype):
    """A filter constructed for 8 landmarks / 4 detections per frame that meets 20 markers and frames of up to 9 detections
    moves into larger buffers (ekf_grow: new tensors from ekf_query_sizes, device-to-device copy, re-bind) instead of
    failing with EKF_ERR_CAPACITY -- and continues BIT FOR BIT like a filter that was built for 32 / 16 from the start."""
    from aruco_slam_amd.synthetic import SyntheticStream
    maker = {"_ekf": _ekf, "_rot": _rot}[make]
    outs = []
    for cap, vis in ((8, 4), (32, 16)):
        rng = np.random.default_rng(4)
        s = SyntheticStream(20, 4, seed=12, rvec_sigma=0.05 if make == "_rot" else 0.0)
        flt = maker(max_landmarks=cap, max_visible=vis, cov_dtype=dtype)
        seen = []
        for t in range(26):
            m = int(rng.integers(2, 10))
            known = min(20, 3 + t)                       # markers appear progressively: several growth steps
            ids = np.sort(rng.choice(known, min(m, known), replace=False))
            if t >= 20:
                ids = np.unique(np.concatenate([ids[:-1], [16 + (t - 20) % 4]]))      # (every marker is seen at least once)
            ids_f, poses = s._observe(ids)
            flt.observe(ids_f, poses)
            seen.append(flt.state[:7].copy())
        assert flt.num_landmarks == 20
        assert flt.backend.max_landmarks >= 20 and flt.backend.max_visible >= 9
        outs.append((np.stack(seen), flt.state, flt.uncertainty, flt.get_lm_uncertainties()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_default_capacity_follows_the_dictionary():
    """EKF(initial_pose, aruco_dict) as the reference constructs it (extended_kalman_filter.py:40-43): the first buffers are
    sized for the dictionary's marker count (DICT_5X5_50 by default, base_filter.py:81-82)."""
    assert _ekf().backend.max_landmarks == 50
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    assert EKF(INIT, 6).backend.max_landmarks == 250          # cv2.aruco.DICT_5X5_250
    assert _rot().backend.max_landmarks == 50


@pytest.mark.parametrize("make", ["_ekf", "_rot"])
def test_sticky_device_error_recovers_through_reset_and_load_checkpoint(tmp_path, make):
    """A device-side error (here: a landmark index out of range in a device-resident detection array, raised by the kernels)
    is sticky: every synchronising call reports it until ekf_reset.  The way back is reset() + load_checkpoint(): the
    restored filter continues bit for bit like one that never failed."""
    import torch
    from aruco_slam_amd.hip_backend import EkfError
    from aruco_slam_amd.synthetic import SyntheticStream
    maker = {"_ekf": _ekf, "_rot": _rot}[make]
    rot = make == "_rot"
    s = SyntheticStream(24, 6, seed=8, rvec_sigma=0.05 if rot else 0.0)
    frames = list(s.bootstrap()) + list(s.steady(8))
    good = maker(max_landmarks=24, max_visible=6, cov_dtype="float64")
    bad = maker(max_landmarks=24, max_visible=6, cov_dtype="float64")
    for ids, poses in frames[:6]:
        good.observe(ids, poses)
        bad.observe(ids, poses)
    ck = tmp_path / "ck.npz"
    bad.save_checkpoint(str(ck))
    # poison: one resident frame with an index beyond the map
    rd = 7 if rot else 3
    idx = torch.tensor([[0, 1, 2, 3, 4, 99]], dtype=torch.int32, device="cuda")
    z = torch.zeros((1, 6, rd), dtype=torch.float64, device="cuda")
    if rot:
        z[:, :, 3] = 1.0
    bad.backend.observe_sequence(idx, z)
    with pytest.raises(EkfError) as err:
        bad.backend.sync()
    assert err.value.code == -1                      # EKF_ERR_INVALID, reported by the kernels
    with pytest.raises(EkfError):                    # ... and sticky
        bad.backend.get_state()
    bad.reset()
    assert bad.num_landmarks == 0
    bad.load_checkpoint(str(ck))
    for ids, poses in frames[6:]:
        good.observe(ids, poses)
        bad.observe(ids, poses)
    assert np.array_equal(good.state, bad.state)
    assert np.array_equal(good.uncertainty, bad.uncertainty)


def test_only_one_handle_of_a_process_pipelines_at_a_time():
    """Two filters with pipelined sequence calls in flight: the device-side gates of two handles could wait for each other
    across the hardware queues HIP multiplexes its streams onto, so the second handle runs its call in serial
    order -- same bits -- and says so; once the first handle has been synchronised the second one may pipeline."""
    import torch
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m = 300, 16
    filters, data = [], []
    for seed in (1, 2):
        s = SyntheticStream(n, m, seed=seed)
        flt = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32", lookahead=True)
        for ids, poses in s.bootstrap():
            flt.observe(ids, poses)
        fr = list(s.steady(400))
        idx = torch.tensor(np.stack([f[0] for f in fr]), dtype=torch.int32, device="cuda")
        z = torch.tensor(np.stack([f[1][:, :3] for f in fr]), dtype=torch.float64, device="cuda")
        flt.backend.sync()
        filters.append(flt)
        data.append((idx, z, fr))
    a, b = filters
    a.backend.observe_sequence(data[0][0], data[0][1])           # 400 frames in flight ...
    b.backend.observe_sequence(data[1][0], data[1][1])           # ... when the second handle asks
    assert a.backend.last_sequence_mode() == "pipelined"
    assert b.backend.last_sequence_mode() in ("serial (another handle of the process is pipelining)", "pipelined")
    a.backend.sync()
    b.backend.sync()
    b.backend.observe_sequence(data[1][0][:4], data[1][1][:4])
    assert b.backend.last_sequence_mode() == "pipelined"
    b.backend.sync()
    # same bits as a run that never pipelined
    ref = _ekf(max_landmarks=n, max_visible=m, cov_dtype="float32", lookahead=False)
    s = SyntheticStream(n, m, seed=2)
    for ids, poses in s.bootstrap():
        ref.observe(ids, poses)
    ref.backend.observe_sequence(data[1][0], data[1][1])
    ref.backend.observe_sequence(data[1][0][:4], data[1][1][:4])
    assert np.array_equal(ref.state, b.state)
    assert np.array_equal(ref.uncertainty, b.uncertainty)


def test_rotations_with_all_50_markers_of_the_dictionary_in_view_vs_oracle():
    """EKF_Rotations with every marker of DICT_5X5_50 detected in a frame: k = 7 x 50 = 350 measurement rows, 22 block
    columns of S (the reference takes any number of detections, ekf_with_rotations.py:115-181; rounds 1 - 2 stopped at 27).
    The streamed factorisation (csrc/ekf_solve_big.h) through the stage kernels, f64, against the oracle; the filter was
    built for 27 detections per frame and grows."""
    from aruco_slam_amd.synthetic import SyntheticStream
    from oracle.ekf_numpy import OracleEKFRotations
    n, m = 60, 50
    s = SyntheticStream(n, m, seed=21, rvec_sigma=0.05)
    flt = _rot(max_landmarks=n, cov_dtype="float64")
    orc = OracleEKFRotations(INIT, mode="fast")
    worst = np.zeros(2)
    frames = list(s.bootstrap()) + list(s.steady(6))
    for ids, poses in frames:
        flt.observe(ids, poses)
        orc.observe(list(ids), poses)
        worst = np.maximum(worst, [rel_err(flt.state, orc.state), rel_err(flt.uncertainty, orc.uncertainty)])
    assert flt.backend.max_visible >= 50
    report("rotations_k350[float64]", state=worst[0], cov=worst[1])
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9, worst
    p = flt.uncertainty
    assert np.array_equal(p, p.T)
