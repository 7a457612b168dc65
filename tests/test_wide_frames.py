"""Wide frames: more detections per frame than the fused front kernel and the gather kernel take (EKF m > 64,
EKF_Rotations m > 50; up to 1024 with EKF_FLAG_WIDE_FRAMES, which HipEkf always sets).  Against the CPU oracle, frame by
frame, on an MI355X.

Tolerances: f64 as in test_hip_parity.py (STEP_TOL / ELEM_TOL); f32 covariance 2e-6 norm-wise up to k = 384 rows (the stage
solve / panel kernels), 1e-5 beyond (blocked factorisation, covariance update in row chunks of 384)."""
import numpy as np
import pytest

from conftest import rel_err, rel_err_elem, report

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
STEP_TOL = {"float64": 1e-10, "float32": 2e-6}
ELEM_TOL = {"float64": 1e-9}
F32_TOL_BLOCKED = 1e-5


def _filter(model, n, m, dtype, **kw):
    if model == "ekf":
        from aruco_slam_amd.filters.extended_kalman_filter import EKF
        return EKF(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, **kw)
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    return EKF_Rotations(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, **kw)


def _oracle(model, dtype):
    from oracle.ekf_numpy import OracleEKF, OracleEKFRotations
    store = np.float32 if dtype == "float32" else np.float64
    if model == "ekf":
        return OracleEKF(INIT, mode="fast", store_dtype=store)
    return OracleEKFRotations(INIT, mode="fast", store_dtype=store)


def _stream(model, n, m, seed):
    from aruco_slam_amd.synthetic import SyntheticStream
    return SyntheticStream(n, m, seed=seed, rvec_sigma=0.05 if model == "rot" else 0.0)


def _tol(model, m, dtype):
    k = (7 if model == "rot" else 3) * m
    if dtype == "float64":
        return STEP_TOL["float64"]
    return STEP_TOL["float32"] if -(-k // 16) * 16 <= 384 else F32_TOL_BLOCKED


def _check(name, flt, ref, dtype, tol, frame):
    st, p = flt.state, flt.uncertainty
    es, ep = rel_err(st, ref.state), rel_err(p, ref.uncertainty)
    out = {"frame": frame, "state": es, "P": ep}
    if dtype == "float64":
        out["state_elem"] = rel_err_elem(st, ref.state)
        out["P_elem"] = rel_err_elem(p, ref.uncertainty)
    assert es <= tol and ep <= tol, (name, out)
    if dtype == "float64":
        assert out["state_elem"] <= ELEM_TOL["float64"] and out["P_elem"] <= ELEM_TOL["float64"], (name, out)
    assert np.array_equal(p, p.T), name
    return out


def _run_parity(model, n, m, dtype, seed=5, steady=3):
    s = _stream(model, n, m, seed)
    flt, ref = _filter(model, n, m, dtype), _oracle(model, dtype)
    tol = _tol(model, m, dtype)
    worst = {}
    for t, (ids, poses) in enumerate(list(s.bootstrap()) + list(s.steady(steady))):
        flt.observe(ids, poses)
        ref.observe(list(ids), poses)
        out = _check(f"{model} n={n} m={m} {dtype}", flt, ref, dtype, tol, t)
        for key, val in out.items():
            if key != "frame":
                worst[key] = max(worst.get(key, 0.0), val)
    report(f"wide_parity_{model}_n{n}_m{m}_{dtype}", k=(7 if model == "rot" else 3) * m, tol=tol, **worst)
    return flt


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m", [(150, 65), (150, 128), (400, 129), (400, 300)])
def test_ekf_wide_frames_match_the_oracle(n, m, dtype):
    _run_parity("ekf", n, m, dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m", [(80, 51), (80, 55), (150, 120)])
def test_rotations_wide_frames_match_the_oracle(n, m, dtype):
    _run_parity("rot", n, m, dtype)


def test_every_marker_seen_twice_in_a_wide_frame():
    """Duplicates are legal (ekf_observe): m = 200 detections of 100 landmarks."""
    s = _stream("ekf", 100, 100, seed=9)
    flt, ref = _filter("ekf", 100, 200, "float64"), _oracle("ekf", "float64")
    frames = list(s.bootstrap())
    ids2 = np.concatenate([np.arange(100), np.arange(100)])
    frames += [s._observe(ids2) for _ in range(3)]
    for t, (ids, poses) in enumerate(frames):
        flt.observe(ids, poses)
        ref.observe(list(ids), poses)
        _check("duplicates", flt, ref, "float64", STEP_TOL["float64"], t)


def test_intermediates_of_a_blocked_wide_frame():
    """k = 900: L L^T = S = A H^T + R (built in NumPy from the fetched A and Jacobian), L W = A, identity padding of L."""
    n, m = 400, 300
    s = _stream("ekf", n, m, seed=2)
    flt = _filter("ekf", n, m, "float64")
    flt.backend.debug_enable_w()
    frames = list(s.bootstrap()) + list(s.steady(1))
    for ids, poses in frames:
        flt.observe(ids, poses)
    ids = frames[-1][0]
    b = flt.backend
    k, kp, dims = 3 * m, -(-3 * m // 16) * 16, flt.backend.dims
    jac, a = b.debug_fetch("jac", m), b.debug_fetch("A", m)
    lmat, w = b.debug_fetch("L", m), b.debug_fetch("W", m)
    resid = b.debug_fetch("resid", m)
    assert np.isfinite(resid).all() and resid.shape == (k,)
    h = np.zeros((k, dims))
    for j, marker in enumerate(ids):
        col = 10 + 3 * flt.landmarks[int(marker)]
        h[3 * j:3 * j + 3, :10] = jac[3 * j:3 * j + 3, :10]
        h[3 * j:3 * j + 3, col:col + 3] += jac[3 * j:3 * j + 3, 10:13]
    sm = a @ h.T + 0.9 * np.eye(k)
    lk = lmat[:k, :k]
    err_s = np.abs(lk @ lk.T - sm).max() / np.abs(sm).max()
    err_w = np.abs(lmat @ w - np.vstack([a, np.zeros((kp - k, dims))])).max() / np.abs(a).max()
    report("wide_intermediates_k900", LLt_vs_S=err_s, LW_vs_A=err_w)
    assert err_s <= 1e-12 and err_w <= 1e-12
    assert np.array_equal(np.triu(lmat, 1), np.zeros_like(lmat))
    assert np.array_equal(lmat[k:, :], np.eye(kp)[k:, :]) and np.array_equal(lmat[:, k:], np.eye(kp)[:, k:])
    assert np.array_equal(w[k:], np.zeros((kp - k, dims)))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_filter_that_grows_into_wide_frames_equals_one_built_large(dtype):
    outs = []
    for cap, vis in ((16, 8), (400, 300)):
        s = _stream("ekf", 400, 8, seed=21)
        rng = np.random.default_rng(3)
        flt = _filter("ekf", cap, vis, dtype)
        sizes = [(np.arange(8),), (np.arange(100),), (np.arange(100, 400),)]
        frames = [s._observe(ids[0]) for ids in sizes]
        frames += [s._observe(np.sort(rng.choice(400, mm, replace=False))) for mm in (300, 100, 8, 300)]
        traj = []
        for ids, poses in frames:
            flt.observe(ids, poses)
            traj.append(flt.state[:7].copy())
        assert flt.backend.max_visible >= 300
        outs.append((np.stack(traj), flt.state, flt.uncertainty))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_fused_and_wide_frames_alternate():
    """m = 60 (fused front kernel) and m = 70 (wide path) in turn, a state getter after every observe (process_frame)."""
    n = 150
    s = _stream("ekf", n, 70, seed=13)
    flt, ref = _filter("ekf", n, 70, "float64"), _oracle("ekf", "float64")
    rng = np.random.default_rng(6)
    frames = list(s.bootstrap())
    frames += [s._observe(np.sort(rng.choice(n, 60 if t % 2 == 0 else 70, replace=False))) for t in range(8)]
    frames += [s._observe(np.sort(rng.choice(n, 60, replace=False))) for _ in range(4)]
    for t, (ids, poses) in enumerate(frames):
        flt.observe(ids, poses)
        cam = flt.backend.get_state(10)
        ref.observe(list(ids), poses)
        assert rel_err(cam, ref.state[:10]) <= STEP_TOL["float64"]
        _check("alternate", flt, ref, "float64", STEP_TOL["float64"], t)


def test_sequence_of_wide_frames_is_serial_and_bitwise_the_per_frame_calls():
    import torch
    n, m = 150, 100
    out = []
    for mode in ("per_frame", "sequence"):
        s = _stream("ekf", n, m, seed=17)
        flt = _filter("ekf", n, m, "float32")
        for ids, poses in s.bootstrap():
            flt.observe(ids, poses)
        frames = list(s.steady(10))
        if mode == "per_frame":
            for ids, poses in frames:
                flt.observe(ids, poses)
        else:
            idx = torch.tensor(np.stack([f[0] for f in frames]), dtype=torch.int32, device="cuda:0")
            z = torch.tensor(np.stack([f[1][:, :3] for f in frames]), dtype=torch.float64, device="cuda:0")
            flt.backend.observe_sequence(idx, z)
            assert flt.backend.last_sequence_mode() == "serial"
        out.append((flt.state, flt.uncertainty))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("dtype,kernels", [("float64", ("valu", "mfma")),
                                           ("float32", ("valu", "mfma", "mfma_tile", "mfma_macro"))])
def test_covariance_kernels_agree_on_blocked_wide_frames(dtype, kernels):
    n, m = 400, 300
    outs = []
    for kern in kernels:
        s = _stream("ekf", n, m, seed=4)
        flt = _filter("ekf", n, m, dtype, cov_kernel=kern)
        for ids, poses in list(s.bootstrap()) + list(s.steady(3)):
            flt.observe(ids, poses)
        p = flt.uncertainty
        assert np.array_equal(p, p.T), kern
        cov_t, dims = flt.backend.cov_t, flt.backend.dims
        assert float(cov_t[dims:, :].abs().max()) == 0.0 and float(cov_t[:, dims:].abs().max()) == 0.0, kern
        outs.append((kern, flt.state, p))
    for kern, st, p in outs[1:]:
        assert np.array_equal(st, outs[0][1]), kern
        assert np.array_equal(p, outs[0][2]), kern


def test_bad_device_index_in_a_wide_frame_is_sticky_until_reset(tmp_path):
    import torch
    from aruco_slam_amd.hip_backend import EkfError
    n, m = 100, 70
    s = _stream("ekf", n, m, seed=8)
    frames = list(s.bootstrap()) + list(s.steady(4))
    good, bad = _filter("ekf", n, m, "float64"), _filter("ekf", n, m, "float64")
    for ids, poses in frames[:3]:
        good.observe(ids, poses)
        bad.observe(ids, poses)
    ck = tmp_path / "ck.npz"
    bad.save_checkpoint(str(ck))
    idx = torch.arange(m, dtype=torch.int32, device="cuda").reshape(1, m)
    idx[0, 5] = 9999
    z = torch.ones((1, m, 3), dtype=torch.float64, device="cuda")
    bad.backend.observe_sequence(idx, z)
    with pytest.raises(EkfError) as err:
        bad.backend.sync()
    assert err.value.code == -1
    with pytest.raises(EkfError):
        bad.backend.get_state()
    bad.reset()
    bad.load_checkpoint(str(ck))
    for ids, poses in frames[3:]:
        good.observe(ids, poses)
        bad.observe(ids, poses)
    assert np.array_equal(good.state, bad.state)
    assert np.array_equal(good.uncertainty, bad.uncertainty)
