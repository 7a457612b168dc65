"""Helpers of the update-kernel sweep (``test_update_sweep.py`` on the GPU, ``test_update_sweep_cpu.py`` here): dense priors,
the extended-precision reference of one step, the componentwise checker, the case table and a restatement of the
kernel dispatch that maps a case to the template instances it runs.

Componentwise bound.  For one step from the prior (x, P) with k measurement rows, the reference
(``oracle/ekf_extended.py``) gives P' and x' to ~2^-64 and the magnitudes

    M_P = |P+Q| + |W|^T |W|,        M_x = |x| + |W|^T |y|      (quaternion entries: |q| + max M_x of their error state).

The checker requires   max |P'_gpu - P'_ref| / M_P <= c_P (k+1) u   and   max |x'_gpu - x'_ref| / M_x <= c_x tau_x.
u = 2^-53 for an f64 covariance, 2^-24 for f32.  Why (k+1) u M_P: P' = (P+Q) - sum_r w_r^T w_r is a sum of k+1 terms,
and a recursive sum of k+1 terms with rounding u carries at most about (k+1) u times the sum of their magnitudes, which is
M_P; the errors W carries from the factorisation and the triangular solve enter through |W|^T|W| with the same form
(and with kappa(S) <= 1e3, which the sweep asserts, their condition factor stays O(1), absorbed by c).
The state: delta = W^T y is a sum of k products, and x' = x + delta (the quaternions through their error state), so an
f64 computation gives (k+1) u64 M_x.  With an f32 covariance the state is still computed in f64, from W and y that come
from the f32-stored prior; if delta is formed from W after its rounding to f32 storage, that adds |W - fl32(W)|^T |y| <=
u32 |W|^T |y| <= u32 M_x.  So tau_x = (k+1) u64 for f64 and (k+1) u64 + u32 for f32.

The constants c are measured (the worst ratio per path on an MI355X, profiles/update_sweep/) with at most 8x head-room.
"""
from __future__ import annotations

import os
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

import support as sp

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "aruco_slam_amd" / "csrc"
INIT = sp.INIT
U = {"float64": 2.0 ** -53, "float32": 2.0 ** -24}
KAPPA_MAX = 1e3
# (c_P, c_x) per path and covariance dtype: the worst ratio measured on an MI355X (profiles/update_sweep/summary.json) times
# 4, rounded up to two digits.  (The f32 c_x are tiny: the state of an f32 filter is computed from the f64 W and is as
# accurate as in an f64 filter, far inside tau_x's u32 term.)
C_BOUNDS = {
    "ekf_fused": {"float64": (12, 4.9), "float32": (2.4, 2.4e-7)},
    "ekf_stage": {"float64": (12, 4.9), "float32": (2.4, 7.6e-8)},
    "ekf_wide": {"float64": (1.1, 0.22), "float32": (0.24, 1.1e-7)},
    "ekf_blocked": {"float64": (0.6, 0.12), "float32": (0.18, 1.5e-7)},
    "rot_fused": {"float64": (3.0, 2.7), "float32": (1.3, 4.3e-7)},
    "rot_stage": {"float64": (0.57, 0.18), "float32": (0.28, 6.8e-8)},
    "rot_wide": {"float64": (0.43, 0.093), "float32": (0.21, 8.0e-8)},
    "rot_blocked": {"float64": (0.32, 0.12), "float32": (0.17, 4.2e-8)},
    "scalar_first": {"float64": (0.94, 0.4), "float32": (0.31, 4.5e-8)},
    "f32_valu": {"float32": (0.69, 1.1e-7)},
    "f32_mfma_tile": {"float32": (0.69, 1.1e-7)},
    "f32_mfma_macro": {"float32": (0.69, 1.1e-7)},
    "f64_valu": {"float64": (2.5, 1.5)},
    "f64_mfma": {"float64": (2.5, 1.5)},
    "tails": {"float64": (4.6, 1.2), "float32": (1.9, 6.8e-8)},
    "batch": {"float64": (7.0, 2.8)},
    "intermediates": {"float64": (36, 390), "float32": (740, 1.3e4)},      # (c of L L^T = S, c of L W = A)
}


# --------------------------------------------------------------------------------------------------------------------
# dense priors
# --------------------------------------------------------------------------------------------------------------------
def _unit_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def dense_prior(model, n, m, seed, dtype="float64"):
    """(state, P, marker ids, frame ids, frame poses) of a random prior with a DENSE covariance.

    P = D C D: C is a correlation matrix from a random rank-4 factor plus a diagonal, so every entry is O(0.1-1) and
    distinct; the scales D lie in [0.05, 2] (camera pose and error state at the low end, which keeps kappa(S) small).
    P is exactly symmetric, and for an f32 filter rounded to f32 (the value both sides start from).  The camera has a
    random unit quaternion, the landmarks lie 1-2 m from it, z = h(x) + N(0, 0.05^2); for EKF_Rotations the landmark
    orientations are moderate Euler angles (|a| <= 0.6) seen from the camera, and the measured angles scatter by 0.02
    around them (far from the quaternion sign tie).  m > n repeats landmarks within the frame."""
    from oracle.ekf_numpy import h_closed, h_rot_closed, _qmul, quat_from_euler_xyz
    rng = np.random.default_rng(seed)
    lmd = 10 if model == "rot" else 3
    dims = lmd * n + 10
    cam = np.zeros(10)
    cam[0:3] = rng.uniform(-1.0, 1.0, 3)
    cam[3:7] = _unit_quat(rng)
    state = [cam]
    angles = rng.uniform(-0.6, 0.6, (n, 3))
    for i in range(n):
        d = rng.normal(size=3)
        xyz = cam[0:3] + d / np.linalg.norm(d) * rng.uniform(1.0, 2.0)
        if lmd == 3:
            state.append(xyz)
        else:
            q = _qmul(cam[3:7], quat_from_euler_xyz(angles[i] + rng.normal(0.0, 0.02, 3)))
            state.append(np.concatenate((xyz, q / np.linalg.norm(q), np.zeros(3))))
    state = np.concatenate(state)
    f = rng.normal(size=(dims, 4))
    c = 0.3 * (f @ f.T) + np.diag(rng.uniform(0.5, 1.5, dims))
    s = 1.0 / np.sqrt(np.diag(c))
    d = rng.uniform(0.05, 1.5, dims)
    d[0:10] = rng.uniform(0.05, 0.07, 10)
    p = (d * s)[:, None] * c * (d * s)[None, :]
    p = np.tril(p) + np.tril(p, -1).T
    if dtype == "float32":
        p = p.astype(np.float32).astype(np.float64)
    ids = rng.choice(n, m, replace=False) if m <= n else np.concatenate((rng.permutation(n), rng.integers(0, n, m - n)))
    poses = np.zeros((m, 6))
    for j, i in enumerate(ids):
        c0 = 10 + lmd * i
        x13 = np.concatenate((cam, state[c0:c0 + 3]))
        poses[j, 0:3] = h_closed(x13) + rng.normal(0.0, 0.05, 3)
        if lmd == 10:
            poses[j, 3:6] = angles[i] + rng.normal(0.0, 0.02, 3)
            assert h_rot_closed(np.concatenate((cam, state[c0:c0 + 10])))[3:7] @ quat_from_euler_xyz(poses[j, 3:6]) > 0.9
    return state, p, list(range(n)), [int(i) for i in ids], poses


def oracle_at(model, state, p, lm_ids, quat="as_written"):
    from oracle.ekf_numpy import OracleEKF, OracleEKFRotations
    orc = OracleEKFRotations(INIT, mode="fast") if model == "rot" else OracleEKF(INIT, mode="fast", quat_mode=quat)
    orc.state = np.array(state, dtype=np.float64)
    orc.uncertainty = np.array(p, dtype=np.float64)
    orc.landmarks = {int(k): i for i, k in enumerate(lm_ids)}
    orc.num_landmarks = len(lm_ids)
    return orc


RefKey = namedtuple("RefKey", "model n m dtype quat")


def prior_seed(key):
    return 1000003 * key.n + 7919 * key.m + (17 if key.model == "rot" else 0) + (5 if key.dtype == "float32" else 0)


def reference(key, factors=False):
    """(prior, extended-precision step) of a RefKey: one per (prior, m), shared by every kernel and path."""
    from oracle.ekf_extended import extended_step
    prior = dense_prior(key.model, key.n, key.m, prior_seed(key), key.dtype)
    state, p, lm_ids, ids, poses = prior
    ref = extended_step(oracle_at(key.model, state, p, lm_ids, key.quat), ids, poses, factors=factors)
    return prior, ref


def references(keys, factors=False):
    """reference() of many keys on a thread pool (the longdouble products release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    keys = list(dict.fromkeys(keys))
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    workers = max(1, min(16, cpus, int(os.environ.get("OMP_NUM_THREADS", cpus))))
    with ThreadPoolExecutor(workers) as pool:
        return dict(zip(keys, pool.map(lambda k: reference(k, factors), keys)))


# --------------------------------------------------------------------------------------------------------------------
# the checker
# --------------------------------------------------------------------------------------------------------------------
def ratios(ref, p_gpu, x_gpu, dtype):
    """(r_P, r_x): the worst componentwise error in units of (k+1) u M_P and tau_x M_x -- the smallest c that passes."""
    k = ref["k"]
    p_gpu = np.asarray(p_gpu, dtype=np.float64)
    tiny = np.finfo(np.float64).tiny       # (M = 0 where P and W vanish: any error there fails)
    ep = np.abs((p_gpu - ref["P1"]) - ref["P1_lo"]) / np.maximum(ref["M_P"], tiny)
    ex = np.abs(np.asarray(x_gpu, dtype=np.float64) - ref["x1"]) / np.maximum(ref["M_x"], tiny)
    tau_x = (k + 1) * U["float64"] + (U["float32"] if dtype == "float32" else 0.0)
    return float(ep.max() / ((k + 1) * U[dtype])), float(ex.max() / tau_x)


def check_step(ref, p_gpu, x_gpu, dtype, c_p, c_x, what=""):
    """Assert the componentwise bounds (and P' bitwise symmetric); return (r_P, r_x)."""
    assert np.array_equal(p_gpu, p_gpu.T), f"{what}: P' is not bitwise symmetric"
    r_p, r_x = ratios(ref, p_gpu, x_gpu, dtype)
    assert r_p <= c_p, f"{what}: P' error {r_p:.3g} (k+1) u M_P > c_P = {c_p}"
    assert r_x <= c_x, f"{what}: state error {r_x:.3g} tau_x M_x > c_x = {c_x}"
    return r_p, r_x


def backward_ratios(ref, lfac, wmat, dtype):
    """Intermediates of the kernel (debug_fetch L [kp, kp], W [kp, N], f64): componentwise backward errors
    |L L^T - S| / (|L| |L|^T) and |L W - A| / (|L| |W|) (the classical bounds of a Cholesky factorisation and of a triangular
    solve, gamma_{k+1} with u of the f64 factorisation), in units of (k+1) u64, computed in longdouble."""
    ld = np.longdouble
    k = ref["k"]
    lk = lfac[:k, :k].astype(ld)
    wk = wmat[:k].astype(ld)
    la = np.abs(lk)
    es = np.abs(lk @ lk.T - ref["S"].astype(ld)) / np.maximum(la @ la.T, np.finfo(np.float64).tiny)
    ew = np.abs(lk @ wk - ref["A"].astype(ld)) / np.maximum(la @ np.abs(wk), np.finfo(np.float64).tiny)
    unit = (k + 1) * U["float64"]
    return float(es.max() / unit), float(ew.max() / unit)


# --------------------------------------------------------------------------------------------------------------------
# the case table
# --------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "group model dtype n m kernel fused quat max_visible")
DTYPES = ("float64", "float32")
# smallest and largest m of every NB = ceil(3 m / 16) of the EKF update (m <= 64)
EKF_NB_BOUNDS = (1, 5, 6, 10, 11, 16, 17, 21, 22, 26, 27, 32, 33, 37, 38, 42, 43, 48, 49, 53, 54, 58, 59, 64)
EKF_NB_LARGEST = EKF_NB_BOUNDS[1::2]
EKF_WIDE_M = (69, 74, 80, 85, 90, 96, 101, 106, 112, 117, 122, 128)      # largest m of NB 13 .. 24
ROT_NB_ONE = (2, 4, 6, 9, 11, 13, 16, 18, 20, 22, 25, 27)                # one m per NB 1 .. 12 of EKF_Rotations
TAILS = ((1, 1), (18, 7), (39, 13), (61, 20), (82, 27), (125, 40))        # N = 13, 64, 127, 193, 256, 385
ALL_KERNELS = (("float64", "valu"), ("float64", "mfma"), ("float32", "valu"), ("float32", "mfma_tile"),
               ("float32", "mfma_macro"))


def _c(group, model, dtype, n, m, kernel="auto", fused=True, quat="as_written", max_visible=None):
    if max_visible is None:
        max_visible = {"ekf": 64, "rot": 55}[model] if n in (125, 63) else max(m, 64 if model == "ekf" else 50)
    return Case(group, model, dtype, n, m, kernel, fused, quat, max_visible)


def sweep_cases():
    out = []
    for dt in DTYPES:
        out += [_c("ekf_fused", "ekf", dt, 125, m) for m in range(1, 65)]
        out += [_c("ekf_stage", "ekf", dt, 125, m, fused=False) for m in EKF_NB_BOUNDS]
        out += [_c("ekf_wide", "ekf", dt, 167, m, max_visible=128) for m in EKF_WIDE_M]
        out += [_c("ekf_blocked", "ekf", dt, 210, m, max_visible=200) for m in (129, 200)]
        for m in range(1, 56):
            grp = "rot_fused" if m <= 27 else "rot_stage" if m <= 50 else "rot_wide" if m <= 54 else "rot_blocked"
            out.append(_c(grp, "rot", dt, 63, m))
        out += [_c("scalar_first", "ekf", dt, 125, m, quat="scalar_first") for m in (16, 40, 64)]
    for kern in ("valu", "mfma_tile", "mfma_macro"):        # f32 covariance kernels, every KB = 1 .. 24 once
        out += [_c(f"f32_{kern}", "ekf", "float32", 125, m, kern) for m in EKF_NB_LARGEST]
        out += [_c(f"f32_{kern}", "ekf", "float32", 167, m, kern, max_visible=128) for m in EKF_WIDE_M]
    for kern in ("valu", "mfma"):                           # f64 kernels across the split / full threshold
        out += [_c(f"f64_{kern}", "ekf", "float64", n, m, kern, max_visible=128) for n in (668, 669) for m in (5, 32, 64, 128)]
    for n, m in TAILS:
        out += [_c("tails", "ekf", dt, n, m, kern, max_visible=64) for dt, kern in ALL_KERNELS]
    return out


def ref_key(case):
    return RefKey(case.model, case.n, case.m, case.dtype, case.quat)


def filter_key(case):
    return (case.model, case.dtype, case.n, case.kernel, case.fused, case.quat, case.max_visible)


# --------------------------------------------------------------------------------------------------------------------
# restatement of the dispatch: which template instances a frame runs
# --------------------------------------------------------------------------------------------------------------------
def compiled_instances():
    """Every instance the launchers can select, parsed from the sources: front kernel FR_GO(NU, MODEL, NB) and its default
    branches (both covariance types), SV_CASE(NB) (solve, no type), PN_CASE(NB) (panel, both types), EKF_COV_CASE(KB)
    (f32 wave-per-tile), CM_CASE(KB) (f32 macro-tile), the f64 split / full pair and the VALU kernel of both types."""
    front = (CSRC / "ekf_front_impl.h").read_text()
    launch = front[front.index("void ekf_launch_front("):]
    fr = {tuple(map(int, t)) for t in re.findall(r"FR_GO\((\d+), (\d+), (\d+)\)", launch)}
    fr |= {tuple(map(int, t)) for t in re.findall(r"ekf_front_go<T, (\d+), (\d+), (\d+)>\(fr, s\)", launch)}
    small = (CSRC / "ekf_small_kernels.hip").read_text()
    sv = {int(x) for x in re.findall(r"SV_CASE\((\d+)\)", small)}
    pn = {int(x) for x in re.findall(r"PN_CASE\((\d+)\)", small)}
    cov = (CSRC / "ekf_cov_update.hip").read_text()
    tile = {int(x) for x in re.findall(r"EKF_COV_CASE\((\d+)\)", cov)}
    macro = {int(x) for x in re.findall(r"CM_CASE\((\d+)\)", (CSRC / "ekf_cov_macro.hip").read_text())}
    out = set()
    for dt in DTYPES:
        out |= {("front", dt) + t for t in fr} | {("panel", dt, nb) for nb in pn} | {("cov_valu", dt)}
    out |= {("solve", nb) for nb in sv}
    out |= {("cov_tile", kb) for kb in tile} | {("cov_macro", kb) for kb in macro}
    out |= {("cov_f64_split",), ("cov_f64_full",)}
    return out


def f64_split_items():
    """The `items <= ...` threshold of the f64 covariance launcher (ekf_cov_update.hip)."""
    return int(re.search(r"if \(items <= (\d+)\)", (CSRC / "ekf_cov_update.hip").read_text()).group(1))


def macro_min_tiles():
    return int(re.search(r"kMacroMinTiles = (\d+);", (CSRC / "ekf_filter.h").read_text()).group(1))


def instances_of(case):
    """The instances one frame of `case` runs -- a Python restatement of the dispatch:
      ekf_frames.hip enqueue_frame (:162-260): fused front kernel if use_front_kernel (:108: not flags bit 2, kpad <= 192);
        else a wide frame (m > 64 / 50, visible_cap, ekf_filter.h:19-20) -- blocked beyond kpad 384 (EKF_WIDE_REUSE_ROWS), else the
        stage solve / panel; else gather + stage solve / panel.  The covariance update runs once, or per 384-row chunk.
      ekf_front_impl.h ekf_launch_front (:1419-1440): NU / MODEL / NB by model and m.
      ekf_small_kernels.hip ekf_launch_solve / ekf_launch_panel (:212-219, :302-311): NB = kpad / 16.
      ekf_cov_update.hip ekf_launch_cov_update (:396-430): VALU when forced; f32: macro-tile when the launch table exists
        (ensure_tiles, ekf_frames.hip:137-142: forced, or kMacroMinTiles lower-triangle tiles), else wave-per-tile KB;
        f64: split up to `items` 32 x 32 tiles, full above."""
    rd = 7 if case.model == "rot" else 3
    lmd = 10 if case.model == "rot" else 3
    k = rd * case.m
    kpad = -(-k // 16) * 16
    nb = kpad // 16
    dims = lmd * case.n + 10
    wide = case.m > (50 if case.model == "rot" else 64)
    out = set()
    if case.fused and kpad <= 192:
        if case.model == "rot":
            out.add(("front", case.dtype, 4, 1, min(nb, 12)))
        elif case.m <= 32:
            out.add(("front", case.dtype, 4, 0, min(nb, 6)))
        else:
            out.add(("front", case.dtype, 8, 0, min(max(nb, 7), 12)))
    elif not (wide and kpad > 384):
        out |= {("solve", nb), ("panel", case.dtype, nb)}
    chunks = [min(384, kpad - r0) // 16 for r0 in range(0, kpad, 384)]
    t128 = -(-dims // 128)
    for kb in chunks:
        if case.kernel == "valu":
            out.add(("cov_valu", case.dtype))
        elif case.dtype == "float32":
            macro = case.kernel != "mfma_tile" and (case.kernel == "mfma_macro" or t128 * (t128 + 1) // 2 >= macro_min_tiles())
            out.add(("cov_macro", kb) if macro else ("cov_tile", kb))
        else:
            t = -(-dims // 32)
            out.add(("cov_f64_split",) if t * (t + 1) // 2 <= f64_split_items() else ("cov_f64_full",))
    return out
