"""One predict + update step in extended precision  --  TEST INFRASTRUCTURE ONLY.

A sharper yardstick than ``ekf_numpy`` for single steps: the measurement z, the prediction h(x) and the Jacobian blocks
come from the f64 oracle (``OracleEKF`` / ``OracleEKFRotations``, ``measurement_blocks``) and are taken as exact inputs;
everything after them runs in ``np.longdouble`` (x87 80-bit, 64-bit significand on x86-64):

    P+Q,   A = H (P+Q),   S = A H^T + r I,   L L^T = S,   W = L^-1 A,   y = L^-1 (z - h),   delta = W^T y,
    P' = (P+Q) - W^T W

and delta is injected by the oracle's own ``_inject`` in f64.  The rounding error of this reference is ~2^-64 times the
magnitudes below, three orders under the f64 bound the GPU tests apply, so the reference counts as exact there.

Besides the step it returns the magnitudes of the componentwise error bounds (``tests/update_sweep_util.py``):
``M_P = |P+Q| + |W|^T |W|`` and ``M_x = |x| + |W|^T |y|``.
"""
from __future__ import annotations

import numpy as np

from oracle.ekf_numpy import R_UNCERTAINTY

LD = np.longdouble
if np.finfo(LD).nmant < 63:      # (no silent fall-back to a double-precision "reference")
    raise ImportError(f"oracle.ekf_extended needs an extended long double (64-bit significand); this platform has "
                      f"{np.finfo(LD).nmant + 1} bits")


def _split(a_ld):
    """longdouble array -> (hi, lo) f64 pair with hi + lo = a to ~2^-106 (pickles, and subtracts exactly)."""
    hi = a_ld.astype(np.float64)
    return hi, (a_ld - hi.astype(LD)).astype(np.float64)


def cholesky_ld(s):
    """Lower Cholesky factor, plain column loop in longdouble."""
    k = s.shape[0]
    lf = np.zeros_like(s)
    for j in range(k):
        d = s[j, j] - lf[j, :j] @ lf[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"S is not positive definite (pivot {j})")
        lf[j, j] = np.sqrt(d)
        lf[j + 1:, j] = (s[j + 1:, j] - lf[j + 1:, :j] @ lf[j, :j]) / lf[j, j]
    return lf


def forward_ld(lf, b):
    """L^-1 b (b: [k] or [k, N]), row loop in longdouble."""
    x = np.empty_like(b)
    for i in range(lf.shape[0]):
        x[i] = (b[i] - lf[i, :i] @ x[:i]) / lf[i, i]
    return x


def extended_step(orc, ids, poses, factors=False):
    """One step of ``orc`` (an ``OracleEKF`` or ``OracleEKFRotations`` holding the prior; not modified) on the frame
    ``ids`` / ``poses``.  Returns a dict:

    ``P1`` / ``P1_lo``: P' as an f64 (hi, lo) pair; ``x1``: posterior state (f64, the oracle's injection);
    ``M_P``, ``M_x``: bound magnitudes (f64); ``delta`` (f64); ``k``; ``kappa``: 2-norm condition number of S;
    with ``factors``: ``S``, ``A``, ``L``, ``W`` (f64 roundings) for checks of the kernel's intermediates."""
    z, hv, jac, col = orc.measurement_blocks(ids, poses)
    rd, lmd = jac.shape[1], jac.shape[2] - 10
    k = rd * len(ids)
    p = np.asarray(orc.uncertainty, dtype=np.float64)
    qd = orc.process_noise_diag()
    n_dims = p.shape[0]
    pq = p.astype(LD)
    pq[np.arange(n_dims), np.arange(n_dims)] += qd.astype(LD)
    jl = jac.astype(LD)
    # A = H (P+Q) and S = A H^T from the nonzero blocks of H: camera columns 0:10 and the landmark's lmd columns
    a = np.empty((k, n_dims), dtype=LD)
    for j, c0 in enumerate(col):
        r = slice(rd * j, rd * j + rd)
        a[r] = jl[j][:, :10] @ pq[:10] + jl[j][:, 10:] @ pq[c0:c0 + lmd]
    s = np.empty((k, k), dtype=LD)
    for j, c0 in enumerate(col):
        r = slice(rd * j, rd * j + rd)
        s[:, r] = a[:, :10] @ jl[j][:, :10].T + a[:, c0:c0 + lmd] @ jl[j][:, 10:].T
    s = 0.5 * (s + s.T)
    s[np.arange(k), np.arange(k)] += LD(R_UNCERTAINTY)      # (r of both models)
    lf = cholesky_ld(s)
    w = forward_ld(lf, a)
    y = forward_ld(lf, (z.astype(LD) - hv.astype(LD)))
    delta = w.T @ y
    p1 = pq - w.T @ w
    p1 = 0.5 * (p1 + p1.T)          # (exactly symmetric: the two halves differ by the order of longdouble sums only)
    wa = np.abs(w).astype(np.float64)
    mp = np.abs(pq).astype(np.float64) + wa.T @ wa
    md = wa.T @ np.abs(y).astype(np.float64)
    x0 = np.asarray(orc.state, dtype=np.float64)
    saved = orc.state
    try:
        orc.state = x0.copy()
        orc._inject(delta.astype(np.float64))
        x1 = np.asarray(orc.state, dtype=np.float64).copy()
    finally:
        orc.state = saved
    mx = np.abs(x0) + md
    # quaternions move with the error state of their pose (delta[3:7] itself is dropped): q' depends on delta[e]
    quats = [(3, 7)] + ([(10 + 10 * i + 3, 10 + 10 * i + 7) for i in range((n_dims - 10) // 10)] if lmd == 10 else [])
    for q0, _ in quats:
        mx[q0:q0 + 4] = np.abs(x0[q0:q0 + 4]) + md[q0 + 4:q0 + 7].max()
    ev = np.linalg.eigvalsh(s.astype(np.float64))
    hi, lo = _split(p1)
    out = {"P1": hi, "P1_lo": lo, "x1": x1, "M_P": mp, "M_x": mx, "delta": delta.astype(np.float64), "k": k,
           "kappa": float(ev[-1] / ev[0])}
    if factors:
        out.update(S=s.astype(np.float64), A=a.astype(np.float64), L=lf.astype(np.float64), W=w.astype(np.float64))
    return out
