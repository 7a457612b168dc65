#!/usr/bin/env python3
"""Which chain sets the period of the pipelined sequence mode?  One warm-up call, then ONE pipelined call of `frames` frames
with role-level stamps; per frame (in-kernel 100 MHz clock, no profiler): the start of the front kernel, and when its
measurement workgroup entered and left the end gate that waits for "covariance update of the previous frame complete".
    gate_spin.py [n=1024] [m=32] [frames=2000] [dtype=float32] [out.json]
A spin of (about) zero polls: the update was over before the front kernel asked -- the front-kernel chain binds.  A spin
is covariance-chain time only where the gate is also the LAST thing of its launch: `leave_to_next_start` is then one kernel
boundary; where it is longer, other workgroups of the front kernel were still running when the gate opened."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def dist(us):
    us = np.asarray(us, dtype=np.float64)
    q = np.percentile(us, [0, 5, 25, 50, 75, 95, 99, 100])
    return {"mean": round(float(us.mean()), 3),
            **{k: round(float(v), 3) for k, v in zip(("min", "p5", "p25", "p50", "p75", "p95", "p99", "max"), q)}}


def main():
    import torch
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    from aruco_slam_amd.synthetic import SyntheticStream
    a = sys.argv[1:]
    n = int(a[0]) if len(a) > 0 else 1024
    m = int(a[1]) if len(a) > 1 else 32
    frames = int(a[2]) if len(a) > 2 else 2000
    dtype = a[3] if len(a) > 3 else "float32"
    out = a[4] if len(a) > 4 else None
    from aruco_slam_amd.hip_backend import GATE_LOG_FRAMES as ring
    assert 16 <= frames <= ring, "the ring holds %d frames" % ring
    warm = 50
    init = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
    s = SyntheticStream(n, m, seed=0)
    flt = EKF(init, max_landmarks=n, max_visible=m, cov_dtype=dtype, lookahead=True)
    flt.backend.debug_enable_stamps(True)
    boot = 0
    for ids, poses in s.bootstrap():
        flt.observe(ids, poses)
        boot += 1
    fr = list(s.steady(warm + frames))
    idx = torch.tensor(np.stack([f[0] for f in fr]), dtype=torch.int32, device="cuda:0")
    z = torch.tensor(np.stack([f[1][:, :3] for f in fr]), dtype=torch.float64, device="cuda:0")
    hip = flt.backend
    hip.observe_sequence(idx[:warm], z[:warm])
    hip.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hip.observe_sequence(idx[warm:], z[warm:])
    hip.sync()
    wall = (time.perf_counter() - t0) * 1e6
    mode = hip.last_sequence_mode()
    log = hip.debug_fetch("gate_log", m)
    first = boot + warm + 1                              # fused-frame number of the call's first frame
    rows = log[[(first + t) & (ring - 1) for t in range(frames)]] / 100.0      # us
    start, enter, leave, polls = rows[:, 0], rows[:, 1], rows[:, 2], log[[(first + t) & (ring - 1) for t in range(frames)], 3]
    g = slice(1, frames)                                 # (frame 0 of a run has no gate)
    res = {
        "shape": {"n": n, "m": m, "cov_dtype": dtype, "frames": frames}, "sequence_mode": mode,
        "wall_us_per_frame": round(wall / frames, 3),
        "starts_in_order": bool(np.all(np.diff(start) > 0)),
        "front_start_to_start_us": dist(np.diff(start)),
        "gate_spin_us": dist((leave - enter)[g]),
        "gate_polls": dist(polls[g]),
        "frames_with_zero_polls": int((polls[g] == 0).sum()),
        "start_to_gate_enter_us": dist((enter - start)[g]),
        "start_to_gate_leave_us": dist((leave - start)[g]),
        "leave_to_next_start_us": dist(start[2:] - leave[1:-1]),
    }
    print(json.dumps(res), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
