"""us per frame of a per-frame observe + get_poses loop at C3 (n = 1024, m = 32, f32), one JSON line:

    python tools/filter_gate_loop.py none|inf|1e300 [frames] [rows]

none: a filter without the gate; inf: built with the gate, off, distances reported every frame (EKF.observe goes through
ekf_observe_gated); 1e300: a gate that rejects nothing.  The gate kernel's own time: the same command under
``rocprofv3 --kernel-trace --stats --output-format csv``, in a run of its own.  rows: the filter is built with
row_noise=True and every frame carries per-detection noise (log-uniform in [0.3, 3]); under rocprofv3 this gives the front
kernel's time with the rows."""
import json, sys, time
from pathlib import Path
import numpy as np
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from aruco_slam_amd.filters.extended_kalman_filter import EKF
from aruco_slam_amd.synthetic import SyntheticStream

mode = sys.argv[1]
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
rows = len(sys.argv) > 3 and sys.argv[3] == "rows"
kw = {} if mode == "none" else {"gate": float(mode)}
if rows:
    kw["row_noise"] = True
noise = np.exp(np.random.default_rng(1).uniform(np.log(0.3), np.log(3.0), (32, 3)))
step = (lambda ids, poses: flt.observe(ids, poses, noise=noise)) if rows else (lambda ids, poses: flt.observe(ids, poses))
init = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
flt = EKF(init, max_landmarks=1024, max_visible=32, cov_dtype="float32", **kw)
stream = SyntheticStream(1024, 32, seed=0)
for ids, poses in stream.bootstrap():
    flt.observe(ids, poses)
steady = list(stream.steady(frames + 300))
for ids, poses in steady[:300]:
    step(ids, poses)
    flt.get_poses()
flt.backend.sync()
t = time.perf_counter()
for ids, poses in steady[300:]:
    step(ids, poses)
    flt.get_poses()
flt.backend.sync()
dt = time.perf_counter() - t
print(json.dumps({"loop": "observe+get_poses", "mode": mode, "row_noise": bool(rows), "n": 1024, "m": 32, "dtype": "float32", "frames": frames,
                  "us_per_frame": 1e6 * dt / frames}), flush=True)
