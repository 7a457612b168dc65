"""Cost of ekf_remove_markers against a device-to-device copy of the covariance, and the host route it replaces.

For every shape (--landmarks n, f32 covariance, max_visible 32) and every removal count (--counts): a filter whose n
landmarks were first-sighted by a synthetic.ragged_log; then, alternating in one process and on the filter's stream,
  * ekf_remove_markers of `count` scattered landmarks into a second pair of buffers (HIP events around the C call: the
    index-map upload and the one launch: gather, fringe of the second covariance buffer, mirror of the state), after
    which `count` markers are added again, outside the timed region, so that every repetition sees n landmarks;
  * hipMemcpyAsync device-to-device of cov_bytes (events around it): the yardstick.  The kernel reads N'^2 and writes cap^2
    elements, so it moves no more bytes than the copy.
--reps repetitions after --warmup warm-ups; median and p90 in microseconds.  Once per shape (with the last removal count),
the host route: get_cov -> np.delete -> set_state_cov into a second filter, wall time (--no-host-route skips it).  One JSON line per point, printed and
appended to profiles/remove/remove_bench.jsonl (--out).  Kernel time alone: `rocprofv3 --kernel-trace --stats -- python
tools/remove_bench.py --no-host-route --reps 20` in a run of its own.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float64)


def hip_runtime():
    """The HIP runtime the process has already loaded (torch's; the in-tree library is linked against it), for
    hipMemcpyAsync: the symbol is resolved through the library that uses it."""
    from aruco_slam_amd import hip_backend
    return C.CDLL(str(hip_backend.LIB_PATH))


def stats(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return {"median_us": float(np.median(v)), "p90_us": float(v[int(np.ceil(0.9 * len(v))) - 1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--landmarks", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--counts", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=str(REPO / "profiles" / "remove" / "remove_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from aruco_slam_amd import _build
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    from aruco_slam_amd.synthetic import ragged_log
    _build.build()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    hip = None
    for n in args.landmarks:
        log = ragged_log(n, (32, 32), 2, seed=0)
        flt = EKF(INIT, max_landmarks=n, max_visible=32, cov_dtype="float32", quat_update="scalar_first")
        flt.process_detection_log(log["ids"], log["poses"], log["offsets"])
        be, lib = flt.backend, flt.backend.lib
        hip = hip or hip_runtime()
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        hip.hipMemcpyAsync.restype = C.c_int
        cov_bytes = be.cov_t.numel() * be.cov_t.element_size()
        nbytes = C.c_size_t()
        be._check(lib.ekf_remove_workspace_bytes(be.h, max(args.counts), C.byref(nbytes)))
        with torch.cuda.device(be.device), torch.cuda.stream(be.stream):
            pairs = [(be.cov_t, be.state_t), (torch.empty_like(be.cov_t), torch.empty_like(be.state_t))]
            ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=be.device)
            scratch = torch.empty_like(be.cov_t)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            cur = 0
            for count in args.counts:
                idx = np.ascontiguousarray(np.linspace(1, n - 2, count).astype(np.int32))
                assert len(set(idx.tolist())) == count
                fresh = np.tile(np.array([0.5, 0.5, 8.0]), (count, 1))
                t_remove, t_copy = [], []
                for rep in range(args.warmup + args.reps):
                    cov_new, state_new = pairs[cur ^ 1]
                    ev[0].record(be.stream)
                    be._check(lib.ekf_remove_markers(be.h, idx.ctypes.data_as(C.POINTER(C.c_int32)), count, cov_new.data_ptr(),
                                                     be.ld, state_new.data_ptr(), ws.data_ptr(), nbytes.value))
                    ev[1].record(be.stream)
                    cur ^= 1
                    be.cov_t, be.state_t = pairs[cur]
                    be.add_markers(fresh)                      # back to n landmarks, outside the timed region
                    ev[2].record(be.stream)
                    rc = hip.hipMemcpyAsync(scratch.data_ptr(), be.cov_t.data_ptr(), cov_bytes, 3, be.stream.cuda_stream)
                    assert rc == 0, rc                          # (3: hipMemcpyDeviceToDevice)
                    ev[3].record(be.stream)
                    be.sync()
                    assert be.num_landmarks == n
                    if rep >= args.warmup:
                        t_remove.append(1e3 * ev[0].elapsed_time(ev[1]))
                        t_copy.append(1e3 * ev[2].elapsed_time(ev[3]))
                rec = {"tool": "remove_bench", "n": n, "dims": be.dims, "ld": be.ld, "cov_dtype": "float32", "removed": count,
                       "cov_bytes": cov_bytes, "reps": args.reps, "remove_call": stats(t_remove), "copy_d2d": stats(t_copy)}
                rec["ratio_median"] = rec["remove_call"]["median_us"] / rec["copy_d2d"]["median_us"]
                if not args.no_host_route and count == args.counts[-1]:
                    # the route the call replaces: read P back, delete on the host, restore into a second filter
                    twin = EKF(INIT, max_landmarks=n, max_visible=32, cov_dtype="float32", quat_update="scalar_first")
                    rows = np.concatenate([np.arange(10 + 3 * i, 13 + 3 * i) for i in idx])
                    be.sync()
                    t0 = time.perf_counter()
                    state, cov = be.get_state(), be.get_cov()
                    cov = np.delete(np.delete(cov, rows, axis=0), rows, axis=1)
                    twin.backend.set_state_cov(np.delete(state, rows), cov)
                    twin.backend.sync()
                    rec["host_route_ms"] = 1e3 * (time.perf_counter() - t0)
                    del twin, cov
                line = json.dumps(rec)
                print(line, flush=True)
                with out.open("a") as fh:
                    fh.write(line + "\n")
        del flt, pairs, scratch


if __name__ == "__main__":
    main()
