"""Scaffolding shared by the test modules (``import support as sp``): the library fixture, the C ABI check, workspace
sizes, bitwise snapshots of filters and batches, log slices, a compiled kernel's resource metadata and the host programs
under ``tests/host``.  Reference arithmetic stays in the ``*_util.py`` files."""
import ctypes
import functools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ekf_slam_hip.h"
INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float64)


# ---- the library ----------------------------------------------------------------------------------------------------------
def load_lib():
    from aruco_slam_amd import _build, hip_backend
    _build.build()
    return hip_backend.load_library()


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def assert_abi(lib, names, *, returns="int"):
    """Every name is declared in the public header (returning ``returns``), listed in EXPORTED_SYMBOLS and in the library."""
    from aruco_slam_amd import hip_backend
    header = HEADER.read_text()
    gap = "" if returns.endswith("*") else " "          # "int ekf_x(", "const char *ekf_x("
    for name in names:
        assert re.search(rf"\b{re.escape(returns)}{gap}{name}\(", header), name
        assert name in hip_backend.EXPORTED_SYMBOLS and hasattr(lib, name), name


def config(lib, **fields):
    """ekf_default_config with ``fields`` set on it."""
    from aruco_slam_amd import hip_backend
    cfg = hip_backend.EkfConfig()
    assert lib.ekf_default_config(ctypes.byref(cfg)) == 0
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


def _sizes(query, *args):
    ld, cov, state, ws = ctypes.c_int64(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = query(*args, ctypes.byref(ld), ctypes.byref(cov), ctypes.byref(state), ctypes.byref(ws))
    return rc, ld.value, cov.value, state.value, ws.value


def query_sizes(lib, **fields):
    """(rc, ld, cov_bytes, state_bytes, ws_bytes) of ekf_query_sizes for the default configuration with ``fields`` set."""
    return _sizes(lib.ekf_query_sizes, ctypes.byref(config(lib, **fields)))


# (model, max_landmarks, max_visible, cov_dtype, flags) -> (ld, cov, state, workspace bytes) of ekf_query_sizes, taken from
# the library of the commit before the gate: what a configuration without a later flag still has to give
PARENT_SIZES = (
    ((0, 50, 50, 0, 8), (256, 524288, 2048, 3279872)),
    ((0, 1024, 32, 1, 8), (3200, 40960000, 25600, 48925184)),
    ((1, 63, 55, 0, 8), (640, 3276800, 5120, 25851904)),
    ((0, 82, 64, 1, 0), (256, 262144, 2048, 3217920)),
    ((1, 24, 27, 0, 4), (256, 524288, 2048, 3885312)),
    ((0, 4000, 1024, 1, 10), (12032, 579076096, 96256, 2143691520)),
)


def sizes(lib, model, n, mv, dtype, flags):
    """(ld, cov, state, workspace bytes) of a configuration written as a key of PARENT_SIZES; the query has to succeed."""
    rc, *got = query_sizes(lib, model=model, max_landmarks=n, max_visible=mv, cov_dtype=dtype, flags=flags)
    assert rc == 0
    return tuple(got)


def batch_query_sizes(lib, cfg, members=4):
    """(rc, ld, cov_bytes, state_bytes, ws_bytes) of ekf_batch_query_sizes."""
    return _sizes(lib.ekf_batch_query_sizes, ctypes.byref(cfg), members)


# ---- snapshots: bitwise comparison ----------------------------------------------------------------------------------------
def snap_filter(flt):
    return np.array(flt.state, dtype=np.float64), flt.uncertainty


def snap_backend(backend):
    return backend.get_state(), backend.get_cov()


def snap_batch(batch, tables=False):
    """[(state, covariance)] of every member; with ``tables`` each member's id table as well."""
    return [(batch.get_state(b), batch.get_cov(b)) + ((dict(batch.landmarks[b]),) if tables else ())
            for b in range(batch.members)]


def difference(a, b, equal_nan=False, where=""):
    """None if ``a`` and ``b`` are the same, otherwise where they first differ.  A list holds members, a tuple the arrays of
    one of them (in a snapshot: 0 the state, 1 the covariance); lengths are compared first, then shapes, then every element
    (NaN equals NaN only with ``equal_nan``).  An id table (a dict) is compared with ``==``."""
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return f"{where} length {len(a)} != {len(b)}"
        for i, (u, v) in enumerate(zip(a, b)):
            found = difference(u, v, equal_nan, f"{where} {'member' if isinstance(a, list) else 'array'} {i}")
            if found:
                return found
        return None
    if isinstance(a, dict):
        return None if a == b else f"{where} table"
    u, v = np.asarray(a), np.asarray(b)
    if u.shape != v.shape:
        return f"{where} shape {u.shape} != {v.shape}"
    return None if np.array_equal(u, v, equal_nan=equal_nan) else f"{where} values"


def same(a, b, *, equal_nan=False):
    return difference(a, b, equal_nan) is None


def assert_same(a, b, what, *, equal_nan=False):
    found = difference(a, b, equal_nan)
    assert found is None, (what, found.strip())


# ---- logs and batches -----------------------------------------------------------------------------------------------------
def sub_log(log, t0, t1):
    """Frames t0 .. t1 - 1 of a ragged log as a log of their own."""
    offs = log["offsets"]
    d0, d1 = int(offs[t0]), int(offs[t1])
    return {"ids": log["ids"][d0:d1], "poses": log["poses"][d0:d1], "offsets": offs[t0:t1 + 1] - d0,
            "has_detections": log["has_detections"][t0:t1]}


def parse_trajectory(text):
    """trajectory.txt of run_slam as an array, one row per line"""
    return np.array([[float(t) for t in line.split()] for line in text.splitlines()])


def parse_map(text):
    """map.txt of run_slam: (ids, positions, uncertainties)"""
    lines = text.splitlines()[4:]
    ids = [int(lines[i]) for i in range(0, len(lines) - 2, 4)]
    xyz = np.array([[float(t) for t in lines[i + 1].split(", ")] for i in range(0, len(lines) - 2, 4)])
    unc = np.array([[float(t) for t in lines[i + 2].split(", ")] for i in range(0, len(lines) - 2, 4)])
    return ids, xyz, unc


def family_batch(members, model, family, **extra):
    """An EKFBatch with the constructor arguments of gating_util.FAMILIES[(model, family)], ``extra`` on top."""
    import gating_util as gu
    from aruco_slam_amd.batch import EKFBatch
    kw = dict(gu.FAMILIES[(model, family)][0])
    kw.update(extra)
    return EKFBatch(members, INIT, model=model, **kw)


def restore(flt, prior):
    """``prior`` = (state, P, landmark ids, ...) into ``flt``, with the id table."""
    state, p, lm_ids = prior[:3]
    flt.landmarks = {int(k): i for i, k in enumerate(lm_ids)}
    flt.num_landmarks = len(lm_ids)
    flt.backend.set_state_cov(state, p)


def host_batch(members=3, model="ekf"):
    """An EKFBatch without device state: observe_indexed records what would reach the library."""
    from aruco_slam_amd.batch import EKFBatch, LM_DIMS
    batch = object.__new__(EKFBatch)
    batch.members = members
    batch.model = model
    batch.lm_dims = LM_DIMS[model]
    batch.landmarks = [{} for _ in range(members)]
    batch.num_landmarks = [0] * members
    batch.calls = []

    def observe_indexed(index, frame_offsets, member_frames, poses, nis=False, cam_cov=False):
        batch.calls.append((index, frame_offsets, member_frames, poses, nis, cam_cov))
        f = int(member_frames[-1])
        traj = np.zeros((f, 7))
        if not (nis or cam_cov):
            return traj
        return traj, np.arange(f, dtype=np.float64) if nis else None, np.zeros((f, 10, 10)) if cam_cov else None

    batch.observe_indexed = observe_indexed
    batch._num_landmarks_device = lambda: np.zeros(members, dtype=np.int32)
    return batch


# ---- compiled kernels and host programs -----------------------------------------------------------------------------------
RESOURCE_FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
                   "vgpr_count", "agpr_count", "sgpr_count")


@functools.lru_cache(maxsize=None)
def compiled_kernels(src, flags=()):
    """``csrc/src`` compiled for gfx950: ((kernel name, ((field, value), ...)), ...) of its ``amdhsa.kernels`` metadata.
    One compilation per (src, flags) per process; the assembly text is not kept."""
    from aruco_slam_amd import _build
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "k.s"
        subprocess.run([_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, "-S", "--cuda-device-only",
                        str(_build.CSRC / src), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")]
    kernels = []
    for entry in re.split(r"\n  - ", meta)[1:]:        # one entry per kernel; its own fields are indented by 4
        fields = dict(re.findall(r"^    \.([a-z_]+):\s+(\S+)", "    " + entry, re.M))
        kernels.append((fields["name"], tuple((k, int(fields[k])) for k in RESOURCE_FIELDS)))
    return tuple(kernels)


def kernel_resources(src, pattern=None, flags=()):
    """{kernel name: {field: int}} (RESOURCE_FIELDS) of the kernels of ``csrc/src`` whose name matches ``pattern``."""
    return {name: dict(fields) for name, fields in compiled_kernels(src, tuple(flags))
            if pattern is None or re.search(pattern, name)}


# scratch bytes, VGPR spills, static LDS bytes: "none of the three" reads [res[k] for k in BUDGET_FIELDS] == [0, 0, 0]
BUDGET_FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")


def build_host_program(main_name, out_dir):
    """Compile tests/host/<main_name>.hip for the host against the device headers of csrc; returns the program's path."""
    from aruco_slam_amd import _build
    exe = Path(out_dir) / main_name.replace("_main", "")
    subprocess.run([_build.hipcc(), "--cuda-host-only", "-O3", "-std=c++17", f"-I{_build.CSRC}",
                    str(REPO / "tests" / "host" / f"{main_name}.hip"), "-o", str(exe)], check=True, capture_output=True)
    return exe
