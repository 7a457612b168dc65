"""The narrow entry points of the C ABI that the Python layer no longer calls still forward: each gives the bits of the
widest entry point of its family with NULL for what it lacks.  Equality only, no tolerance.  The shapes are the smallest that
pass through first sightings, an empty frame, a member without a log and both optional inputs."""
import ctypes as C

import numpy as np
import pytest

import support as sp

pytestmark = pytest.mark.gpu

INIT = sp.INIT
# member 0 (and the one log of the replicas): two first sightings, an empty frame, a re-observation and a first sighting
LM_INDEX = np.array([0, 1, 0, 2], dtype=np.int32)
FRAME_OFFSETS = np.array([0, 2, 2, 4], dtype=np.int64)
MEMBER_FRAMES = np.array([0, 3, 3], dtype=np.int64)          # member 1: no log
POSES = np.array([[0.3, -0.2, 2.0, 0.10, -0.20, 0.05], [-0.4, 0.1, 2.5, -0.10, 0.30, 0.20],
                  [0.32, -0.21, 1.98, 0.10, -0.20, 0.05], [0.1, 0.4, 3.0, 0.20, 0.10, -0.30]])
ROWS = np.array([[1e-3, 2e-3, 4e-3], [2e-3, 1e-3, 3e-3], [5e-4, 1e-3, 2e-3], [3e-3, 3e-3, 1e-3]])
SCALES = np.array([1.0, 0.5, 2.0])
F, D = 3, 4


@pytest.fixture(scope="module")
def batch():
    from aruco_slam_amd.batch import EKFBatch
    b = EKFBatch(2, INIT, model="ekf", max_landmarks=4, max_visible=4, row_noise=True, frame_scale=True,
                 quat_update="scalar_first")
    yield b
    b.close()


def _members(batch):
    """State, covariance of both members, status and landmark counts after a direct library call."""
    counts = batch._num_landmarks_device()
    batch.num_landmarks = [int(v) for v in counts]
    return [batch.get_state(0), batch.get_cov(0), batch.get_state(1), batch.get_cov(1), np.array(batch.status()), counts]


def _run(batch, nbytes_of, call, shapes):
    """A freshly reset batch, outputs ``shapes`` (name -> shape) prefilled with NaN on the batch's stream, ``call(dev, ws,
    bytes, out)`` -> the library's return code (dev: host array -> device tensor).  Returns the outputs and the members."""
    import torch
    batch.reset()
    nbytes = C.c_size_t()
    batch._check(nbytes_of(C.byref(nbytes)))
    with torch.cuda.device(batch.device), torch.cuda.stream(batch.stream):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(batch.device)
        ws = torch.empty((max(nbytes.value, 256),), dtype=torch.uint8, device=batch.device)
        out = {k: torch.full(s, float("nan"), dtype=torch.float64, device=batch.device) for k, s in shapes.items()}
        batch._check(call(dev, ws, nbytes.value, out))
        batch.stream.synchronize()
    return [t.cpu().numpy() for t in out.values()] + _members(batch)


# the arguments of ekf_batch_observe_logs_moved after the log itself, and which of them each narrower entry point has
WIDE = ("poses", "rows", "scale", "motion", "ws", "bytes", "traj", "nis", "cov", "mahal")
NARROW = {
    "ekf_batch_observe_logs": ("poses", "ws", "bytes", "traj"),
    "ekf_batch_observe_logs_diag": ("poses", "ws", "bytes", "traj", "nis", "cov"),
    "ekf_batch_observe_logs_gated": ("poses", "ws", "bytes", "traj", "nis", "cov", "mahal"),
    "ekf_batch_observe_logs_rows": ("poses", "rows", "ws", "bytes", "traj", "nis", "cov", "mahal"),
    "ekf_batch_observe_logs_scaled": ("poses", "rows", "scale", "ws", "bytes", "traj", "nis", "cov", "mahal"),
}
OUT_SHAPES = {"traj": (F, 7), "nis": (F,), "cov": (F, 10, 10), "mahal": (D,)}


@pytest.mark.parametrize("name", list(NARROW))
def test_batch_log_entry_points_forward_to_the_widest(batch, name):
    from aruco_slam_amd.hip_backend import _iptr, _lptr
    has = NARROW[name]
    shapes = {k: s for k, s in OUT_SHAPES.items() if k in has}
    host = {"poses": POSES, "rows": ROWS, "scale": SCALES}

    def call(fn, keys):
        def go(dev, ws, nbytes, out):
            tensors = {**{k: dev(host[k]) for k in host if k in has}, **out}      # (uploaded on the batch's stream)
            value = {"ws": ws.data_ptr(), "bytes": nbytes, **{k: t.data_ptr() for k, t in tensors.items()}}
            return fn(batch.h, _iptr(LM_INDEX), _lptr(FRAME_OFFSETS), _lptr(MEMBER_FRAMES), *(value.get(k) for k in keys))
        return go

    sizes = lambda n: batch.lib.ekf_batch_log_workspace_bytes(batch.h, D, F, n)
    narrow = _run(batch, sizes, call(getattr(batch.lib, name), has), shapes)
    wide = _run(batch, sizes, call(batch.lib.ekf_batch_observe_logs_moved, WIDE), shapes)
    assert sp.same(narrow, wide, equal_nan=True)
    # (not vacuous: member 0 ran, with its three landmarks; member 1 did not)
    assert np.isfinite(narrow[0]).all() and list(narrow[-1]) == [3, 0] and not narrow[-2].any()


def test_batch_replica_entry_point_forwards_to_the_gated_one(batch):
    from aruco_slam_amd.batch import replica_sigma
    from aruco_slam_amd.hip_backend import _dptr, _iptr, _lptr
    sigma = replica_sigma(0.01, 2)
    shapes = {"traj": (2, F, 7), "nis": (2, F), "cov": (2, F, 10, 10)}

    def call(fn, tail):
        def go(dev, ws, nbytes, out):
            poses = dev(POSES)
            return fn(batch.h, _iptr(LM_INDEX), _lptr(FRAME_OFFSETS), F, poses.data_ptr(), _dptr(sigma), 7, 3, ws.data_ptr(),
                      nbytes, out["traj"].data_ptr(), out["nis"].data_ptr(), out["cov"].data_ptr(), *tail)
        return go

    sizes = lambda n: batch.lib.ekf_batch_replica_workspace_bytes(batch.h, D, F, n)
    narrow = _run(batch, sizes, call(batch.lib.ekf_batch_observe_replicas, ()), shapes)
    wide = _run(batch, sizes, call(batch.lib.ekf_batch_observe_replicas_gated, (None,)), shapes)
    assert sp.same(narrow, wide, equal_nan=True)
    assert np.isfinite(narrow[0]).all() and list(narrow[-1]) == [3, 3]
    assert not np.array_equal(narrow[0][0], narrow[0][1])          # (the replicas drew their own noise)


def test_batch_refusals_of_the_log_call_and_of_the_history_size(batch):
    """The validation that ``ekf_batch_history_bytes`` and the log call share, on a bound handle (so on a device): a malformed
    ``member_frames``, a frozen member with a first sighting and a log over capacity are refused by both with the same code
    and message, and nothing runs."""
    import torch
    from aruco_slam_amd.hip_backend import _iptr, _lptr
    lib = batch.lib
    over = (np.arange(5, dtype=np.int32), np.array([0, 4, 5], dtype=np.int64), np.array([0, 2, 2], dtype=np.int64))
    cases = [
        ((LM_INDEX, FRAME_OFFSETS, np.array([0, 3, 2], dtype=np.int64)), False, -1, "member_frames must be non-decreasing"),
        ((LM_INDEX, FRAME_OFFSETS, np.array([1, 3, 3], dtype=np.int64)), False, -1, "member_frames[0] must be 0"),
        ((LM_INDEX, FRAME_OFFSETS, MEMBER_FRAMES), True, -4,
         "member 0's log holds a first sighting, and the member's map is frozen"),
        (over, False, -2, "member 0's log needs more landmarks than max_landmarks"),
    ]
    for (idx, fo, mf), frozen, code, message in cases:
        batch.reset()
        if frozen:
            batch.freeze_map(0)
        before = _members(batch)
        n = C.c_size_t()
        assert lib.ekf_batch_history_bytes(batch.h, _iptr(idx), _lptr(fo), _lptr(mf), 0, C.byref(n)) == code
        assert lib.ekf_last_error_string().decode() == message
        with torch.cuda.device(batch.device), torch.cuda.stream(batch.stream):
            poses = torch.zeros((idx.shape[0], 6), dtype=torch.float64, device=batch.device)
            ws = torch.empty((1 << 16,), dtype=torch.uint8, device=batch.device)
            traj = torch.empty((8, 7), dtype=torch.float64, device=batch.device)
            hist = torch.empty((1 << 20,), dtype=torch.uint8, device=batch.device)
            log = (batch.h, _iptr(idx), _lptr(fo), _lptr(mf), poses.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(),
                   traj.data_ptr(), None, None, None)
            for rc in (lib.ekf_batch_observe_logs_moved(*log),
                       lib.ekf_batch_observe_logs_recorded(*log, hist.data_ptr(), hist.numel())):
                assert rc == code and lib.ekf_last_error_string().decode() == message
            batch.stream.synchronize()
        assert sp.same(_members(batch), before, equal_nan=True)
    batch.reset()


# ---- the single filter's sequence call ------------------------------------------------------------------------------------
SEQ_INDEX = np.array([[0, 1], [1, 2], [0, 2]], dtype=np.int32)
LANDMARKS = np.array([[0.3, -0.2, 2.0], [-0.4, 0.1, 2.5], [0.1, 0.4, 3.0]])


def _sequence(name, has):
    import torch
    from aruco_slam_amd.hip_backend import HipEkf, _dptr
    flt = HipEkf(3, 2, cov_dtype="float64", quat_mode="scalar_first", row_noise=True, frame_scale=True)
    try:
        flt.reset(INIT)
        flt.add_markers(LANDMARKS)
        rng = np.random.default_rng(5)
        z = LANDMARKS[SEQ_INDEX] + 0.01 * rng.standard_normal((3, 2, 3))
        rows = 1e-3 * (1.0 + rng.random((3, 2, 3)))
        idx_t = torch.tensor(SEQ_INDEX, dtype=torch.int32, device=flt.device)
        z_t = torch.tensor(z, dtype=torch.float64, device=flt.device)
        rows_t = torch.tensor(rows, dtype=torch.float64, device=flt.device)
        traj = torch.full((3, 7), float("nan"), dtype=torch.float64, device=flt.device)
        torch.cuda.synchronize(flt.device)
        value = {"rows": rows_t.data_ptr(), "scale": _dptr(SCALES)}
        keys = ("rows", "scale", "motion") if name.endswith("_moved") else has
        flt._check(getattr(flt.lib, name)(flt.h, idx_t.data_ptr(), z_t.data_ptr(), *(value.get(k) if k in has else None for k in keys),
                                          2, 3, traj.data_ptr()))
        mode = flt.last_sequence_mode()
        flt.sync()
        return [traj.cpu().numpy(), flt.get_state(), flt.get_cov()], mode
    finally:
        flt.close()


@pytest.mark.parametrize("name,has", [("ekf_observe_sequence_device", ()), ("ekf_observe_sequence_device_rows", ("rows",)),
                                      ("ekf_observe_sequence_device_scaled", ("rows", "scale"))])
def test_sequence_entry_points_forward_to_the_widest(name, has):
    narrow, narrow_mode = _sequence(name, has)
    wide, wide_mode = _sequence("ekf_observe_sequence_device_moved", has)
    assert sp.same(narrow, wide, equal_nan=True) and narrow_mode == wide_mode and narrow_mode != "none"
    assert np.isfinite(narrow[0]).all() and not np.array_equal(narrow[0][0], narrow[0][2])
