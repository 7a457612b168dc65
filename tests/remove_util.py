"""Helpers of ``test_remove_markers.py``: filters with a dense covariance from a short synthetic run, and the TWIN of a
removal, built by the restore path that existed before it: read state and P back, ``np.delete`` the rows and columns on the
host, and ``set_state_cov`` them into a fresh filter of the same configuration."""
import numpy as np

import support as sp

INIT = sp.INIT
LMD = {"ekf": 3, "ekf_rotations": 10}
GATES = {"ekf": 11.345, "ekf_rotations": 18.475}


def make_filter(model, **kw):
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    if model == "ekf_rotations":
        return EKF_Rotations(INIT, **kw)
    return EKF(INIT, quat_update="scalar_first", **kw)


class Scene:
    """Seeded landmarks and camera path (``synthetic.SyntheticStream``): frames of chosen marker ids (= landmark numbers of
    the stream)."""

    def __init__(self, model, n, m, seed=0):
        from aruco_slam_amd.synthetic import SyntheticStream
        self.stream = SyntheticStream(n, m, seed=seed, rvec_sigma=0.05 if model == "ekf_rotations" else 0.0)
        self.n, self.m = n, m

    def bootstrap(self):
        return [(ids.tolist(), poses) for ids, poses in self.stream.bootstrap()]

    def frame(self, ids):
        ids, poses = self.stream._observe(np.asarray(ids))
        return ids.tolist(), poses

    def frames(self, count, pool, m=None):
        """``count`` frames of ``m`` distinct ids drawn from ``pool``."""
        m = self.m if m is None else m
        return [self.frame(np.sort(self.stream.rng.choice(np.asarray(pool), m, replace=False))) for _ in range(count)]


def as_log(frames):
    counts = np.array([len(ids) for ids, _ in frames], dtype=np.int64)
    return {"ids": np.concatenate([np.asarray(ids, dtype=np.int32) for ids, _ in frames]),
            "poses": np.concatenate([p for _, p in frames]),
            "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64)}


def dense_filter(model, n, m, steady=6, seed=0, **kw):
    """(filter, scene): every one of ``n`` landmarks first sighted (marker id = landmark index), then ``steady`` frames, so
    that P is dense."""
    scene = Scene(model, n, m, seed)
    flt = make_filter(model, max_landmarks=n, max_visible=m, **kw)
    log = as_log(scene.bootstrap() + scene.frames(steady, np.arange(n)))
    flt.process_detection_log(log["ids"], log["poses"], log["offsets"])
    return flt, scene


def deleted(model, state, cov, index):
    """(state, cov) with the landmarks ``index`` deleted on the host."""
    lmd = LMD[model]
    rows = np.concatenate([np.arange(10 + lmd * i, 10 + lmd * (i + 1)) for i in index]).astype(int) if len(index) else \
        np.zeros(0, dtype=int)
    return np.delete(state, rows), np.delete(np.delete(cov, rows, axis=0), rows, axis=1)


def twin_of(model, flt, ids, **kw):
    """The twin of ``flt.remove_markers(ids)``, built BEFORE the removal by the restore path."""
    from aruco_slam_amd.filters.map_management import renumber_landmarks
    be = flt.backend
    index = [flt.landmarks[k] for k in ids]
    state, cov = deleted(model, be.get_state(), be.get_cov(), index)
    twin = make_filter(model, max_landmarks=be.max_landmarks, max_visible=be.max_visible, cov_dtype=be.cov_dtype, **kw)
    twin.backend.set_state_cov(state, cov)
    twin.landmarks = renumber_landmarks(flt.landmarks, index)
    twin.num_landmarks = flt.num_landmarks - len(index)
    twin._pruned = True
    return twin


def remove_into_nan(flt, ids):
    """``flt.remove_markers(ids)`` with the new tensors filled with NaN beforehand: an element the call does not write shows."""
    import torch
    be = flt.backend
    be._remove_into([flt.landmarks[k] for k in ids], torch.full_like(be.cov_t, float("nan")),
                    torch.full_like(be.state_t, float("nan")))
    flt._drop_from_table(list(ids))


def assert_same(a, b, raw=True):
    """Two filters hold the same bits: state, full covariance, landmark table; ``raw``: the whole device tensors too, the
    capacity padding included."""
    assert a.landmarks == b.landmarks and a.num_landmarks == b.num_landmarks
    assert np.array_equal(a.backend.get_state(), b.backend.get_state(), equal_nan=True)
    assert np.array_equal(a.backend.get_cov(), b.backend.get_cov(), equal_nan=True)
    if raw:
        assert np.array_equal(a.backend.state_t.cpu().numpy(), b.backend.state_t.cpu().numpy(), equal_nan=True)
        assert np.array_equal(a.backend.cov_t.cpu().numpy(), b.backend.cov_t.cpu().numpy(), equal_nan=True)


def assert_zero_padding(flt):
    """The raw tensors are exactly zero outside N' x N' and beyond N'."""
    be = flt.backend
    n = be.dims
    cov, state = be.cov_t.cpu().numpy(), be.state_t.cpu().numpy()
    assert not np.isnan(cov).any() and not np.isnan(state).any()
    assert not cov[n:, :].any() and not cov[:, n:].any() and not state[n:].any()
