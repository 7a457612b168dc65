"""Map management on the host: which landmarks to prune, and what pruning does to the marker-id -> landmark-index table.

Pure Python, no device.  The removal itself is ``BaseFilter.remove_markers`` (``ekf_remove_markers`` in
``include/ekf_slam_hip.h``): deleting a landmark's rows and columns of P and its state entries, on the device.

The per-detection gate exempts first sightings by design (their z = h by construction), so a mis-decoded id, or a marker
seen once from a flipped IPPE pose, enters the map unchecked.  ``TentativeLandmarks`` is the usual remedy: a landmark has to
be seen again before it may stay.
"""
from __future__ import annotations


def renumber_landmarks(landmarks: dict, removed_indices) -> dict:
    """The marker-id -> landmark-index table after the landmarks with ``removed_indices`` are gone (rule 2 of the removal
    semantics): their ids are dropped, every other id keeps its order, new index = old index - (number of removed indices
    below it).  ``landmarks`` is not modified.  ``ValueError`` for a duplicate or an index the table does not hold."""
    removed = sorted(int(i) for i in removed_indices)
    if any(a == b for a, b in zip(removed, removed[1:])):
        raise ValueError("duplicate landmark index in the removal list")
    held = set(landmarks.values())
    if any(i not in held for i in removed):
        raise ValueError("the landmark table holds no such index")
    gone = set(removed)
    out = {}
    for marker, index in landmarks.items():
        if index in gone:
            continue
        below = 0
        for r in removed:      # (removal lists are a handful of entries)
            if r > index:
                break
            below += 1
        out[marker] = index - below
    return out


class TentativeLandmarks:
    """Confirmation policy: a landmark first sighted in frame ``t0`` is tentative.  Every LATER frame in which at least one
    detection of it was used (not rejected by the gate) counts one hit; at ``hits`` hits it is confirmed for good.  At the
    end of frame ``t``, every landmark that is still tentative with ``t - t0 + 1 >= window`` is returned for removal and
    forgotten: seen again later, it starts over as a first sighting.  Frames are counted by the calls of ``end_frame``
    (frames without detections included)."""

    def __init__(self, hits: int, window: int) -> None:
        hits, window = int(hits), int(window)
        if hits < 1 or window < 2:
            raise ValueError("confirm needs hits >= 1 and window >= 2 (the first sighting counts no hit)")
        self.hits, self.window = hits, window
        self.frame = 0              # index of the next frame
        self.tentative = {}         # marker id -> [t0, hits so far], in order of first sighting
        self.confirmed = set()

    def confirm(self, ids) -> None:
        """Landmarks that are confirmed from the start (restored from a map file or a checkpoint)."""
        for marker in ids:
            self.tentative.pop(marker, None)
            self.confirmed.add(marker)

    def forget(self, ids) -> None:
        """Landmarks removed by other means: seen again, they are first sightings."""
        for marker in ids:
            self.tentative.pop(marker, None)
            self.confirmed.discard(marker)

    def clear(self) -> None:
        self.frame = 0
        self.tentative.clear()
        self.confirmed.clear()

    def end_frame(self, ids=(), used=None) -> list:
        """One frame: ``ids`` the marker ids of its detections (empty: none), ``used`` bool per detection (None: all were
        used).  Returns the marker ids to remove now, in order of first sighting."""
        t = self.frame
        self.frame += 1
        ids = list(ids)
        used = [True] * len(ids) if used is None else [bool(u) for u in used]
        if len(used) != len(ids):
            raise ValueError("used must have one entry per detection")
        hit = set()
        for marker, ok in zip(ids, used):
            if marker in self.confirmed:
                continue
            entry = self.tentative.get(marker)
            if entry is None:
                self.tentative[marker] = [t, 0]      # first sighting: tentative from this frame, no hit yet
            elif ok and entry[0] < t:
                hit.add(marker)
        for marker in hit:
            entry = self.tentative[marker]
            entry[1] += 1
            if entry[1] >= self.hits:
                del self.tentative[marker]
                self.confirmed.add(marker)
        stale = [marker for marker, (t0, _) in self.tentative.items() if t - t0 + 1 >= self.window]
        for marker in stale:
            del self.tentative[marker]
        return stale
