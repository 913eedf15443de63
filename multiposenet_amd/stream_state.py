"""What the stages that ride on the tracker share (`zones.ZoneCounter`, `trails.TrackTrails`, `density.DensityMap`,
`track_metrics.TrackEvaluator`): per-stream state on the device as a prev / next pair - a launch reads `prev` and writes
`next`, `commit()` advances - and the checks of their constructors' plain arguments."""
import numpy as np


def integer(owner, name, value, lo, hi):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError(f"{owner}: {name} must be an integer in {lo}..{hi} (got {value!r})")
    return int(value)


def flag(owner, name, value):
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{owner}: {name} must be False or True (got {value!r})")
    return bool(value)


def choice(owner, name, value, choices):
    if not isinstance(value, str) or value not in choices:
        raise ValueError(f"{owner}: {name} must be one of {list(choices)} (got {value!r})")
    return value


class StreamState:
    """The state of `streams` cameras, `stream_bytes` each, as the uint8 device tensors `prev` and `next`. A subclass sets
    `keyword` (the predict_* keyword it is passed as: it begins the messages) and `_serials`, a counter of its own, and has
    `streams` and `device` in place before `_make_state`."""
    keyword = None
    _serials = None

    def _make_state(self, stream_bytes):
        import torch
        self.stream_bytes = stream_bytes
        self.prev = torch.zeros(self.streams * stream_bytes, dtype=torch.uint8, device=self.device)
        self.next = torch.zeros(self.streams * stream_bytes, dtype=torch.uint8, device=self.device)
        self.serial = next(self._serials)                           # process-unique: part of the key of a Detector's graph

    def check_batch(self, b):
        """The number of images of a call -> frames per stream."""
        if b < 1 or b % self.streams != 0:
            raise ValueError(f"{self.keyword}=: {b} images are not a whole number of frames for each of {self.streams} streams")
        return b // self.streams

    def commit(self):
        """The last launch's state becomes the current one: one small device copy on the current stream."""
        self.prev.copy_(self.next, non_blocking=True)

    def _part(self, stream):
        """The bytes of one stream's state in `prev` / `next`, as a slice."""
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream must be in 0..{self.streams - 1} (got {stream})")
        return slice(int(stream) * self.stream_bytes, (int(stream) + 1) * self.stream_bytes)

    def reset(self, stream=None):
        """Set the state to zero - everything the stage remembers, its frame count included: of all streams, or of one."""
        part = slice(None) if stream is None else self._part(stream)
        self.prev[part].zero_()
        self.next[part].zero_()

    def _raw_state(self, stream):
        """A host copy of one stream's current state, as a uint8 array."""
        return self.prev[self._part(stream)].cpu().numpy()
