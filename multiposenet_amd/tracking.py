"""Person identities across the frames of a video, on the device: `mpn_pose_track` (include/mpn.h) matches the persons of every
frame greedily, by box IoU or keypoint OKS, against the tracks the earlier frames left; `mpn_pose_track_optimal`
(`PoseTracker(assignment='optimal')`) solves the frame's linear assignment instead.

    tracker = PoseTracker(streams=1, similarity='oks')           # one camera; a batch is consecutive frames
    for frames in batches:
        for person in detector.predict_images(frames, track=tracker):
            person['track_ids']                                  # int32 [n], 0 = untracked; also track_hits / _new / _similarity

Inside the Detector the launch follows the gather in the captured graph and its rows arrive in the record's one copy. The
launch is a PURE function of (record, prev): it writes the new state to `next` and never touches `prev`, because the Detector
runs its device side eagerly and then replays the graph on an entry's first call (and again when the variables change) - an
in-place update would step the state twice there. The state advances when `commit()` queues `prev.copy_(next)` behind the
launch, outside the graph; the Detector does that once per call. `update()` is the same launch for host dicts.

    tracker = PoseTracker(streams=1, smooth=OneEuro(rate=30.0))  # + 'keypoints_smoothed' f32 [n,17,3], 'keypoint_velocities' [n,17,2]

`smooth=` adds `mpn_pose_smooth` behind the track launch: one One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) per track slot
and joint, keyed by the slot and the id the track launch gave the row, with a prev / next state of its own that `commit()`
advances in the same way. The units are pixels of the call's 'keypoints': `beta` multiplies a speed in pixels per second and
so depends on the resolution.

    tracker = PoseTracker(streams=1, motion=ConstantVelocity())  # + 'coasting_ids' / _misses / _boxes / _keypoints

`motion=` makes the launch `mpn_pose_track_motion`: every track carries a velocity per frame of its box and of its keypoint
centroid, a frame's detections are compared with where the track is expected in that frame (the last observed pose plus the
velocity times the frames since), and the tracks that are alive but were not detected in a frame come back at that expected
pose. The velocities are a third prev / next state that `commit()` advances.
"""
import itertools
import math

import numpy as np

from . import _lib
from .pose_metrics import fill_record

SIMILARITIES = {'iou': 0, 'oks': 1}
ASSIGNMENTS = {'greedy': 'mpn_pose_track', 'optimal': 'mpn_pose_track_optimal'}      # the entry `launch` calls
MAX_TRACKS = 64                          # slots per stream the kernel takes (one lane of a wave per slot)
MAX_BOXES = 64                           # detections per image
NUM_KEYPOINTS = 17
FLAG_NEW, FLAG_OVERFLOW = 1, 2

# a row of mpn_pose_track's output and the state of one stream (include/mpn.h)
_OUT = np.dtype([('track_id', np.int32), ('slot', np.int32), ('hits', np.int32), ('flags', np.int32),
                 ('similarity', np.float64)])
_HEAD = np.dtype([('next_id', np.int32), ('dropped', np.int32), ('pad', np.int32, (2,))])
_SLOT = np.dtype([('id', np.int32), ('hits', np.int32), ('age', np.int32), ('misses', np.int32), ('box', np.float32, (4,)),
                  ('score', np.float32), ('keypoints', np.float32, (NUM_KEYPOINTS, 3))])

# a coasting row of mpn_pose_track_motion and its motion state of one stream
_COAST = np.dtype([('id', np.int32), ('misses', np.int32), ('box', np.float32, (4,)), ('keypoints', np.float32, (NUM_KEYPOINTS, 2))])
_MOTION_HEAD = np.dtype([('pad', np.int32, (4,))])
_MOTION_SLOT = np.dtype([('id', np.int32), ('seen', np.int32), ('vel', np.float32, (6,))])

# a row of mpn_pose_smooth's output and its state of one stream
_SMOOTH_OUT = np.dtype([('keypoints', np.float32, (NUM_KEYPOINTS, 3)), ('velocities', np.float32, (NUM_KEYPOINTS, 2))])
_SMOOTH_HEAD = np.dtype([('frames', np.int32), ('pad', np.int32, (3,))])
_SMOOTH_SLOT = np.dtype([('id', np.int32),
                         ('joints', [('last', np.int32), ('hat', np.float32, (4,))], (NUM_KEYPOINTS,)),     # x, y, dx, dy
                         ('pad', np.int32, (2,))])

_serials = itertools.count(1)


class _Parameters:
    """Launch parameters as float32 values in the subclass's `__slots__`, checked (a number, finite, then the subclass's
    `_rule`) and immutable; equal and hashed by value."""
    __slots__ = ()

    def __init__(self, **values):
        cls = type(self).__name__
        for name, given in values.items():
            try:
                with np.errstate(over='ignore'):
                    v = float(np.float32(given))                    # what the launch receives (too large: inf, refused below)
            except (TypeError, ValueError):
                raise ValueError(f"{cls}: {name} must be a number (got {given!r})") from None
            if not math.isfinite(v):
                raise ValueError(f"{cls}: {name} must be finite (got {given!r})")
            rule = self._rule(name, v)
            if rule:
                raise ValueError(f"{cls}: {name} must be {rule} (got {given!r})")
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is immutable")

    def __delattr__(self, name):
        raise AttributeError(f"{type(self).__name__} is immutable")

    def astuple(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return type(other) is type(self) and self.astuple() == other.astuple()

    def __hash__(self):
        return hash(self.astuple())

    def __repr__(self):
        return f"{type(self).__name__}(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__) + ")"


class OneEuro(_Parameters):
    """The parameters of the One-Euro filter `PoseTracker(smooth=...)` runs on every tracked joint. Immutable.

    rate: frames per second of a stream (a frame a person is missing from still counts as 1 / rate seconds).
    min_cutoff: the low-pass cutoff in Hz at rest - lower is smoother and lags more. beta: how fast the cutoff rises with the
    estimated speed, Hz per (pixel / second) - higher follows fast motion more closely. d_cutoff: the cutoff of the speed
    estimate itself. min_keypoint_score: a sample whose score is below it (not >=) is returned raw and restarts the joint's
    filter."""
    __slots__ = ('rate', 'min_cutoff', 'beta', 'd_cutoff', 'min_keypoint_score')

    def __init__(self, rate=30.0, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, min_keypoint_score=0.0):
        super().__init__(rate=rate, min_cutoff=min_cutoff, beta=beta, d_cutoff=d_cutoff, min_keypoint_score=min_keypoint_score)

    @staticmethod
    def _rule(name, v):
        if name in ('rate', 'min_cutoff', 'd_cutoff') and not v > 0:
            return "> 0"
        if name == 'beta' and not v >= 0:
            return ">= 0"


class ConstantVelocity(_Parameters):
    """The parameters of the constant-velocity prediction `PoseTracker(motion=...)` matches against. Immutable.

    velocity_gain: the weight in 0..1 of a newly observed velocity (the step from a track's last observed pose to the detection
    it is matched with, per frame) against the velocity the track carried; a track's second observation sets its velocity
    outright. 0 keeps every velocity 0: the tracker then matches as one without motion=. damping: the factor in 0..1 a
    track's velocity is multiplied with in every frame it is not detected in; 1 lets it coast at full speed.
    The defaults are NOT tuned: there are no trained weights and no video in this repository to tune them on."""
    __slots__ = ('velocity_gain', 'damping')

    def __init__(self, velocity_gain=0.5, damping=1.0):
        super().__init__(velocity_gain=velocity_gain, damping=damping)

    @staticmethod
    def _rule(name, v):
        if not 0 <= v <= 1:
            return "in 0..1"


# the prev / next state pairs of a tracker: (prefix of the attributes `prev`, `next`, `state_bytes`, `stream_bytes`; the
# option that asks for the pair; the library's size function; the head and slot of one stream; the name in messages)
_STATES = (('', None, 'mpn_pose_track_state_bytes', _HEAD, _SLOT, 'mpn_pose_track'),
           ('smooth_', 'smooth', 'mpn_pose_smooth_state_bytes', _SMOOTH_HEAD, _SMOOTH_SLOT, 'mpn_pose_smooth'),
           ('motion_', 'motion', 'mpn_pose_track_motion_state_bytes', _MOTION_HEAD, _MOTION_SLOT, 'mpn_pose_track_motion'))


class PoseTracker:
    """The tracks of `streams` independent cameras, `max_tracks` slots each, on the device.

    A call over b images sees b / streams consecutive frames per stream: stream s owns images s*F .. s*F+F-1 in time order.
    similarity: 'oks' (float64 OKS with the track's last keypoints in the ground-truth role; needs a PRN) or 'iou' (float32
    IoU of the boxes). A pair matches at similarity >= match_threshold, the largest first; a track unmatched for more than
    max_misses frames in a row is dropped; an unmatched detection with score >= new_track_score starts a track in the lowest
    free slot, or is counted in `dropped` when there is none. Ids count from 1 per stream and are never reused.
    max_boxes: the detection slots per image of the records this tracker reads (the Detector's params['max_boxes']).
    smooth: None, or a OneEuro: every tracked person's keypoints are filtered on the device as well (`mpn_pose_smooth`), which
    adds 'keypoints_smoothed' and 'keypoint_velocities' to what `unpack` / `update` / the Detector return.
    motion: None, or a ConstantVelocity: the launch is `mpn_pose_track_motion` - a detection is compared with the pose its
    track is predicted to have in the frame (box and keypoints moved by the track's velocity times the frames since it was
    last detected), so that a person who was hidden for a few frames, or who moves by more than a box width per frame, keeps
    the id. What a matched track stores is still the detection itself. Adds the coasting tracks of every image - alive, not
    detected in it - at their predicted pose: 'coasting_ids' int32 [m], 'coasting_misses' int32 [m], 'coasting_boxes' f32 [m,4],
    'coasting_keypoints' f32 [m,17,2]. With motion=None nothing changes.
    assignment: 'greedy' (the largest similarity first, as above) or 'optimal': the frame's pairs at similarity >=
    match_threshold are matched so that the sum of their similarities, quantised to steps of 2^-20, is the largest any matching
    reaches (the Hungarian method on the device, `mpn_pose_track_optimal`): persons side by side or crossing keep their ids
    where taking the largest pair first would hand them on. Everything else - the state, the rows, the keys - is the same."""

    def __init__(self, streams=1, max_tracks=32, similarity='oks', match_threshold=0.3, max_misses=10, new_track_score=0.3,
                 max_boxes=25, device=None, smooth=None, motion=None, assignment='greedy'):
        if similarity not in SIMILARITIES:
            raise ValueError(f"similarity must be one of {sorted(SIMILARITIES)} (got {similarity!r})")
        if assignment not in ASSIGNMENTS:
            raise ValueError(f"assignment must be one of {sorted(ASSIGNMENTS)} (got {assignment!r})")
        self.assignment = assignment
        if smooth is not None and not isinstance(smooth, OneEuro):
            raise ValueError(f"smooth must be None or a tracking.OneEuro (got {smooth!r})")
        self.smooth = smooth
        if motion is not None and not isinstance(motion, ConstantVelocity):
            raise ValueError(f"motion must be None or a tracking.ConstantVelocity (got {motion!r})")
        self.motion = motion
        self.streams, self.max_tracks, self.max_boxes = int(streams), int(max_tracks), int(max_boxes)
        self.similarity, self.max_misses = similarity, int(max_misses)
        self.match_threshold, self.new_track_score = float(match_threshold), float(new_track_score)
        if self.streams < 1:
            raise ValueError(f"streams must be at least 1 (got {streams})")
        if not 1 <= self.max_tracks <= MAX_TRACKS:
            raise ValueError(f"max_tracks must be in 1..{MAX_TRACKS} (got {max_tracks}): one lane of a wave per slot")
        if not 1 <= self.max_boxes <= MAX_BOXES:
            raise ValueError(f"max_boxes must be in 1..{MAX_BOXES} (got {max_boxes})")
        if self.max_misses < 0:
            raise ValueError(f"max_misses must not be negative (got {max_misses})")
        import torch
        self.device = torch.device(device) if device is not None else _lib.current_device()
        for prefix, _, size, head, slot, name in self._states():
            state_bytes = getattr(_lib.lib(), size)(self.streams, self.max_tracks)
            stream_bytes = head.itemsize + self.max_tracks * slot.itemsize
            if state_bytes == 0 or state_bytes != self.streams * stream_bytes:
                raise _lib.MpnError(f"{name}: the state's layout is not the one this binding was written against")
            setattr(self, prefix + 'state_bytes', state_bytes)
            setattr(self, prefix + 'stream_bytes', stream_bytes)
            for which in ('prev', 'next'):
                setattr(self, prefix + which, torch.zeros(state_bytes, dtype=torch.uint8, device=self.device))
        self.serial = next(_serials)                                # process-unique: part of the key of a Detector's graph
        self._update = {}                                           # update(): device record and rows per batch size

    def _states(self):
        """The rows of _STATES this tracker keeps: the track state, with smooth= the filters', with motion= the velocities'."""
        return [s for s in _STATES if s[1] is None or getattr(self, s[1]) is not None]

    def _pairs(self, stream=None):
        """(row of _STATES, prev, next) of every state this tracker keeps: whole, or cut to the bytes of one stream."""
        if stream is not None and not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream must be in 0..{self.streams - 1} (got {stream})")
        res = []
        for state in self._states():
            prev, nxt = getattr(self, state[0] + 'prev'), getattr(self, state[0] + 'next')
            if stream is not None:
                n = getattr(self, state[0] + 'stream_bytes')
                part = slice(int(stream) * n, int(stream) * n + n)
                prev, nxt = prev[part], nxt[part]
            res.append((state, prev, nxt))
        return res

    def check_batch(self, b):
        """The number of images of a call -> frames per stream."""
        if b < 1 or b % self.streams != 0:
            raise ValueError(f"track=: {b} images are not a whole number of frames for each of {self.streams} streams")
        return b // self.streams

    def row_offsets(self, b):
        """The layout of a call's rows for b images -> (n, at, end): mpn_pose_track's rows in [0, n), with smooth= the
        smoothed rows behind them, with motion= the coasting rows in [at, end), behind those at the next multiple of 8 bytes
        (at = end = where the rows end without motion=). Every size is the library's, checked against this binding's rows."""
        self.check_batch(b)

        def rows(size, per_image, row, what):
            n = getattr(_lib.lib(), size)(b, per_image)
            if n == 0 or n != b * per_image * row.itemsize:
                raise ValueError(f"{what} are more than one launch takes")
            return n
        n = at = rows('mpn_pose_track_out_bytes', self.max_boxes, _OUT, f"mpn_pose_track: {b} x {self.max_boxes} slots")
        if self.smooth is not None:
            at += rows('mpn_pose_smooth_out_bytes', self.max_boxes, _SMOOTH_OUT, f"mpn_pose_smooth: {b} x {self.max_boxes} slots")
        if self.motion is None:
            return n, at, at
        at = (at + 7) // 8 * 8
        return n, at, at + rows('mpn_pose_track_coast_bytes', self.max_tracks, _COAST,
                                f"mpn_pose_track_motion: {b} x {self.max_tracks} coasting rows")

    def track_bytes(self, b):
        """The bytes of mpn_pose_track's rows for b images."""
        return self.row_offsets(b)[0]

    def coast_offset(self, b):
        """Where the coasting rows of a motion= tracker begin within a call's rows: behind the track rows and any smoothed
        rows, at the next multiple of 8 bytes."""
        return self.row_offsets(b)[1]

    def out_bytes(self, b):
        """The bytes of a call's rows for b images: the track rows, with smooth= the smoothed rows behind them, and with
        motion= the coasting rows behind those."""
        return self.row_offsets(b)[2]

    def launch(self, record, out, b, coast=None):
        """record: the uint8 device tensor mpn_pose_gather wrote for (b, max_boxes); out: uint8 device tensor of
        `track_bytes(b)`. Reads `prev`, writes `next` and out; the state does not advance before `commit()`. A motion= tracker
        also reads `motion_prev` and writes `motion_next` and the coasting rows: to `coast`, or, without it, into `out` at
        `coast_offset(b)` (out is then a call's whole `out_bytes(b)`)."""
        self.check_batch(b)
        if self.motion is not None:
            _, at, end = self.row_offsets(b)
            if coast is None:
                coast = out[at:end]
            if coast.numel() < end - at:
                raise ValueError(f"launch: a motion= tracker writes {end - at} bytes of coasting "
                                 f"rows for {b} images (got room for {coast.numel()})")
            _lib.call("mpn_pose_track_motion", _lib.ptr(record), b, self.max_boxes, self.streams, self.max_tracks,
                      SIMILARITIES[self.similarity], int(self.assignment == 'optimal'), self.match_threshold, self.new_track_score,
                      self.max_misses, self.motion.velocity_gain, self.motion.damping, _lib.ptr(self.prev), _lib.ptr(self.next),
                      _lib.ptr(self.motion_prev), _lib.ptr(self.motion_next), _lib.ptr(out), _lib.ptr(coast), _lib.stream_ptr())
            return out
        _lib.call(ASSIGNMENTS[self.assignment], _lib.ptr(record), b, self.max_boxes, self.streams, self.max_tracks,
                  SIMILARITIES[self.similarity], self.match_threshold, self.new_track_score, self.max_misses,
                  _lib.ptr(self.prev), _lib.ptr(self.next), _lib.ptr(out), _lib.stream_ptr())
        return out

    def launch_smooth(self, record, track_out, out, b):
        """record and track_out: what `launch` read and wrote (uint8 device tensors); out: uint8 device tensor of
        `mpn_pose_smooth_out_bytes(b, max_boxes)`. Reads `smooth_prev`, writes `smooth_next` and out; `commit()` advances the state."""
        if self.smooth is None:
            raise ValueError("launch_smooth: this tracker was made without smooth=")
        self.check_batch(b)
        _lib.call("mpn_pose_smooth", _lib.ptr(record), _lib.ptr(track_out), b, self.max_boxes, self.streams, self.max_tracks,
                  *self.smooth.astuple(), _lib.ptr(self.smooth_prev), _lib.ptr(self.smooth_next), _lib.ptr(out),
                  _lib.stream_ptr())
        return out

    def launch_all(self, record, out, b):
        """`launch` and, with smooth=, `launch_smooth` behind it: out is a uint8 device tensor of `out_bytes(b)`, the track rows
        first (then the smoothed rows, then the coasting rows of motion=)."""
        n, at, _ = self.row_offsets(b)
        self.launch(record, out[:n], b, out[at:] if self.motion is not None else None)
        if self.smooth is not None:
            self.launch_smooth(record, out[:n], out[n:at], b)
        return out

    def commit(self):
        """The last launch's state becomes the current one: one small device copy on the current stream (one more with smooth=,
        one more with motion=)."""
        for _, prev, nxt in self._pairs():
            prev.copy_(nxt, non_blocking=True)

    def reset(self, stream=None):
        """Forget every track and start the ids at 1 again: of all streams, or of one."""
        for _, prev, nxt in self._pairs(stream):
            prev.zero_()
            nxt.zero_()

    def unpack(self, out, counts):
        """A host copy of the output rows (uint8 array) and the record's per-image counts -> a list of dicts, one per image:
        'track_ids' int32 [n] (0 = untracked), 'track_hits' int32 [n], 'track_new' bool [n], 'track_similarity' f64 [n],
        in the image's record order. With smooth= the smoothed rows lie behind the track rows and add 'keypoints_smoothed' f32
        [n,17,3] (x, y, score; raw for an untracked person, a joint's first sample and a sample below min_keypoint_score) and
        'keypoint_velocities' f32 [n,17,2] (pixels per second; 0 there). With motion= the coasting rows lie behind those and add
        'coasting_ids' int32 [m], 'coasting_misses' int32 [m] (frames in a row without a detection, this one included),
        'coasting_boxes' f32 [m,4] and 'coasting_keypoints' f32 [m,17,2]: the image's tracks that are alive and were not detected
        in it, in slot order, at the pose predicted for this frame."""
        n, at, end = self.row_offsets(len(counts))
        rows = np.frombuffer(out, np.uint8, n).view(_OUT)
        smooth = None
        if self.smooth is not None:
            smooth = np.frombuffer(out, np.uint8, len(rows) * _SMOOTH_OUT.itemsize, n).view(_SMOOTH_OUT)
        coast = None
        if self.motion is not None:
            coast = np.frombuffer(out, np.uint8, end - at, at).view(_COAST).reshape(len(counts), self.max_tracks)
        res, s = [], 0
        for i, n in enumerate(counts):
            r = rows[s:s + int(n)]
            res.append({'track_ids': r['track_id'].copy(), 'track_hits': r['hits'].copy(),
                        'track_new': (r['flags'] & FLAG_NEW) != 0, 'track_similarity': r['similarity'].copy()})
            if smooth is not None:
                res[-1]['keypoints_smoothed'] = smooth['keypoints'][s:s + int(n)].copy()
                res[-1]['keypoint_velocities'] = smooth['velocities'][s:s + int(n)].copy()
            if coast is not None:
                c = coast[i][coast[i]['id'] != 0]
                res[-1].update({'coasting_ids': c['id'].copy(), 'coasting_misses': c['misses'].copy(),
                                'coasting_boxes': c['box'].copy(), 'coasting_keypoints': c['keypoints'].copy()})
            s += int(n)
        return res

    def tracks(self, stream=0):
        """A host copy of one stream's current state: {'next_id', 'dropped', 'slots' int [m] (the live slots), 'ids', 'hits',
        'age', 'misses' int32 [m], 'boxes' f32 [m,4], 'scores' f32 [m], 'keypoints' f32 [m,17,3]}. With smooth= also 'frames'
        (the frames the stream's filters have seen), 'keypoints_smoothed' f32 [m,17,2] (x_hat, y_hat of the live slots; of a
        slot whose track was not detected since the slot changed hands, the earlier track's) and 'keypoint_last' int32 [m,17]
        (the frame number of each joint's last sample, 0 = none). With motion= also 'velocities' f32 [m,6] (per frame: of the
        box's ymin, xmin, ymax, xmax, normalised, and of the keypoint centroid's x, y in pixels), 'seen' int32 [m] (the matches
        a track's velocity has taken in) and 'boxes_predicted' f32 [m,4], 'keypoints_predicted' f32 [m,17,2]: where the next
        frame's detections are compared with, computed here from the copied state in the kernel's float32 steps."""
        host = {}                                                   # per pair: the stream's head and its slots
        for (prefix, _, _, head, slot, _), prev, _ in self._pairs(stream):
            raw = prev.cpu().numpy()
            host[prefix] = raw[:head.itemsize].view(head)[0], raw[head.itemsize:].view(slot)
        head, slots = host['']
        live = np.nonzero(slots['id'] != 0)[0]
        s = slots[live]
        res = {'next_id': max(int(head['next_id']), 1), 'dropped': int(head['dropped']), 'slots': live,
               'ids': s['id'].copy(), 'hits': s['hits'].copy(), 'age': s['age'].copy(), 'misses': s['misses'].copy(),
               'boxes': s['box'].copy(), 'scores': s['score'].copy(), 'keypoints': s['keypoints'].copy()}
        if self.smooth is not None:
            joints = host['smooth_'][1]['joints'][live]
            res['frames'] = int(host['smooth_'][0]['frames'])
            res['keypoints_smoothed'] = joints['hat'][..., :2].copy()
            res['keypoint_last'] = joints['last'].copy()
        if self.motion is not None:
            m = host['motion_'][1][live]
            own = (m['id'] == s['id'])[:, None]                     # (as the launch reads a slot another track left)
            vel = np.where(own, m['vel'], np.float32(0)).astype(np.float32)
            gap = (s['misses'] + 1).astype(np.float32)[:, None]
            res['velocities'] = vel
            res['seen'] = np.where(own[:, 0], m['seen'], 0).astype(np.int32)
            res['boxes_predicted'] = s['box'] + vel[:, :4] * gap
            res['keypoints_predicted'] = s['keypoints'][:, :, :2] + (vel[:, 4:] * gap)[:, None, :]
        return res

    def update(self, outputs):
        """The same launch for host arrays: b result dicts ('boxes', 'scores', 'keypoints' as `Detector.predict_*` returns
        them; at most max_boxes persons each) are packed into a record, uploaded, tracked and committed. Returns what
        `unpack` returns."""
        import torch
        outputs = list(outputs)
        b = len(outputs)
        nbytes = self.out_bytes(b)
        record, counts = fill_record(outputs, b, self.max_boxes)
        with torch.cuda.device(self.device):
            if b not in self._update:
                self._update[b] = (torch.zeros(len(record), dtype=torch.uint8, device=self.device),
                                   torch.zeros(nbytes, dtype=torch.uint8, device=self.device))
            dev_record, dev_out = self._update[b]
            dev_record.copy_(torch.from_numpy(record))
            self.launch_all(dev_record, dev_out, b)
            self.commit()
            out = dev_out.cpu().numpy()
        return self.unpack(out, counts)
