"""Motion trails for the persons `Detector.predict_*(track=...)` returns: where each identity has been, as a polyline of its
last `length` anchors, newest first - in every result dict and, with `annotate`, drawn into the frame.

The history - an anchor per person (the feet, or the box, `ZoneCounter`'s rule), a ring of anchors per identity - lives on
the device (`mpn_track_trails`, include/mpn.h): inside the Detector's captured graph behind the tracker's launches when
`predict_*` is given `trails=`, or through `TrackTrails.update` for host dicts that carry 'track_ids' from any tracker. The
picture (`mpn_draw_trails`) blends the polylines over the annotated RGBA frames in place, before they are encoded.

    tracker = PoseTracker(streams=1)
    trails = TrackTrails(streams=1, frame_size=(720, 1280), length=32)
    for frames in batches:
        for person in detector.predict_images(frames, track=tracker, trails=trails, annotate='jpeg'):
            person['trails']['points'], person['trails']['count'], person['annotated_jpeg']

Like the tracker's, the launch is a PURE function of its inputs and the previous state; `commit()` advances the state (the
Detector does that once per call). Only persons the tracker gave an id have a history: coasting tracks are not rows of the
record and add no points, and a person whose identity switches starts a new trail. Trails are one pixel wide."""
import itertools
import math

import numpy as np

from . import _lib
from .pose_metrics import fill_record
from .stream_state import StreamState, flag, integer
from .zones import ANCHORS, MAX_BOXES, SLOTS, track_rows_of

MAX_LENGTH, MAX_EVERY, MAX_GAP = 64, 255, 65535
FLAG_TRACKED, FLAG_ANKLES, FLAG_NO_ANCHOR, FLAG_APPENDED, FLAG_RESTARTED = 1, 2, 4, 8, 16
TABLE_HEADER_WORDS, TABLE_FADE = 4, 1
DESC_WORDS = 8                          # mpn_draw_desc in 32-bit words


def slot_dtype(length):
    """A slot of the state (include/mpn.h) for trails of `length` points."""
    return np.dtype([('id', np.int32), ('last', np.int32), ('last_append', np.int32), ('count', np.int32), ('head', np.int32),
                     ('pad', np.int32, (3,)), ('ring', np.float32, (length, 2))])


def state_dtype(length):
    """The state of one stream."""
    return np.dtype([('frames', np.int32), ('pad', np.int32, (3,)), ('slots', slot_dtype(length), (SLOTS,))])


def row_dtype(length):
    """A row of mpn_track_trails' out."""
    return np.dtype([('n', np.int32), ('flags', np.uint32), ('points', np.float32, (length + 1, 2))])


def draw_table(palette, fade, min_alpha, length):
    """The table of mpn_draw_trails as a uint8 array: flags, min_alpha, K, P, the palette (R | G<<8 | B<<16 per word)."""
    size = _lib.lib().mpn_draw_trails_tables_bytes(len(palette))
    if size == 0:
        raise ValueError(f"TrackTrails: palette must hold 1..256 colours (got {len(palette)})")
    table = np.zeros(size, np.uint8)
    words = table[:(TABLE_HEADER_WORDS + len(palette)) * 4].view(np.int32)
    words[:TABLE_HEADER_WORDS] = (TABLE_FADE if fade else 0, min_alpha, length, len(palette))
    words[TABLE_HEADER_WORDS:] = [c[0] | c[1] << 8 | c[2] << 16 for c in palette]
    return table


def rows_of(outputs, b, max_boxes, length):
    """The 'trails' of b result dicts -> rows of mpn_track_trails' out for the record `fill_record` packs of them (uint8)."""
    rows = np.zeros(b * max_boxes, row_dtype(length))
    at = 0
    for i, o in enumerate(outputs):
        t = o.get('trails')
        if t is None or 'track_ids' not in o:
            raise ValueError("draw_trails: the output dict needs 'trails' and 'track_ids'")
        n = len(t['count'])
        points = np.asarray(t['points'], np.float32)
        if points.shape != (n, length + 1, 2) or n != len(o['track_ids']) or n > max_boxes:
            raise ValueError(f"draw_trails: image {i} has 'points' of shape {points.shape} for {len(o['track_ids'])} persons; "
                             f"trails of length {length} have [n, {length + 1}, 2], n <= {max_boxes}")
        r = rows[at:at + n]
        r['n'], r['points'] = t['count'], points
        r['flags'] = np.where(np.asarray(t['tracked'], bool), FLAG_TRACKED, 0)
        at += n
    return rows.view(np.uint8)


class TrackTrails(StreamState):
    """The last `length` anchors of every tracked identity, for `streams` independent cameras, on the device
    (`mpn_track_trails`), and how `annotate` draws them (`mpn_draw_trails`).

    frame_size: (height, width) of the frames in source pixels, the unit of every point. length: the points a trail keeps
    (1..64). every: a point is kept once per `every` frames (1..255); between them the trail ends at the person's current
    anchor. max_gap: an identity that was not observed for more than max_gap frames starts a new trail (0: never; up to
    65535). anchor, min_keypoint_score: the point that stands for a person, as for `zones.ZoneCounter`: 'feet' (the mean of the
    ankles whose score is >= min_keypoint_score, else 'box_bottom'), 'box_bottom' or 'box_centre'. max_boxes: the detection
    slots per image of the records (the Detector's params['max_boxes']).
    draw: with `annotate`, the trails are drawn into the frame. palette: None (`draw.DEFAULT_PALETTE`, the colours of
    `TrackStyle`) or 1..256 (r, g, b): a trail has palette[(track_id - 1) % len(palette)]. fade: the newest segment is opaque
    and segment s from the newest has alpha 255 - s * (255 - min_alpha) // max(length - 1, 1); False: every segment is opaque.

    A call over b images sees b / streams consecutive frames per stream, stream s owning images s*F .. s*F+F-1 in time order,
    as `tracking.PoseTracker` does. The object owns the drawing's table on the device and the state - per stream 64 identities
    with their rings - as a prev / next pair. `launch` is pure; `commit()` advances the state. No default is tuned on video."""
    keyword, _serials = 'trails', itertools.count(1)

    def __init__(self, streams=1, frame_size=None, length=32, every=1, max_gap=30, anchor='feet', min_keypoint_score=0.0,
                 draw=True, fade=True, min_alpha=64, palette=None, max_boxes=25, device=None):
        from .inference.draw import DEFAULT_PALETTE, MAX_PALETTE, _colour
        if isinstance(streams, (bool, np.bool_)) or not isinstance(streams, (int, np.integer)) or streams < 1:
            raise ValueError(f"TrackTrails: streams must be an integer >= 1 (got {streams!r})")
        self.max_boxes = integer('TrackTrails', 'max_boxes', max_boxes, 1, MAX_BOXES)
        try:
            height, width = (float(v) for v in frame_size)
        except (TypeError, ValueError):
            raise ValueError(f"TrackTrails: frame_size must be (height, width) (got {frame_size!r})") from None
        if not (math.isfinite(height) and math.isfinite(width) and height > 0 and width > 0):
            raise ValueError(f"TrackTrails: frame_size must be two positive numbers (height, width) (got {frame_size!r})")
        self.length = integer('TrackTrails', 'length', length, 1, MAX_LENGTH)
        self.every = integer('TrackTrails', 'every', every, 1, MAX_EVERY)
        self.max_gap = integer('TrackTrails', 'max_gap', max_gap, 0, MAX_GAP)
        if not isinstance(anchor, str) or anchor not in ANCHORS:
            raise ValueError(f"TrackTrails: anchor must be one of {list(ANCHORS)} (got {anchor!r})")
        try:
            mks = float(min_keypoint_score)
        except (TypeError, ValueError):
            raise ValueError(f"TrackTrails: min_keypoint_score must be a number (got {min_keypoint_score!r})") from None
        if not math.isfinite(mks):
            raise ValueError(f"TrackTrails: min_keypoint_score must be finite (got {min_keypoint_score!r})")
        self.draw, self.fade = flag('TrackTrails', 'draw', draw), flag('TrackTrails', 'fade', fade)
        self.min_alpha = integer('TrackTrails', 'min_alpha', min_alpha, 0, 255)
        if palette is None:
            palette = DEFAULT_PALETTE
        try:
            palette = tuple(palette)
        except TypeError:
            raise ValueError(f"TrackTrails: palette must be a sequence of (r, g, b) (got {palette!r})") from None
        if not 1 <= len(palette) <= MAX_PALETTE:
            raise ValueError(f"TrackTrails: palette must hold 1..{MAX_PALETTE} colours (got {len(palette)})")
        try:
            self.palette = tuple(_colour(f"palette[{i}]", c) for i, c in enumerate(palette))
        except ValueError as e:
            raise ValueError(str(e).replace("TrackStyle:", "TrackTrails:")) from None
        self.streams, self.frame_size = int(streams), (height, width)
        self.anchor, self.min_keypoint_score = anchor, mks
        self.row, self.state_row = row_dtype(self.length), state_dtype(self.length)
        lib = _lib.lib()
        self.state_bytes = lib.mpn_track_trails_state_bytes(self.streams, self.length)
        if self.state_bytes != self.streams * self.state_row.itemsize:
            raise ValueError(f"TrackTrails: streams = {streams!r} are more than mpn_track_trails takes")
        self.host_table = draw_table(self.palette, self.fade, self.min_alpha, self.length)
        import torch
        self.device = torch.device(device) if device is not None else _lib.current_device()
        self.table = torch.from_numpy(self.host_table.copy()).to(self.device)
        self._make_state(self.state_row.itemsize)
        self._update, self._work = {}, {}
        self.last_out = None

    # ---------------------------------------------------------------- the device side
    def check_frame_sizes(self, sizes):
        """Raises unless every (height, width) of `sizes` is the object's frame_size."""
        for h, w in sizes:
            if (float(h), float(w)) != self.frame_size:
                raise ValueError(f"trails=: the trails are in the pixels of {self.frame_size[0]:g} x {self.frame_size[1]:g} "
                                 f"frames (height x width), this call has a frame of {h} x {w}")

    def out_bytes(self, b):
        """The bytes of a call's rows for b images."""
        self.check_batch(b)
        n = _lib.lib().mpn_track_trails_out_bytes(b, self.max_boxes, self.length)
        if n == 0 or n != b * self.max_boxes * self.row.itemsize:
            raise ValueError(f"mpn_track_trails: {b} x {self.max_boxes} slots are more than one launch takes")
        return n

    def launch(self, record, track_rows, out, b, keypoints=True):
        """record: the uint8 device tensor the tracker read; track_rows: the uint8 device tensor of mpn_pose_track's rows for it;
        out: uint8 device tensor of `out_bytes(b)`. keypoints=False (a record without keypoints, whose zeros would pass for
        ankles): 'feet' reads as 'box_bottom'. Reads `prev`, writes `next` and out; `commit()` advances the state."""
        self.check_batch(b)
        _lib.call("mpn_track_trails", _lib.ptr(record), _lib.ptr(track_rows), b, self.max_boxes, self.streams, self.length,
                  self.every, self.max_gap, ANCHORS[self.anchor], self.min_keypoint_score, self.frame_size[0], self.frame_size[1],
                  int(bool(keypoints)), _lib.ptr(self.prev), _lib.ptr(self.next), _lib.ptr(out), _lib.stream_ptr())
        return out

    def launch_draw(self, descs, record, track_rows, trail_rows, out_rgba, b):
        """mpn_draw_trails over the RGBA frames `out_rgba` (flat uint8 device tensor) that mpn_draw_detections / mpn_draw_tracks
        wrote for the descriptors `descs`: the rows `launch` wrote, as polylines, IN PLACE. The workspace of a batch size is
        made on its first use (before a capture: the Detector's warm-up run)."""
        import torch
        if b not in self._work:
            need = _lib.lib().mpn_draw_trails_workspace_bytes(b, self.max_boxes, self.length)
            if need == 0:
                raise ValueError(f"mpn_draw_trails: {b} x {self.max_boxes} slots are more than one launch takes")
            self._work[b] = torch.empty(need, dtype=torch.uint8, device=self.device)
        work = self._work[b]
        _lib.call("mpn_draw_trails", _lib.ptr(descs), _lib.ptr(record), record.numel(), _lib.ptr(track_rows), _lib.ptr(trail_rows),
                  _lib.ptr(self.table), self.table.numel(), b, self.max_boxes, self.length, _lib.ptr(out_rgba), out_rgba.numel(),
                  _lib.ptr(work), work.numel(), _lib.stream_ptr())
        return out_rgba

    def state(self, stream=0):
        """A host copy of one stream's current state, as a `state_dtype(length)` record."""
        return self._raw_state(stream).view(self.state_row)[0]

    def unpack(self, out, counts):
        """A host copy of the output rows (uint8 array) and the record's per-image counts -> a list of b dicts. With n persons
        in the image's record order: 'points' f32 [n, length + 1, 2] as (x, y), newest first, zero behind 'count'; 'count' int32
        [n]; 'tracked' (the person has a history here), 'appended' (this frame's anchor was kept), 'restarted' (the trail began
        anew after a gap), 'anchor_from_keypoints' bool [n]."""
        b = len(counts)
        rows = np.frombuffer(out, np.uint8, b * self.max_boxes * self.row.itemsize).view(self.row)
        res, s = [], 0
        for i in range(b):
            n = int(counts[i])
            r = rows[s:s + n]
            res.append({'points': r['points'].copy(), 'count': r['n'].copy(), 'tracked': (r['flags'] & FLAG_TRACKED) != 0,
                        'appended': (r['flags'] & FLAG_APPENDED) != 0, 'restarted': (r['flags'] & FLAG_RESTARTED) != 0,
                        'anchor_from_keypoints': (r['flags'] & FLAG_ANKLES) != 0})
            s += n
        return res

    def update(self, outputs):
        """The same launch for host arrays: b result dicts that carry 'boxes', 'scores', 'track_ids' and, optionally,
        'keypoints' (as `Detector.predict_*(track=...)` returns them, or with the ids of any other tracker; at most max_boxes
        persons each) are packed, uploaded, run and committed. Dicts without 'keypoints' take the box fallback. Returns what
        `unpack` returns."""
        import torch
        outputs = list(outputs)
        b = len(outputs)
        nbytes = self.out_bytes(b)
        rows = track_rows_of(outputs, b, self.max_boxes)
        record, counts = fill_record(outputs, b, self.max_boxes)
        keypoints = all('keypoints' in o and len(o['keypoints']) == len(o['scores']) for o in outputs)
        with torch.cuda.device(self.device):
            if b not in self._update:
                self._update[b] = (torch.zeros(len(record), dtype=torch.uint8, device=self.device),
                                   torch.zeros(len(rows), dtype=torch.uint8, device=self.device),
                                   torch.zeros(nbytes, dtype=torch.uint8, device=self.device))
            dev_record, dev_rows, dev_out = self._update[b]
            dev_record.copy_(torch.from_numpy(record))
            dev_rows.copy_(torch.from_numpy(rows))
            self.launch(dev_record, dev_rows, dev_out, b, keypoints)
            self.commit()
            out = dev_out.cpu().numpy()
        self.last_out = out                                         # the call's raw rows (include/mpn.h)
        return self.unpack(out, counts)

    def draw_frame(self, image, output):
        """`inference.draw_trails`: one host frame, uint8 [h, w, 3] or [h, w, 4], and its result dict -> uint8 [h, w, 4]."""
        import torch
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] not in (3, 4) or image.shape[0] < 1 or image.shape[1] < 1:
            raise ValueError(f"draw_trails: image must be uint8 [h, w, 3] or [h, w, 4] (got {image.dtype} {image.shape})")
        h, w = image.shape[:2]
        rgba = np.full((h, w, 4), 255, np.uint8)
        rgba[..., :image.shape[2]] = image
        if not isinstance(output, dict) or 'trails' not in output or 'track_ids' not in output:
            raise ValueError("draw_trails: the output dict needs 'trails' and 'track_ids'")
        placeholder = {'scores': np.zeros(len(output['track_ids']), np.float32), 'track_ids': output['track_ids'],
                       'trails': output['trails']}                  # (the drawing reads the record's counts alone)
        trail_rows = rows_of([placeholder], 1, self.max_boxes, self.length)
        track_rows = track_rows_of([placeholder], 1, self.max_boxes)
        record, _ = fill_record([placeholder], 1, self.max_boxes)
        desc = np.zeros((1, DESC_WORDS), np.int32)
        desc[0, 4:6] = (h, w)
        nbytes = (h * w * 4 + 15) // 16 * 16
        with torch.cuda.device(self.device):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)        # noqa: E731
            frame = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
            frame[:h * w * 4].copy_(up(rgba.reshape(-1)))
            self.launch_draw(up(desc), up(record), up(track_rows), up(trail_rows), frame, 1)
            return frame[:h * w * 4].cpu().numpy().reshape(h, w, 4)


def draw_trails(image, outputs, trails):
    """The one-frame drawing call: a host RGB or RGBA frame (uint8 [h, w, 3] or [h, w, 4]) and the result dict of that frame,
    which carries 'trails' and 'track_ids' (as `Detector.predict_*(trails=...)` or `TrackTrails.update` return them) -> the
    frame as uint8 [h, w, 4] with the trails drawn by `mpn_draw_trails`, as `annotate` draws them. trails: the TrackTrails,
    whose palette, fade, min_alpha and length say how."""
    if not isinstance(trails, TrackTrails):
        raise ValueError("draw_trails: trails must be a trails.TrackTrails")
    return trails.draw_frame(image, outputs)
