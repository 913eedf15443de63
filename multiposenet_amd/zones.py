"""Zones and counting lines for the persons `Detector.predict_*(track=...)` returns: how many stand in an area, who entered and
who left, how long each stayed, and how many crossed a line in each direction.

The per-frame work - an anchor per person (the feet, or the box), a crossing-number test per polygon, a debounced membership
per identity and a segment test per line - runs on the device (`mpn_zone_events`, include/mpn.h): inside the Detector's
captured graph behind the tracker's launches when `predict_*` is given `zones=`, or through `ZoneCounter.update` for host dicts
that carry 'track_ids' from any tracker.

    tracker = PoseTracker(streams=1)
    counter = ZoneCounter(streams=1, frame_size=(720, 1280), zones={'door': [(0, 0), (400, 0), (400, 720), (0, 720)]},
                          lines={'gate': ((640, 0), (640, 720))})
    for frames in batches:
        for person in detector.predict_images(frames, track=tracker, zones=counter):
            person['zones']['occupancy'], person['zones']['inside'], person['zones']['line_positive']
    counter.totals()                                        # {'frames', 'entries': {'door': ...}, 'line_positive': {'gate': ...}, ...}

Like the tracker's, the launch is a PURE function of its inputs and the previous state; `commit()` advances the state (the
Detector does that once per call). Only persons the tracker gave an id are counted as identities: persons below the
Detector's score_threshold are not in the record at all, coasting tracks are not rows of it, and a track that dies inside a
zone leaves no exit event. Line crossings are not debounced: a person who wavers on a line crosses it many times, in both
directions, and `positive - negative` is the number to use."""
import itertools
import math

import numpy as np

from . import _lib
from .stream_state import StreamState
from .tracking import fill_record

MAX_ZONES = MAX_LINES = MAX_VERTICES = 16
MAX_BOXES = 64
SLOTS = 64
ANCHORS = {'feet': 0, 'box_bottom': 1, 'box_centre': 2}
FLAG_TRACKED, FLAG_ANKLES, FLAG_NO_ANCHOR = 1, 2, 4

# the table, the state of one stream and the rows of mpn_zone_events' out (include/mpn.h)
TABLE = np.dtype([('num_zones', np.int32), ('num_lines', np.int32), ('min_frames', np.int32), ('anchor', np.int32),
                  ('height', np.float64), ('width', np.float64), ('min_keypoint_score', np.float64),
                  ('vertex_count', np.int32, (MAX_ZONES,)), ('vertices', np.float64, (MAX_ZONES, MAX_VERTICES, 2)),
                  ('lines', np.float64, (MAX_LINES, 2, 2))])
SLOT = np.dtype([('id', np.int32), ('inside', np.uint32), ('last', np.int32), ('pad', np.int32), ('anchor', np.float64, (2,)),
                 ('entered_frame', np.int32, (MAX_ZONES,)), ('run', np.uint8, (MAX_ZONES,))])
STATE = np.dtype([('frames', np.int32), ('pad', np.int32, (3,)), ('zone_entries', np.uint32, (MAX_ZONES,)),
                  ('zone_exits', np.uint32, (MAX_ZONES,)), ('line_positive', np.uint32, (MAX_LINES,)),
                  ('line_negative', np.uint32, (MAX_LINES,)), ('slots', SLOT, (SLOTS,))])
PERSON = np.dtype([('inside', np.uint32), ('entered', np.uint32), ('exited', np.uint32), ('crossed_positive', np.uint32),
                   ('crossed_negative', np.uint32), ('flags', np.uint32), ('anchor', np.float64, (2,)),
                   ('dwell', np.int32, (MAX_ZONES,))])
IMAGE = np.dtype([(k, np.uint32, (16,)) for k in ('occupancy', 'entries', 'exits', 'positive', 'negative', 'total_entries',
                                                  'total_exits', 'total_positive', 'total_negative')])
_TRACK_ROW = np.dtype([('track_id', np.int32), ('slot', np.int32), ('hits', np.int32), ('flags', np.int32),
                       ('similarity', np.float64)])


def _named(what, given, most):
    """zones= / lines= as a dict or a list -> [(name, value)], at most `most`."""
    if given is None:
        return []
    items = list(given.items()) if isinstance(given, dict) else [(str(i), v) for i, v in enumerate(given)]
    if len(items) > most:
        raise ValueError(f"ZoneCounter: {what} must hold at most {most} entries (got {len(items)})")
    return [(str(k), v) for k, v in items]


def _points(what, name, value, lo, hi):
    """A sequence of lo..hi finite (x, y) pairs -> f64 [n, 2]."""
    try:
        pts = np.asarray(value, np.float64)
    except (TypeError, ValueError):
        pts = None
    if pts is None or pts.ndim != 2 or pts.shape[1] != 2 or not lo <= len(pts) <= hi:
        many = f"{lo}..{hi}" if lo != hi else str(lo)
        raise ValueError(f"ZoneCounter: {what} {name!r} must be {many} (x, y) points (got {value!r})")
    if not np.isfinite(pts).all():
        raise ValueError(f"ZoneCounter: {what} {name!r} must have finite coordinates (got {value!r})")
    return pts


def build_table(frame_size, zones=None, lines=None, anchor='feet', min_frames=1, min_keypoint_score=0.0):
    """The checked arguments of a ZoneCounter -> (the table as a TABLE record array of one element, zone names, line names).
    Raises ValueError for everything the kernel would only clamp."""
    try:
        height, width = (float(v) for v in frame_size)
    except (TypeError, ValueError):
        raise ValueError(f"ZoneCounter: frame_size must be (height, width) (got {frame_size!r})") from None
    if not (math.isfinite(height) and math.isfinite(width) and height > 0 and width > 0):
        raise ValueError(f"ZoneCounter: frame_size must be two positive numbers (height, width) (got {frame_size!r})")
    zones, lines = _named('zones', zones, MAX_ZONES), _named('lines', lines, MAX_LINES)
    if not zones and not lines:
        raise ValueError("ZoneCounter: zones or lines must be given (got neither)")
    if not isinstance(anchor, str) or anchor not in ANCHORS:
        raise ValueError(f"ZoneCounter: anchor must be one of {list(ANCHORS)} (got {anchor!r})")
    if isinstance(min_frames, (bool, np.bool_)) or not isinstance(min_frames, (int, np.integer)) or not 1 <= min_frames <= 255:
        raise ValueError(f"ZoneCounter: min_frames must be an integer in 1..255 (got {min_frames!r})")
    try:
        mks = float(min_keypoint_score)
    except (TypeError, ValueError):
        raise ValueError(f"ZoneCounter: min_keypoint_score must be a number (got {min_keypoint_score!r})") from None
    if not math.isfinite(mks):
        raise ValueError(f"ZoneCounter: min_keypoint_score must be finite (got {min_keypoint_score!r})")
    table = np.zeros(1, TABLE)
    t = table[0]
    t['num_zones'], t['num_lines'], t['min_frames'], t['anchor'] = len(zones), len(lines), int(min_frames), ANCHORS[anchor]
    t['height'], t['width'], t['min_keypoint_score'] = height, width, mks
    t['vertex_count'][:] = 3                                        # (of the zones that are not there: in range all the same)
    for z, (name, polygon) in enumerate(zones):
        pts = _points('zone', name, polygon, 3, MAX_VERTICES)
        t['vertex_count'][z] = len(pts)
        t['vertices'][z, :len(pts)] = pts
    for l, (name, pq) in enumerate(lines):
        pts = _points('line', name, pq, 2, 2)
        if (pts[0] == pts[1]).all():
            raise ValueError(f"ZoneCounter: line {name!r} must have two different end points (got {pq!r})")
        t['lines'][l] = pts
    return table, [k for k, _ in zones], [k for k, _ in lines]


def track_rows_of(outputs, b, max_boxes):
    """The 'track_ids' of b result dicts -> rows of mpn_pose_track's out for the record `fill_record` packs of them (uint8):
    the ids where the record's rows are, slot -1 (this stage never reads it)."""
    rows = np.zeros(b * max_boxes, _TRACK_ROW)
    rows['slot'] = -1
    at = 0
    for i, o in enumerate(outputs):
        if 'track_ids' not in o:
            raise ValueError("ZoneCounter: every output dict needs 'track_ids' (a tracker's identities)")
        ids = np.asarray(o['track_ids'], np.int32).reshape(-1)
        if len(ids) != len(o['scores']):
            raise ValueError(f"ZoneCounter: image {i} has {len(o['scores'])} persons and {len(ids)} track_ids")
        rows['track_id'][at:at + len(ids)] = ids
        at += len(ids)
    return rows.view(np.uint8)


class ZoneCounter(StreamState):
    """Occupancy, entries, exits and dwell times of up to 16 polygons and signed crossings of up to 16 lines, for `streams`
    independent cameras that share one geometry, on the device (`mpn_zone_events`).

    frame_size: (height, width) of the frames in source pixels, the unit of every coordinate here. zones: a dict or list of
    polygons, each 3..16 (x, y) points; lines: a dict or list of ((x, y), (x, y)) pairs P, Q - a movement that ends on the
    side of the line where (Q - P) x (C - P) > 0 is a positive crossing. anchor: the point that stands for a person: 'feet'
    (the mean of the ankles whose score is >= min_keypoint_score, else 'box_bottom'), 'box_bottom' (the middle of the box's
    lower side) or 'box_centre'.
    min_frames: a person enters or leaves a zone after this many consecutive observed frames on the other side of its boundary
    (1: at once). max_boxes: the detection slots per image of the records (the Detector's params['max_boxes']).

    A call over b images sees b / streams consecutive frames per stream, stream s owning images s*F .. s*F+F-1 in time order,
    as `tracking.PoseTracker` does. The counter owns the table on the device and the state - per stream the cumulative
    counters and 64 identities with their membership, last anchor and dwell - as a prev / next pair. `launch` is pure;
    `commit()` advances the state. No default is tuned on video."""
    keyword, _serials = 'zones', itertools.count(1)

    def __init__(self, streams=1, frame_size=None, zones=None, lines=None, anchor='feet', min_frames=1, min_keypoint_score=0.0,
                 max_boxes=25, device=None):
        if isinstance(streams, (bool, np.bool_)) or not isinstance(streams, (int, np.integer)) or streams < 1:
            raise ValueError(f"ZoneCounter: streams must be an integer >= 1 (got {streams!r})")
        if isinstance(max_boxes, (bool, np.bool_)) or not isinstance(max_boxes, (int, np.integer)) or not 1 <= max_boxes <= MAX_BOXES:
            raise ValueError(f"ZoneCounter: max_boxes must be an integer in 1..{MAX_BOXES} (got {max_boxes!r})")
        table, self.zone_names, self.line_names = build_table(frame_size, zones, lines, anchor, min_frames, min_keypoint_score)
        self.streams, self.max_boxes = int(streams), int(max_boxes)
        self.frame_size = (float(table[0]['height']), float(table[0]['width']))
        self.anchor, self.min_frames, self.min_keypoint_score = anchor, int(min_frames), float(min_keypoint_score)
        lib = _lib.lib()
        self.state_bytes = lib.mpn_zone_state_bytes(self.streams)
        if lib.mpn_zone_table_bytes() != TABLE.itemsize or self.state_bytes != self.streams * STATE.itemsize:
            raise _lib.MpnError("mpn_zone_events: the table's or the state's layout is not the one this binding was written against")
        import torch
        self.device = torch.device(device) if device is not None else _lib.current_device()
        self.host_table = table
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(self.device)
        boxes_only = table.copy()                                   # for records without keypoints: 'feet' is its own fallback
        if boxes_only[0]['anchor'] == ANCHORS['feet']:
            boxes_only[0]['anchor'] = ANCHORS['box_bottom']
        self.table_boxes = torch.from_numpy(boxes_only.view(np.uint8).copy()).to(self.device)
        self._make_state(STATE.itemsize)
        self._update = {}
        self.last_out = None

    # ---------------------------------------------------------------- the device side
    def check_frame_sizes(self, sizes):
        """Raises unless every (height, width) of `sizes` is the counter's frame_size."""
        for h, w in sizes:
            if (float(h), float(w)) != self.frame_size:
                raise ValueError(f"zones=: the counter's zones are in the pixels of {self.frame_size[0]:g} x {self.frame_size[1]:g} "
                                 f"frames (height x width), this call has a frame of {h} x {w}")

    def out_bytes(self, b):
        """The bytes of a call's rows for b images."""
        self.check_batch(b)
        n = _lib.lib().mpn_zone_out_bytes(b, self.max_boxes)
        if n == 0 or n != b * (self.max_boxes * PERSON.itemsize + IMAGE.itemsize):
            raise ValueError(f"mpn_zone_events: {b} x {self.max_boxes} slots are more than one launch takes")
        return n

    def launch(self, record, track_rows, out, b, keypoints=True):
        """record: the uint8 device tensor the tracker read; track_rows: the uint8 device tensor of mpn_pose_track's rows for it;
        out: uint8 device tensor of `out_bytes(b)`. keypoints=False (a record without keypoints, whose zeros would pass for
        ankles): 'feet' reads as 'box_bottom'. Reads `prev`, writes `next` and out; `commit()` advances the state."""
        self.check_batch(b)
        _lib.call("mpn_zone_events", _lib.ptr(record), _lib.ptr(track_rows), b, self.max_boxes, self.streams,
                  _lib.ptr(self.table if keypoints else self.table_boxes), _lib.ptr(self.prev), _lib.ptr(self.next), _lib.ptr(out),
                  _lib.stream_ptr())
        return out

    def state(self, stream=0):
        """A host copy of one stream's current state, as a STATE record."""
        return self._raw_state(stream).view(STATE)[0]

    def totals(self, stream=0):
        """A host copy of one stream's cumulative counters: {'frames', 'entries', 'exits' (by zone name), 'line_positive',
        'line_negative' (by line name)}."""
        st = self.state(stream)
        return {'frames': int(st['frames']),
                'entries': {k: int(st['zone_entries'][i]) for i, k in enumerate(self.zone_names)},
                'exits': {k: int(st['zone_exits'][i]) for i, k in enumerate(self.zone_names)},
                'line_positive': {k: int(st['line_positive'][i]) for i, k in enumerate(self.line_names)},
                'line_negative': {k: int(st['line_negative'][i]) for i, k in enumerate(self.line_names)}}

    def unpack(self, out, counts):
        """A host copy of the output rows (uint8 array) and the record's per-image counts -> a list of b dicts. With Z zones
        and L lines, in the order they were given, and n persons in the image's record order: 'inside', 'entered', 'exited'
        bool [n, Z]; 'crossed_positive', 'crossed_negative' bool [n, L]; 'anchor' f64 [n, 2] (x, y); 'anchor_from_keypoints'
        bool [n]; 'tracked' bool [n] (the person has an identity here); 'no_anchor' bool [n]; 'dwell_frames' int32 [n, Z]; and
        for the frame 'occupancy', 'entries', 'exits', 'total_entries', 'total_exits' uint32 [Z], 'line_positive',
        'line_negative', 'total_line_positive', 'total_line_negative' uint32 [L]."""
        b = len(counts)
        Z, L = len(self.zone_names), len(self.line_names)
        at = b * self.max_boxes * PERSON.itemsize
        persons = np.frombuffer(out, np.uint8, at).view(PERSON)
        images = np.frombuffer(out, np.uint8, b * IMAGE.itemsize, at).view(IMAGE)
        zbits, lbits = np.arange(Z, dtype=np.uint32)[None, :], np.arange(L, dtype=np.uint32)[None, :]
        res, s = [], 0
        for i in range(b):
            n = int(counts[i])
            r, im = persons[s:s + n], images[i]
            res.append({'inside': ((r['inside'][:, None] >> zbits) & 1) != 0, 'entered': ((r['entered'][:, None] >> zbits) & 1) != 0,
                        'exited': ((r['exited'][:, None] >> zbits) & 1) != 0,
                        'crossed_positive': ((r['crossed_positive'][:, None] >> lbits) & 1) != 0,
                        'crossed_negative': ((r['crossed_negative'][:, None] >> lbits) & 1) != 0,
                        'anchor': r['anchor'].copy(), 'anchor_from_keypoints': (r['flags'] & FLAG_ANKLES) != 0,
                        'tracked': (r['flags'] & FLAG_TRACKED) != 0, 'no_anchor': (r['flags'] & FLAG_NO_ANCHOR) != 0,
                        'dwell_frames': r['dwell'][:, :Z].copy(),
                        'occupancy': im['occupancy'][:Z].copy(), 'entries': im['entries'][:Z].copy(), 'exits': im['exits'][:Z].copy(),
                        'total_entries': im['total_entries'][:Z].copy(), 'total_exits': im['total_exits'][:Z].copy(),
                        'line_positive': im['positive'][:L].copy(), 'line_negative': im['negative'][:L].copy(),
                        'total_line_positive': im['total_positive'][:L].copy(),
                        'total_line_negative': im['total_negative'][:L].copy()})
            s += n
        return res

    def update(self, outputs):
        """The same launch for host arrays: b result dicts that carry 'boxes', 'scores', 'keypoints' and 'track_ids' (as
        `Detector.predict_*(track=...)` returns them, or with the ids of any other tracker; at most max_boxes persons each)
        are packed, uploaded, counted and committed. Dicts without 'keypoints' take the box fallback. Returns what `unpack`
        returns."""
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
        self.last_out = out                                         # the call's raw rows (the two tables of include/mpn.h)
        return self.unpack(out, counts)
