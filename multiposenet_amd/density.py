"""Density maps for the persons `Detector.predict_*` returns: where in the picture persons stand, and how much, accumulated
over a grid of square cells for as long as the object lives - a dwell or footfall heat map - as a grid on request and, with
`annotate`, laid over the frame as a colour wash.

Two planes of counters per stream live on the device (`mpn_density_map`, include/mpn.h): `dwell` counts person-frames per
cell and needs no identities; `visits` counts the arrivals of an identity in a cell and needs `track=`. The launch runs inside
the Detector's captured graph behind the tracker's launches when `predict_*` is given `density=`, or through
`DensityMap.update` for host dicts. The picture (`mpn_draw_density`) blends a colour per level over the annotated RGBA frames
in place, before they are encoded.

    density = DensityMap(streams=1, frame_size=(720, 1280), cell=16)
    for frames in batches:
        for person in detector.predict_images(frames, density=density, annotate='jpeg'):
            person['density']['cell'], person['annotated_jpeg']
    density.grid()                                                  # uint32 [45, 80]

Like the tracker's, the launch is a PURE function of its inputs and the previous state; `commit()` advances the state (the
Detector does that once per call). Persons below the call's score_threshold are not rows of the record and are not counted, nor
are coasting tracks. With half_life every counter is halved once per half_life frames: stepwise, not exponential. No default
is tuned on video."""
import itertools
import math

import numpy as np

from . import _lib
from .pose_metrics import fill_record
from .stream_state import StreamState, choice, flag, integer
from .zones import ANCHORS, MAX_BOXES, SLOTS, track_rows_of

MIN_CELL, MAX_CELL, MAX_SIDE, MAX_CELLS, MAX_HALF_LIFE, MAX_FULL_SCALE = 4, 256, 8192, 16384, 65535, 2 ** 31 - 1
FOOTPRINTS = {'anchor': 0, 'box': 1}
PLANES = {'dwell': 0, 'visits': 1}
FLAG_TRACKED, FLAG_ANKLES, FLAG_NO_ANCHOR, FLAG_OUTSIDE, FLAG_VISIT = 1, 2, 4, 8, 16
TABLE_HEADER_WORDS, TABLE_SMOOTH, TABLE_SHOW_VISITS = 8, 1, 2
DESC_WORDS = 8                          # mpn_draw_desc in 32-bit words

SLOT = np.dtype([('id', np.int32), ('last', np.int32), ('cell1', np.int32), ('pad', np.int32)])
ROW = np.dtype([('row', np.int32), ('col', np.int32), ('flags', np.uint32), ('cells', np.uint32)])
IMAGE = np.dtype([('max_dwell', np.uint32), ('max_visits', np.uint32), ('counted', np.uint32), ('visits', np.uint32)])


def state_dtype(gh, gw):
    """The state of one stream (include/mpn.h) for a grid of gh x gw cells."""
    return np.dtype([('frames', np.int32), ('max_dwell', np.uint32), ('max_visits', np.uint32), ('pad', np.int32, (5,)),
                     ('slots', SLOT, (SLOTS,)), ('dwell', np.uint32, (gh, gw)), ('visits', np.uint32, (gh, gw))])


def draw_table(colormap, opacity, smooth, full_scale, show):
    """The table of mpn_draw_density as a uint8 array: flags, full_scale, six zero words, then per level R | G<<8 | B<<16 |
    A<<24 with A[l] = (opacity * l + 127) // 255 and A[0] = 0. colormap: uint8 [256, 3]."""
    table = np.zeros(_lib.lib().mpn_draw_density_tables_bytes(), np.uint8)
    words = table.view(np.uint32)
    words[0] = (TABLE_SMOOTH if smooth else 0) | (TABLE_SHOW_VISITS if show == 'visits' else 0)
    words[1] = full_scale
    rgb = np.asarray(colormap, np.uint32)
    alpha = (opacity * np.arange(256, dtype=np.uint32) + 127) // 255
    alpha[0] = 0
    words[TABLE_HEADER_WORDS:TABLE_HEADER_WORDS + 256] = rgb[:, 0] | rgb[:, 1] << 8 | rgb[:, 2] << 16 | alpha << 24
    return table


class DensityMap(StreamState):
    """Where persons stand, accumulated per cell of a grid over the frame, for `streams` independent cameras, on the device
    (`mpn_density_map`), and how `annotate` draws it (`mpn_draw_density`).

    frame_size: (height, width) of the frames in source pixels, two integers in 1..8192. cell: the side of a cell in pixels
    (4..256); the grid has ceil(height / cell) x ceil(width / cell) cells, at most 16384. footprint: 'anchor' (a person adds 1
    to the cell its anchor stands in) or 'box' (to every cell whose centre its box covers). anchor, min_keypoint_score: the
    point that stands for a person, as for `zones.ZoneCounter`. half_life: every counter is halved once per half_life frames
    (0: never; up to 65535). show: the plane the picture shows, 'dwell' (person-frames per cell) or 'visits' (arrivals of an
    identity in a cell: it needs the tracker's ids). max_boxes: the detection slots per image of the records.
    draw: with `annotate`, the map is laid over the frame. smooth: the levels are interpolated between the cells' centres.
    full_scale: the count at which the colour saturates (1..2^31-1), or 0: each frame's own maximum. opacity: the alpha of the
    highest level (0..255); level l has (opacity * l + 127) // 255 and level 0 is not drawn. colormap: None (the RGB of
    `inference.maps.colour_table()`, matplotlib's 'autumn') or uint8 [256, 3].

    A call over b images sees b / streams consecutive frames per stream, stream s owning images s*F .. s*F+F-1 in time order,
    as `tracking.PoseTracker` does. The object owns the drawing's table on the device and the state - per stream 64 identities
    with the cell each was last seen in, and the two planes - as a prev / next pair. `launch` is pure; `commit()` advances the
    state. No default is tuned on video."""
    keyword, _serials = 'density', itertools.count(1)

    def __init__(self, streams=1, frame_size=None, cell=16, footprint='anchor', anchor='feet', min_keypoint_score=0.0, half_life=0,
                 show='dwell', draw=True, smooth=True, full_scale=0, opacity=160, colormap=None, max_boxes=25, device=None):
        if isinstance(streams, (bool, np.bool_)) or not isinstance(streams, (int, np.integer)) or streams < 1:
            raise ValueError(f"DensityMap: streams must be an integer >= 1 (got {streams!r})")
        self.max_boxes = integer('DensityMap', 'max_boxes', max_boxes, 1, MAX_BOXES)
        try:
            height, width = frame_size
        except (TypeError, ValueError):
            raise ValueError(f"DensityMap: frame_size must be (height, width) (got {frame_size!r})") from None
        for v in (height, width):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_SIDE:
                raise ValueError(f"DensityMap: frame_size must be two integers (height, width) in 1..{MAX_SIDE} (got {frame_size!r})")
        self.cell = integer('DensityMap', 'cell', cell, MIN_CELL, MAX_CELL)
        self.gh, self.gw = -(-int(height) // self.cell), -(-int(width) // self.cell)
        if self.gh * self.gw > MAX_CELLS:
            raise ValueError(f"DensityMap: a grid of {self.gh} x {self.gw} cells has more than {MAX_CELLS}; take a larger cell "
                             f"(got {cell!r})")
        self.footprint = choice('DensityMap', 'footprint', footprint, FOOTPRINTS)
        self.anchor = choice('DensityMap', 'anchor', anchor, ANCHORS)
        try:
            mks = float(min_keypoint_score)
        except (TypeError, ValueError):
            raise ValueError(f"DensityMap: min_keypoint_score must be a number (got {min_keypoint_score!r})") from None
        if not math.isfinite(mks):
            raise ValueError(f"DensityMap: min_keypoint_score must be finite (got {min_keypoint_score!r})")
        self.half_life = integer('DensityMap', 'half_life', half_life, 0, MAX_HALF_LIFE)
        self.show = choice('DensityMap', 'show', show, PLANES)
        self.draw, self.smooth = flag('DensityMap', 'draw', draw), flag('DensityMap', 'smooth', smooth)
        self.full_scale = integer('DensityMap', 'full_scale', full_scale, 0, MAX_FULL_SCALE)
        self.opacity = integer('DensityMap', 'opacity', opacity, 0, 255)
        if colormap is None:
            from .inference.maps import colour_table
            colormap = colour_table()[:, :3]
        else:
            colormap = np.asarray(colormap)
            if colormap.dtype != np.uint8 or colormap.shape != (256, 3):
                raise ValueError(f"DensityMap: colormap must be None or uint8 [256, 3] (got {colormap.dtype} {colormap.shape})")
        self.colormap = np.array(colormap, np.uint8)
        self.streams, self.frame_size = int(streams), (int(height), int(width))
        self.min_keypoint_score = mks
        self.state_row = state_dtype(self.gh, self.gw)
        lib = _lib.lib()
        self.state_bytes = lib.mpn_density_state_bytes(self.streams, self.gh, self.gw)
        if self.state_bytes != self.streams * self.state_row.itemsize:
            raise ValueError(f"DensityMap: streams = {streams!r} are more than mpn_density_map takes")
        self.host_table = draw_table(self.colormap, self.opacity, self.smooth, self.full_scale, self.show)
        import torch
        self.device = torch.device(device) if device is not None else _lib.current_device()
        self.table = torch.from_numpy(self.host_table.copy()).to(self.device)
        self._make_state(self.state_row.itemsize)
        self._update, self._work, self._snapshots = {}, {}, {}
        self.last_out = None

    # ---------------------------------------------------------------- the device side
    def check_frame_sizes(self, sizes):
        """Raises unless every (height, width) of `sizes` is the object's frame_size."""
        for h, w in sizes:
            if (int(h), int(w)) != self.frame_size:
                raise ValueError(f"density=: the grid covers {self.frame_size[0]} x {self.frame_size[1]} frames (height x width), "
                                 f"this call has a frame of {h} x {w}")

    def out_bytes(self, b):
        """The bytes of a call's rows for b images."""
        self.check_batch(b)
        n = _lib.lib().mpn_density_out_bytes(b, self.max_boxes)
        if n == 0 or n != b * self.max_boxes * ROW.itemsize + b * IMAGE.itemsize:
            raise ValueError(f"mpn_density_map: {b} x {self.max_boxes} slots are more than one launch takes")
        return n

    def snapshots(self, b):
        """The device buffer of a batch size's snapshots, uint8 of b * G * 4 bytes, made on its first use (before a capture: the
        Detector's warm-up run)."""
        import torch
        if b not in self._snapshots:
            need = _lib.lib().mpn_density_snapshot_bytes(b, self.gh, self.gw)
            if need == 0:
                raise ValueError(f"mpn_density_map: {b} images are more than one launch takes")
            self._snapshots[b] = torch.zeros(need, dtype=torch.uint8, device=self.device)
        return self._snapshots[b]

    def launch(self, record, track_rows, out, b, keypoints=True, snapshots=None):
        """record: the uint8 device tensor of mpn_pose_gather's layout; track_rows: the uint8 device tensor of mpn_pose_track's
        rows for it, or None (no identities: the dwell plane alone); out: uint8 device tensor of `out_bytes(b)`. keypoints=False
        (a record without keypoints, whose zeros would pass for ankles): 'feet' reads as 'box_bottom'. snapshots: None or
        `snapshots(b)`. Reads `prev`, writes `next`, out and the snapshots; `commit()` advances the state."""
        self.check_batch(b)
        if track_rows is None and self.show == 'visits':
            raise ValueError("density=: show='visits' counts the arrivals of identities: it needs a tracker's ids")
        _lib.call("mpn_density_map", _lib.ptr(record), _lib.ptr(track_rows) if track_rows is not None else None, b, self.max_boxes,
                  self.streams, self.frame_size[0], self.frame_size[1], self.cell, FOOTPRINTS[self.footprint], ANCHORS[self.anchor],
                  self.min_keypoint_score, int(bool(keypoints)), self.half_life, PLANES[self.show], _lib.ptr(self.prev),
                  _lib.ptr(self.next), _lib.ptr(out), _lib.ptr(snapshots) if snapshots is not None else None, _lib.stream_ptr())
        return out

    def launch_draw(self, descs, snapshots, rows, out_rgba, b):
        """mpn_draw_density over the RGBA frames `out_rgba` (flat uint8 device tensor) that the drawing wrote for the descriptors
        `descs`: the snapshots and rows `launch` wrote, as a colour wash, IN PLACE. The workspace of a batch size is made on its
        first use (before a capture: the Detector's warm-up run)."""
        import torch
        if b not in self._work:
            need = _lib.lib().mpn_draw_density_workspace_bytes(b, self.gh, self.gw)
            if need == 0:
                raise ValueError(f"mpn_draw_density: {b} images are more than one launch takes")
            self._work[b] = torch.empty(need, dtype=torch.uint8, device=self.device)
        work = self._work[b]
        _lib.call("mpn_draw_density", _lib.ptr(descs), _lib.ptr(snapshots), _lib.ptr(rows), _lib.ptr(self.table), self.table.numel(),
                  b, self.max_boxes, self.frame_size[0], self.frame_size[1], self.cell, _lib.ptr(out_rgba), out_rgba.numel(),
                  _lib.ptr(work), work.numel(), _lib.stream_ptr())
        return out_rgba

    def state(self, stream=0):
        """A host copy of one stream's current state, as a `state_dtype(gh, gw)` record."""
        return self._raw_state(stream).view(self.state_row)[0]

    def grid(self, stream=0, plane='dwell'):
        """A host copy of one stream's current plane, 'dwell' or 'visits': uint32 [gh, gw]."""
        if not isinstance(plane, str) or plane not in PLANES:
            raise ValueError(f"plane must be one of {list(PLANES)} (got {plane!r})")
        return self.state(stream)[plane].copy()

    def unpack(self, out, counts):
        """A host copy of the output rows (uint8 array) and the record's per-image counts -> a list of b dicts. With n persons
        in the image's record order: 'cell' int32 [n, 2], (row, col) of the person's anchor cell, -1, -1 when it has none;
        'cells' int32 [n], the cells this person added to; 'tracked' (the person has an identity here), 'visit' (it arrived in
        its cell in this frame), 'outside' (its anchor is not in the frame), 'anchor_from_keypoints' bool [n]; and the frame's
        'max_dwell', 'max_visits' (the planes' maxima after it), 'counted' (persons that added to a cell) and 'visits' as ints."""
        b = len(counts)
        person_bytes = b * self.max_boxes * ROW.itemsize
        rows = np.frombuffer(out, np.uint8, person_bytes).view(ROW)
        images = np.frombuffer(out, np.uint8, b * IMAGE.itemsize, person_bytes).view(IMAGE)
        res, s = [], 0
        for i in range(b):
            n = int(counts[i])
            r = rows[s:s + n]
            res.append({'cell': np.stack([r['row'], r['col']], axis=1).astype(np.int32).reshape(n, 2),
                        'cells': r['cells'].astype(np.int32), 'tracked': (r['flags'] & FLAG_TRACKED) != 0,
                        'visit': (r['flags'] & FLAG_VISIT) != 0, 'outside': (r['flags'] & FLAG_OUTSIDE) != 0,
                        'anchor_from_keypoints': (r['flags'] & FLAG_ANKLES) != 0,
                        'max_dwell': int(images[i]['max_dwell']), 'max_visits': int(images[i]['max_visits']),
                        'counted': int(images[i]['counted']), 'visits': int(images[i]['visits'])})
            s += n
        return res

    def update(self, outputs):
        """The same launch for host arrays: b result dicts that carry 'boxes' and 'scores' and, optionally, 'keypoints' and
        'track_ids' (as `Detector.predict_*` returns them; at most max_boxes persons each) are packed, uploaded, run and
        committed. Dicts without 'keypoints' take the box fallback; unless every dict has 'track_ids' there are no identities:
        the dwell plane alone is counted, and show='visits' is refused. Returns what `unpack` returns."""
        import torch
        outputs = list(outputs)
        b = len(outputs)
        nbytes = self.out_bytes(b)
        for o in outputs:
            if 'boxes' not in o or 'scores' not in o:
                raise ValueError("DensityMap: every output dict needs 'boxes' and 'scores'")
        tracked = all('track_ids' in o for o in outputs)
        if not tracked and self.show == 'visits':
            raise ValueError("DensityMap: show='visits' counts the arrivals of identities: every output dict needs 'track_ids'")
        rows = track_rows_of(outputs, b, self.max_boxes) if tracked else None
        record, counts = fill_record(outputs, b, self.max_boxes)
        keypoints = all('keypoints' in o and len(o['keypoints']) == len(o['scores']) for o in outputs)
        with torch.cuda.device(self.device):
            if b not in self._update:
                self._update[b] = (torch.zeros(len(record), dtype=torch.uint8, device=self.device),
                                   torch.zeros(b * self.max_boxes * 24, dtype=torch.uint8, device=self.device),
                                   torch.zeros(nbytes, dtype=torch.uint8, device=self.device))
            dev_record, dev_rows, dev_out = self._update[b]
            dev_record.copy_(torch.from_numpy(record))
            if tracked:
                dev_rows.copy_(torch.from_numpy(rows))
            self.launch(dev_record, dev_rows if tracked else None, dev_out, b, keypoints)
            self.commit()
            out = dev_out.cpu().numpy()
        self.last_out = out                                         # the call's raw rows (include/mpn.h)
        return self.unpack(out, counts)

    def draw_frame(self, image, stream=0):
        """`inference.draw_density`: one host frame of frame_size, uint8 [h, w, 3] or [h, w, 4] -> uint8 [h, w, 4] with the
        stream's current `show` plane laid over it."""
        import torch
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] not in (3, 4) or image.shape[0] < 1 or image.shape[1] < 1:
            raise ValueError(f"draw_density: image must be uint8 [h, w, 3] or [h, w, 4] (got {image.dtype} {image.shape})")
        h, w = image.shape[:2]
        if (h, w) != self.frame_size:
            raise ValueError(f"draw_density: the grid covers {self.frame_size[0]} x {self.frame_size[1]} frames (height x width), "
                             f"the image is {h} x {w}")
        state = self.state(stream)
        rgba = np.full((h, w, 4), 255, np.uint8)
        rgba[..., :image.shape[2]] = image
        rows = np.zeros(self.max_boxes * ROW.itemsize + IMAGE.itemsize, np.uint8)
        rows[self.max_boxes * ROW.itemsize:].view(IMAGE)[0] = (state['max_dwell'], state['max_visits'], 0, 0)
        desc = np.zeros((1, DESC_WORDS), np.int32)
        desc[0, 4:6] = (h, w)
        nbytes = (h * w * 4 + 15) // 16 * 16
        with torch.cuda.device(self.device):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)        # noqa: E731
            frame = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
            frame[:h * w * 4].copy_(up(rgba.reshape(-1)))
            self.launch_draw(up(desc), up(state[self.show].reshape(-1).view(np.uint8)), up(rows), frame, 1)
            return frame[:h * w * 4].cpu().numpy().reshape(h, w, 4)


def draw_density(image, density, stream=0):
    """The one-frame drawing call: a host RGB or RGBA frame (uint8 [h, w, 3] or [h, w, 4]) of the DensityMap's frame_size -> the
    frame as uint8 [h, w, 4] with the current grid of `stream` laid over it by `mpn_draw_density`, as `annotate` draws it.
    density: the DensityMap, whose show, smooth, full_scale, opacity and colormap say how."""
    if not isinstance(density, DensityMap):
        raise ValueError("draw_density: density must be a density.DensityMap")
    return density.draw_frame(image, stream)
