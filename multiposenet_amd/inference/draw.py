"""Host side of the annotated frames (`mpn_draw_detections`, include/mpn.h): the reference notebook's `draw_everything`
(inference/predict.ipynb, cells 10 and 12) drawn on the device - the frame as RGBA, every kept person's box in red, skeleton in
white, keypoints as red dots, byte for byte what Pillow draws there. Here: where every frame of a ragged batch lies in the
packed output, the descriptors, the device buffers of one batch shape and the launch.

`mpn_draw_tracks` draws the same picture for persons with identities (a `tracking.PoseTracker`'s rows): a colour per track id
and the id as a label. Here: `TrackStyle`, which says how, its table for the kernels, the digit stamps of the label, rendered
once per process from Pillow's default font, and `Buffers.launch_tracks`."""
import functools
import math

import numpy as np

from .. import _lib
from .resample import _round16

DESC_WORDS = 8                         # mpn_draw_desc in 32-bit words (32 bytes; checked against the library)
MAX_BOXES = 128                        # MPN_DRAW_MAX_BOXES

# mpn_draw_tracks' style table (include/mpn.h): header words, limits, the label's padding
TABLE_HEADER_WORDS, STAMP_WORDS = 58, 5
MAX_PALETTE, MAX_CELL, MAX_STAMP_H, LABEL_PAD = 256, 32, 48, 1
FLAG_LABELS, FLAG_HIDE = 1, 2
# identity colours: none is the red or the white of an untracked person
DEFAULT_PALETTE = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (148, 103, 189), (140, 86, 75), (227, 119, 194),
                   (23, 190, 207), (188, 189, 34), (0, 128, 128), (128, 0, 128), (0, 0, 205), (210, 105, 30))


@functools.lru_cache(maxsize=8)
def digit_stamps(label_size=10):
    """(stamps, cell) of the digits 0..9 in Pillow's default font at `label_size`: stamps = ten (mask uint8 [h, w], (ox, oy)),
    what `ImageDraw.text` blends for the digit and where (`font.getmask2`'s offset, added to the text's position); cell = the
    widest digit's advance, rounded up. Rendered once per size and process."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default(size=label_size)
    stamps, cell = [], 0
    for digit in "0123456789":
        core, (ox, oy) = font.getmask2(digit, 'L')
        sw, sh = core.size
        mask = np.zeros((max(sh, 0), max(sw, 0)), np.uint8)
        if sw > 0 and sh > 0:
            im = Image.new('L', (sw, sh), 0)
            ImageDraw.Draw(im).text((-ox, -oy), digit, fill=255, font=font)     # the mask itself: BLEND8(m, 0, 255) = m
            mask = np.asarray(im).copy()
        mask.setflags(write=False)
        stamps.append((mask, (int(ox), int(oy))))
        cell = max(cell, int(math.ceil(font.getlength(digit))))
    return tuple(stamps), cell


def label_metrics(stamps, cell):
    """(top, bot) of ten digit stamps: the rows, relative to the text's position, the digits cover. Raises ValueError when a
    stamp lies more than the label's padding outside its cell: the label's rectangle would not enclose it. (A glyph a pixel
    wider than its advance is fine: it reaches into the neighbouring cell, and the kernel blends both digits there.)"""
    top = min(oy for _, (_, oy) in stamps)
    bot = max(oy + m.shape[0] for m, (_, oy) in stamps)
    for d, (m, (ox, _)) in enumerate(stamps):
        if ox < -LABEL_PAD or ox + m.shape[1] > cell + LABEL_PAD:
            raise ValueError(f"the stamp of digit {d} (columns {ox} .. {ox + m.shape[1] - 1}) leaves its cell of {cell} pixels "
                             f"by more than the label's padding of {LABEL_PAD}")
    return top, bot


def _colour(name, c):
    try:
        r, g, b = (int(v) for v in c)
        if any(int(v) != v for v in c):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"TrackStyle: {name} must be (r, g, b) integers (got {c!r})") from None
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError(f"TrackStyle: {name} must lie in 0..255 (got {c!r})")
    return r, g, b


class TrackStyle:
    """How `annotate` draws tracked persons (`mpn_draw_tracks`). Immutable and hashable: part of the key of a Detector's graph.

    palette: None (DEFAULT_PALETTE) or 1..256 (r, g, b); a person with track id t > 0 has its box, dots and label in
    palette[(t - 1) % len(palette)], its skeleton in line_color. labels: the id in decimal digits on a filled tag above the
    box (inside it at the top of the frame), in text_color, in Pillow's default font at label_size. keypoints: 'frame' draws
    the frame's own keypoints, 'smoothed' the tracker's 'keypoints_smoothed' (needs PoseTracker(smooth=...)). untracked:
    'plain' draws a person without an id as `annotate` always has (red and white), 'hide' leaves it out."""
    __slots__ = ('palette', 'labels', 'label_size', 'keypoints', 'untracked', 'line_color', 'text_color')

    def __init__(self, palette=None, labels=True, label_size=10, keypoints='frame', untracked='plain',
                 line_color=(255, 255, 255), text_color=(255, 255, 255)):
        if palette is None:
            palette = DEFAULT_PALETTE
        try:
            palette = tuple(palette)
        except TypeError:
            raise ValueError(f"TrackStyle: palette must be a sequence of (r, g, b) (got {palette!r})") from None
        if not 1 <= len(palette) <= MAX_PALETTE:
            raise ValueError(f"TrackStyle: palette must hold 1..{MAX_PALETTE} colours (got {len(palette)})")
        if not isinstance(labels, (bool, np.bool_)):
            raise ValueError(f"TrackStyle: labels must be False or True (got {labels!r})")
        if isinstance(label_size, (bool, np.bool_)) or not isinstance(label_size, (int, np.integer)) or label_size < 1:
            raise ValueError(f"TrackStyle: label_size must be a positive integer (got {label_size!r})")
        if keypoints not in ('frame', 'smoothed'):
            raise ValueError(f"TrackStyle: keypoints must be 'frame' or 'smoothed' (got {keypoints!r})")
        if untracked not in ('plain', 'hide'):
            raise ValueError(f"TrackStyle: untracked must be 'plain' or 'hide' (got {untracked!r})")
        values = dict(palette=tuple(_colour(f"palette[{i}]", c) for i, c in enumerate(palette)), labels=bool(labels),
                      label_size=int(label_size), keypoints=keypoints, untracked=untracked,
                      line_color=_colour('line_color', line_color), text_color=_colour('text_color', text_color))
        for name, v in values.items():
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("TrackStyle is immutable")

    def __delattr__(self, name):
        raise AttributeError("TrackStyle is immutable")

    def astuple(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, TrackStyle) and self.astuple() == other.astuple()

    def __hash__(self):
        return hash(self.astuple())

    def __repr__(self):
        return "TrackStyle(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__) + ")"

    def tables(self, stamps=None, cell=None):
        """The style table of mpn_draw_tracks as a uint8 array (include/mpn.h: flags, colours, palette, the ten stamp
        descriptors, the stamps' L8 bytes). stamps, cell: default `digit_stamps(label_size)`."""
        if stamps is None:
            stamps, cell = digit_stamps(self.label_size)
        top, bot = label_metrics(stamps, cell)
        size = _lib.lib().mpn_draw_tracks_tables_bytes(len(self.palette), cell, bot - top)
        if size == 0:
            raise ValueError(f"TrackStyle: label_size {self.label_size} gives digit cells of {cell} x {bot - top} pixels; "
                             f"mpn_draw_tracks takes 1..{MAX_CELL} x 0..{MAX_STAMP_H}")
        table = np.zeros(size, np.uint8)
        words = table[:(TABLE_HEADER_WORDS + len(self.palette)) * 4].view(np.int32)
        pack = lambda c: c[0] | c[1] << 8 | c[2] << 16                                          # noqa: E731
        words[:7] = ((FLAG_LABELS if self.labels else 0) | (FLAG_HIDE if self.untracked == 'hide' else 0),
                     pack(self.line_color), pack(self.text_color), len(self.palette), cell, top, bot)
        words[TABLE_HEADER_WORDS:] = [pack(c) for c in self.palette]
        at = words.nbytes
        for d, (mask, (ox, oy)) in enumerate(stamps):
            h, w = mask.shape
            words[8 + STAMP_WORDS * d:8 + STAMP_WORDS * (d + 1)] = (w, h, ox, oy, at)
            table[at:at + h * w] = mask.reshape(-1)
            at += h * w
        table.setflags(write=False)
        return table


def out_capacity(source_bytes, b):
    """Bytes of packed RGBA output that hold ANY b frames whose packed RGB sources fit source_bytes (each frame's h*w*4 is
    rounded up to 16 bytes)."""
    return _round16(int(source_bytes) // 3 * 4 + 16 * b)


def layout(shapes, src_offsets):
    """[(h, w)] and the byte offsets of the frames in the packed sources -> (descriptors int32 [b, DESC_WORDS],
    frames [(out_offset, h, w)], out_bytes)."""
    desc = np.zeros((len(shapes), DESC_WORDS), np.int32)
    d64 = desc.view(np.int64)                                    # words 0-1 src_offset, 2-3 out_offset
    frames, at = [], 0
    for i, ((h, w), src) in enumerate(zip(shapes, src_offsets)):
        d64[i, 0], d64[i, 1] = src, at
        desc[i, 4:6] = (h, w)
        frames.append((at, int(h), int(w)))
        at += _round16(h * w * 4)
    return desc, frames, at


class Buffers:
    """The device side of the drawing for b frames of at most `source_bytes` packed RGB bytes: descriptors (with their pinned
    staging), the packed output, the primitive workspace, and an empty record for a graph without a person detector."""

    def __init__(self, b, max_boxes, source_bytes, device):
        import torch
        lib = _lib.lib()
        if lib.mpn_draw_desc_bytes() != DESC_WORDS * 4:
            raise _lib.MpnError("mpn_draw_detections: the descriptor's layout is not the one this binding was written against")
        work = max(lib.mpn_draw_detections_workspace_bytes(b, max_boxes), lib.mpn_draw_tracks_workspace_bytes(b, max_boxes))
        if work == 0:
            raise ValueError(f"annotate: {b} x {max_boxes} slots are more than mpn_draw_detections draws in one launch "
                             f"(max_boxes <= {MAX_BOXES}, b * max_boxes <= 4096)")
        self.b, self.max_boxes = b, max_boxes
        self.desc_stage = torch.zeros((b, DESC_WORDS), dtype=torch.int32).pin_memory()
        self.desc = torch.zeros((b, DESC_WORDS), dtype=torch.int32, device=device)
        self.out = torch.empty(out_capacity(source_bytes, b), dtype=torch.uint8, device=device)
        self.work = torch.empty(work, dtype=torch.uint8, device=device)
        self.no_record = torch.zeros(lib.mpn_pose_gather_record_bytes(b, max_boxes), dtype=torch.uint8, device=device)
        self.frames, self.out_bytes = [], 0

    def place(self, shapes, src_offsets):
        """This call's frames: the descriptors go to the device (one small copy, ordered before the launch on the stream)."""
        desc, self.frames, self.out_bytes = layout(shapes, src_offsets)
        if self.out_bytes > self.out.numel():
            raise ValueError("annotate: the frames exceed the output buffer")     # (out_capacity rules it out)
        self.desc_stage.numpy()[...] = desc
        self.desc.copy_(self.desc_stage, non_blocking=True)

    def launch(self, sources, record, with_keypoints):
        """sources: flat uint8 device tensor; record: mpn_pose_gather's (None: no persons) -> the packed RGBA output."""
        record = self.no_record if record is None else record
        _lib.call("mpn_draw_detections", _lib.ptr(sources), sources.numel(), _lib.ptr(self.desc), _lib.ptr(record), record.numel(),
                  self.b, self.max_boxes, int(bool(with_keypoints)), _lib.ptr(self.out), self.out.numel(), _lib.ptr(self.work),
                  self.work.numel(), _lib.stream_ptr())
        return self.out

    def launch_tracks(self, sources, record, track_rows, smooth_rows, tables, with_keypoints):
        """`launch` for tracked persons (mpn_draw_tracks): track_rows / smooth_rows are what mpn_pose_track / mpn_pose_smooth
        wrote for `record` (uint8 device tensors; smooth_rows None: the frame's own keypoints), tables a `TrackStyle.tables()`
        on the device."""
        _lib.call("mpn_draw_tracks", _lib.ptr(sources), sources.numel(), _lib.ptr(self.desc), _lib.ptr(record), record.numel(),
                  _lib.ptr(track_rows), _lib.ptr(smooth_rows), _lib.ptr(tables), tables.numel(), self.b, self.max_boxes,
                  int(bool(with_keypoints)), _lib.ptr(self.out), self.out.numel(), _lib.ptr(self.work), self.work.numel(),
                  _lib.stream_ptr())
        return self.out

    def unpack(self, host):
        """A host copy of the packed output -> the frames as uint8 [h, w, 4] arrays of their own."""
        return [host[at:at + h * w * 4].reshape(h, w, 4).copy() for at, h, w in self.frames]
