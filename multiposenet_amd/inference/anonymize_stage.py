"""Persons made unrecognisable on the device (`mpn_anonymize`, include/mpn.h states the arithmetic): per person of a record the
head - a square around the five face joints - or the whole box is pixelated, blurred or filled, inside the captured graph of
the `predict_*` methods, between the gather (or `mpn_pose_nms`) and the drawing.

    detector.predict_jpegs(files, annotate='jpeg', anonymize=Anonymize())      # 'annotated_jpeg' shows the anonymised frame
    anonymize(image, outputs, Anonymize(mode='blur'))                          # the same launch for one host frame

Here: `Anonymize`, which says how; `Anonymizer`, the device buffers of one batch shape and the launch, in the manner of
`draw.Buffers`; `anonymize`, the one-frame host call."""
import ctypes
import math

import numpy as np

from .. import _lib
from ..stream_state import choice, integer
from . import draw

REGIONS = {'head': 0, 'box': 1}
MODES = {'pixelate': 0, 'blur': 1, 'fill': 2}
SHAPES = {'ellipse': 0, 'rectangle': 1}
MAX_BLOCKS, MAX_RADIUS = 32, 12                                     # MPN_ANONYMIZE_MAX_BLOCKS, MPN_ANONYMIZE_MAX_RADIUS
MAX_BOXES = draw.MAX_BOXES
NUM_KEYPOINTS = 17


class Params(ctypes.Structure):
    """mpn_anonymize_params (include/mpn.h); its size is checked against the library."""
    _fields_ = [('region', ctypes.c_int32), ('mode', ctypes.c_int32), ('shape', ctypes.c_int32), ('blocks', ctypes.c_int32),
                ('radius', ctypes.c_int32), ('color', ctypes.c_int32), ('min_keypoint_score', ctypes.c_float),
                ('reserved', ctypes.c_int32), ('scale', ctypes.c_double), ('min_size', ctypes.c_double),
                ('fallback', ctypes.c_double)]


def _number(name, value, rule, ok):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"Anonymize: {name} must be a number (got {value!r})") from None
    if isinstance(value, (bool, np.bool_, str)):
        raise ValueError(f"Anonymize: {name} must be a number (got {value!r})")
    if not math.isfinite(v):
        raise ValueError(f"Anonymize: {name} must be finite (got {value!r})")
    if not ok(v):
        raise ValueError(f"Anonymize: {name} must be {rule} (got {value!r})")
    return v


class Anonymize:
    """How persons are made unrecognisable (`Detector.predict_*(anonymize=...)`, `anonymize`). Immutable and hashable: part
    of the key of a Detector's graph.

    region: 'head' - the square around the mean of the face joints (nose, eyes, ears) that score at least
    min_keypoint_score, its half side the largest distance of such a joint from the mean along x or y times `scale`, at least
    the box height times `min_size`; a person without such a joint (or a Detector without the PRN) takes the top `fallback`
    of its box instead - or 'box', the whole box. shape: the 'ellipse' inscribed in the region, or the 'rectangle'. mode:
    'pixelate' - a mosaic of at most blocks x blocks cells, each the mean of its source pixels; 'blur' - three box blurs of
    radius `radius`, close to a Gaussian; 'fill' - `color`. overlay: True draws boxes, skeletons and identities over the
    anonymised frame as `annotate` does without it, False returns the anonymised frame alone.
    The defaults are NOT tuned: there are no trained weights in this repository to tune them on."""
    __slots__ = ('region', 'mode', 'shape', 'blocks', 'radius', 'color', 'scale', 'min_size', 'fallback', 'min_keypoint_score',
                 'overlay')

    def __init__(self, region='head', mode='pixelate', shape='ellipse', blocks=8, radius=8, color=(0, 0, 0), scale=2.0,
                 min_size=0.1, fallback=0.25, min_keypoint_score=0.0, overlay=True):
        try:
            rgb = tuple(color)
            if len(rgb) != 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in rgb):
                raise TypeError
        except TypeError:
            raise ValueError(f"Anonymize: color must be three integers (r, g, b) (got {color!r})") from None
        if not all(0 <= v <= 255 for v in rgb):
            raise ValueError(f"Anonymize: color must lie in 0..255 (got {color!r})")
        if not isinstance(overlay, (bool, np.bool_)):
            raise ValueError(f"Anonymize: overlay must be False or True (got {overlay!r})")
        mks = _number('min_keypoint_score', min_keypoint_score, "finite", lambda v: True)
        with np.errstate(over='ignore'):
            mks32 = float(np.float32(mks))                          # what the launch compares against
        if not math.isfinite(mks32):
            raise ValueError(f"Anonymize: min_keypoint_score must be finite (got {min_keypoint_score!r})")
        values = dict(region=choice('Anonymize', 'region', region, REGIONS), mode=choice('Anonymize', 'mode', mode, MODES),
                      shape=choice('Anonymize', 'shape', shape, SHAPES), blocks=integer('Anonymize', 'blocks', blocks, 2, MAX_BLOCKS),
                      radius=integer('Anonymize', 'radius', radius, 1, MAX_RADIUS), color=tuple(int(v) for v in rgb),
                      scale=_number('scale', scale, "> 0", lambda v: v > 0),
                      min_size=_number('min_size', min_size, ">= 0", lambda v: v >= 0),
                      fallback=_number('fallback', fallback, "in (0, 1]", lambda v: 0 < v <= 1),
                      min_keypoint_score=mks32, overlay=bool(overlay))
        for name in self.__slots__:
            object.__setattr__(self, name, values[name])

    def __setattr__(self, name, value):
        raise AttributeError("Anonymize is immutable")

    def __delattr__(self, name):
        raise AttributeError("Anonymize is immutable")

    def astuple(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return type(other) is Anonymize and self.astuple() == other.astuple()

    def __hash__(self):
        return hash(self.astuple())

    def __repr__(self):
        return "Anonymize(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__) + ")"

    def params(self):
        """The mpn_anonymize_params of this spec."""
        r, g, b = self.color
        return Params(REGIONS[self.region], MODES[self.mode], SHAPES[self.shape], self.blocks, self.radius, r | g << 8 | b << 16,
                      self.min_keypoint_score, 0, self.scale, self.min_size, self.fallback)


def check_spec(spec):
    if not isinstance(spec, Anonymize):
        raise ValueError(f"anonymize must be None or an inference.Anonymize (got {spec!r})")
    return spec


def check_max_boxes(max_boxes):
    if not 1 <= int(max_boxes) <= MAX_BOXES:
        raise ValueError(f"anonymize: max_boxes must be in 1..{MAX_BOXES} (got {max_boxes}), as for annotate")
    return int(max_boxes)


def add_arguments(ap):
    """The command line's flags of the stage (track_frames)."""
    ap.add_argument("--anonymize", nargs="?", const="head", default=None, choices=tuple(REGIONS), metavar="REGION",
                    help="make every detected person unrecognisable in the frames of --frames-out, on the device: its 'head' "
                         "(default) or its whole 'box'")
    ap.add_argument("--anonymize-mode", choices=tuple(MODES), default="pixelate", help="how (--anonymize)")
    ap.add_argument("--anonymize-shape", choices=tuple(SHAPES), default="ellipse", help="the region's shape (--anonymize)")
    ap.add_argument("--anonymize-blocks", type=int, default=8, metavar="N", help="mosaic cells per side, 2..32 (--anonymize)")
    ap.add_argument("--anonymize-radius", type=int, default=8, metavar="R", help="box blur radius, 1..12 (--anonymize)")
    ap.add_argument("--anonymize-no-overlay", action="store_true",
                    help="write the anonymised frames alone, without boxes, skeletons and identities (--anonymize)")


def from_arguments(ap, args):
    """The parsed flags of `add_arguments` -> None or the Anonymize; a bad value ends the program through ap.error (status 2)."""
    if args.anonymize is None:
        return None
    try:
        return Anonymize(region=args.anonymize, mode=args.anonymize_mode, shape=args.anonymize_shape, blocks=args.anonymize_blocks,
                         radius=args.anonymize_radius, overlay=not args.anonymize_no_overlay)
    except ValueError as e:
        ap.error(str(e))


class Anonymizer:
    """The device side of `mpn_anonymize` for b frames of at most `source_bytes` packed RGB bytes: descriptors (with their
    pinned staging), the output - a buffer like the sources, every frame at its source offset - and the workspace. The grids
    depend on (b, max_boxes, spec) alone: the launch can be captured, and the graph follows whatever `place` uploads later."""

    def __init__(self, b, max_boxes, source_bytes, device, spec=None):
        import torch
        lib = _lib.lib()
        if lib.mpn_draw_desc_bytes() != draw.DESC_WORDS * 4 or lib.mpn_anonymize_params_bytes() != ctypes.sizeof(Params):
            raise _lib.MpnError("mpn_anonymize: the layout of the descriptors or the parameters is not the one this binding "
                                "was written against")
        work = lib.mpn_anonymize_workspace_bytes(int(b), int(max_boxes))
        if work == 0:
            raise ValueError(f"anonymize: {b} x {max_boxes} slots are more than mpn_anonymize takes in one launch "
                             f"(max_boxes <= {MAX_BOXES}, b * max_boxes <= 4096)")
        self.b, self.max_boxes, self.spec = int(b), int(max_boxes), Anonymize() if spec is None else check_spec(spec)
        self.device = torch.device(device)
        self.desc_stage = torch.zeros((self.b, draw.DESC_WORDS), dtype=torch.int32).pin_memory()
        self.desc = torch.zeros((self.b, draw.DESC_WORDS), dtype=torch.int32, device=device)
        self.out = torch.empty(max(int(source_bytes), 3), dtype=torch.uint8, device=device)
        self.work = torch.empty(work, dtype=torch.uint8, device=device)
        self.frames = []

    def place(self, shapes, src_offsets):
        """This call's frames: the descriptors go to the device (one small copy, ordered before the launch on the stream)."""
        desc, _, _ = draw.layout(shapes, src_offsets)
        frames = [(int(at), int(h), int(w)) for (h, w), at in zip(shapes, src_offsets)]
        if any(at + h * w * 3 > self.out.numel() for at, h, w in frames):
            raise ValueError("anonymize: the frames exceed the output buffer")
        self.frames = frames
        self.desc_stage.numpy()[...] = desc
        self.desc.copy_(self.desc_stage, non_blocking=True)

    def launch(self, sources, record, with_keypoints, spec=None):
        """sources: flat uint8 device tensor; record: mpn_pose_gather's (uint8 device tensor) -> the packed RGB output."""
        params = (self.spec if spec is None else check_spec(spec)).params()
        _lib.call("mpn_anonymize", _lib.ptr(sources), sources.numel(), _lib.ptr(self.desc), _lib.ptr(record), record.numel(),
                  self.b, self.max_boxes, int(bool(with_keypoints)), ctypes.byref(params), _lib.ptr(self.out), self.out.numel(),
                  _lib.ptr(self.work), self.work.numel(), _lib.stream_ptr())
        return self.out

    def unpack(self, host):
        """A host copy of the packed output -> the frames as uint8 [h, w, 3] arrays of their own."""
        return [host[at:at + h * w * 3].reshape(h, w, 3).copy() for at, h, w in self.frames]


def pixel_keypoints(boxes, keypoint_scores, keypoint_positions, height, width):
    """mpn_pose_gather's float32 arithmetic (include/mpn.h) for host arrays: boxes [n, 4] normalised, positions [n, 17, 2]
    (y, x) normalised to the box -> [n, 17, 3] (x, y, score): x = xmin*width + pos_x * (xmax*width - xmin*width)."""
    f = np.float32
    boxes = np.asarray(boxes, f).reshape(-1, 4)
    pos = np.asarray(keypoint_positions, f).reshape(len(boxes), NUM_KEYPOINTS, 2)
    out = np.zeros((len(boxes), NUM_KEYPOINTS, 3), f)
    for c, (lo_i, hi_i, size, p_i) in enumerate(((1, 3, f(width), 1), (0, 2, f(height), 0))):
        lo = (boxes[:, lo_i] * size).astype(f)[:, None]
        hi = (boxes[:, hi_i] * size).astype(f)[:, None]
        out[:, :, c] = (lo + (pos[:, :, p_i] * (hi - lo).astype(f)).astype(f)).astype(f)
    out[:, :, 2] = np.asarray(keypoint_scores, f).reshape(len(boxes), NUM_KEYPOINTS)
    return out


_anonymizers = {}


def anonymize(image, outputs, spec=None):
    """One uint8 [h, w, 3] host frame and its result dict ('boxes' [n, 4] normalised; 'keypoints' [n, 17, 3] in image pixels as
    `predict_batch` returns them, or 'keypoint_positions' + 'keypoint_scores' as `Detector.__call__` returns them, which go
    through the gather's float32 arithmetic; neither: boxes only, every person takes the fallback region) -> the anonymised
    frame, uint8 [h, w, 3], made by one mpn_anonymize on the device. spec: an `Anonymize` (default: `Anonymize()`);
    `overlay` draws nothing here."""
    import torch
    from ..pose_metrics import fill_record
    spec = Anonymize() if spec is None else check_spec(spec)
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8 or image.size == 0:
        raise ValueError(f"image must be uint8 [height, width, 3] (got {image.dtype} {image.shape})")
    h, w, _ = image.shape
    boxes = np.asarray(outputs['boxes'], np.float32).reshape(-1, 4)
    n = len(boxes)
    person = {'boxes': boxes, 'scores': np.zeros(n, np.float32)}
    if 'keypoints' in outputs and len(outputs['keypoints']) == n:
        person['keypoints'] = np.asarray(outputs['keypoints'], np.float32)
    elif all(k in outputs and len(outputs[k]) == n for k in ('keypoint_positions', 'keypoint_scores')):
        person['keypoints'] = pixel_keypoints(boxes, outputs['keypoint_scores'], outputs['keypoint_positions'], h, w)
    max_boxes = 32
    while max_boxes < n:
        max_boxes *= 2
    check_max_boxes(max_boxes)
    device = _lib.current_device()
    capacity = 1 << max(int(image.size - 1).bit_length(), 12)
    key = (max_boxes, capacity, str(device))
    if key not in _anonymizers:
        _anonymizers[key] = Anonymizer(1, max_boxes, capacity, device)
    a = _anonymizers[key]
    record, _ = fill_record([person], 1, max_boxes)
    with torch.cuda.device(device):
        sources = torch.zeros(capacity, dtype=torch.uint8, device=device)
        sources[:image.size].copy_(torch.from_numpy(np.ascontiguousarray(image).reshape(-1)))
        a.place([(h, w)], [0])
        out = a.launch(sources, torch.from_numpy(record).to(device), 'keypoints' in person, spec)
        return a.unpack(out.cpu().numpy())[0]
