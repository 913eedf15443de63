"""The picture of every detected person, cut and resized on the device (`mpn_person_crops`, include/mpn.h states the
arithmetic): per person of a record Pillow's bicubic `resize((new_w, new_h), box=(x0, y0, x1, y1))` of its frame, byte for
byte, inside the captured graph of the `predict_*` methods, and optionally the JPEG file of every crop - only crops, or
compressed bytes, cross the link, never a whole frame.

    outs = detector.predict_images(frames, crops=PersonCrops())               # outs[i]['crops'] uint8 [n, 256, 128, 3]
    outs = detector.predict_jpegs(files, crops=PersonCrops(format='jpeg'))    # outs[i]['crops'] a list of n bytes
    person_crops(image, outputs, PersonCrops(fit='pad'))                      # the same launch for one host frame

Here: `PersonCrops`, which says how; `CropBuffers`, the device buffers of one batch shape and the launch, in the manner of
`anonymize_stage.Anonymizer`; `PersonCropper` and `person_crops`, the one-frame host call."""
import math

import numpy as np

from .. import _lib
from ..stream_state import choice, integer
from . import draw, jpeg

FITS = {'stretch': 0, 'pad': 1}
FORMATS = ('rgb', 'jpeg')
MAX_H, MAX_W = 512, 256                                             # MPN_PERSON_CROPS_MAX_H, MPN_PERSON_CROPS_MAX_W
MAX_PAD = 4.0
MAX_BOXES = draw.MAX_BOXES
TAP_WORDS = 68                                                      # MPN_PERSON_CROPS_TAP_WORDS
LDS_BYTES = 163840                                                  # MPN_PERSON_CROPS_LDS_BYTES
EMPTY, TOO_LARGE, CLIPPED, USED = 1, 2, 4, 8                        # MPN_PERSON_CROPS_*
# mpn_person_crops_info (64 bytes; checked against the library)
INFO = np.dtype([('rect', np.float64, (4,)), ('placed', np.int32, (4,)), ('flags', np.int32), ('image', np.int32),
                 ('ksize_x', np.int32), ('ksize_y', np.int32)])


def tile_rows(height, width):
    """The output rows a block of mpn_person_crops' second launch makes: the largest tile whose source rows at a 16x reduction,
    tile * 16 + 64 rows of width * 3 bytes, fit the block's LDS_BYTES ("Person crops")."""
    return min(height, max(1, (LDS_BYTES // (width * 3) - 64) // 16))


class PersonCrops:
    """How persons are cut out (`Detector.predict_*(crops=...)`, `person_crops`). Immutable and hashable: the object itself is
    part of the key of a Detector's graph.

    size: (height, width) of every crop, multiples of 8 with 8 <= height <= 512 and 8 <= width <= 256. pad: the box grows by
    pad times its width on the left and on the right and by pad times its height above and below, then is clamped to the
    frame. fit: 'stretch' resizes the rectangle to the whole crop; 'pad' keeps its aspect ratio and centres it, every other
    pixel `fill`. format: 'rgb' returns uint8 arrays, 'jpeg' the files Pillow would write for them with `jpeg_quality` and
    `jpeg_subsampling`, encoded on the device. max_boxes: the Detector's."""
    __slots__ = ('size', 'pad', 'fit', 'fill', 'format', 'jpeg_quality', 'jpeg_subsampling', 'max_boxes')

    def __init__(self, size=(256, 128), pad=0.0, fit='stretch', fill=(0, 0, 0), format='rgb', jpeg_quality=75,
                 jpeg_subsampling='4:2:0', max_boxes=25):
        try:
            hw = tuple(size)
            if len(hw) != 2 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in hw):
                raise TypeError
        except TypeError:
            raise ValueError(f"PersonCrops: size must be two integers (height, width) (got {size!r})") from None
        height, width = int(hw[0]), int(hw[1])
        if height % 8 or width % 8 or not 8 <= height <= MAX_H or not 8 <= width <= MAX_W:
            raise ValueError(f"PersonCrops: size must be multiples of 8 with 8 <= height <= {MAX_H} and 8 <= width <= {MAX_W} "
                             f"(got {size!r})")
        try:
            if isinstance(pad, (bool, np.bool_, str)):
                raise TypeError
            p = float(pad)
        except (TypeError, ValueError):
            raise ValueError(f"PersonCrops: pad must be a number (got {pad!r})") from None
        if not math.isfinite(p) or not 0.0 <= p <= MAX_PAD:
            raise ValueError(f"PersonCrops: pad must be in 0..{MAX_PAD:g} (got {pad!r})")
        try:
            rgb = tuple(fill)
            if len(rgb) != 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in rgb):
                raise TypeError
        except TypeError:
            raise ValueError(f"PersonCrops: fill must be three integers (r, g, b) (got {fill!r})") from None
        if not all(0 <= v <= 255 for v in rgb):
            raise ValueError(f"PersonCrops: fill must lie in 0..255 (got {fill!r})")
        try:
            jpeg.quality_tables(jpeg_quality)
            if isinstance(jpeg_quality, (bool, np.bool_)) or int(jpeg_quality) != jpeg_quality:
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"PersonCrops: jpeg_quality must be an integer in 1..100 (got {jpeg_quality!r})") from None
        if not isinstance(jpeg_subsampling, str) or jpeg_subsampling not in jpeg.SAMPLING:
            raise ValueError(f"PersonCrops: jpeg_subsampling must be one of {sorted(jpeg.SAMPLING)} (got {jpeg_subsampling!r})")
        values = dict(size=(height, width), pad=p, fit=choice('PersonCrops', 'fit', fit, FITS), fill=tuple(int(v) for v in rgb),
                      format=choice('PersonCrops', 'format', format, FORMATS), jpeg_quality=int(jpeg_quality),
                      jpeg_subsampling=jpeg_subsampling, max_boxes=integer('PersonCrops', 'max_boxes', max_boxes, 1, MAX_BOXES))
        for name in self.__slots__:
            object.__setattr__(self, name, values[name])

    def __setattr__(self, name, value):
        raise AttributeError("PersonCrops is immutable")

    def __delattr__(self, name):
        raise AttributeError("PersonCrops is immutable")

    def astuple(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return type(other) is PersonCrops and self.astuple() == other.astuple()

    def __hash__(self):
        return hash(self.astuple())

    def __repr__(self):
        return "PersonCrops(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__) + ")"

    @property
    def fill_word(self):
        r, g, b = self.fill
        return r | g << 8 | b << 16

    @property
    def crop_bytes(self):
        return self.size[0] * self.size[1] * 3


def check_spec(spec):
    if not isinstance(spec, PersonCrops):
        raise ValueError(f"crops must be None or an inference.PersonCrops (got {spec!r})")
    return spec


def add_arguments(ap):
    """The command line's flags of the stage (track_frames)."""
    ap.add_argument("--crops-out", metavar="DIR", default=None,
                    help="write every detected person as DIR/<frame name>_<k>.jpg (and _id<track id>.jpg where it has an id), cut, "
                         "resized and JPEG-encoded on the device")
    ap.add_argument("--crop-size", type=int, nargs=2, default=None, metavar=("H", "W"), help="of every crop (--crops-out)")
    ap.add_argument("--crop-pad", type=float, default=None, metavar="P", help="grow the box by P times its size (--crops-out)")
    ap.add_argument("--crop-fit", choices=tuple(FITS), default=None, help="stretch the box to the crop or pad it (--crops-out)")
    ap.add_argument("--crop-quality", type=int, default=None, metavar="Q", help="JPEG quality of the crops (--crops-out)")


def from_arguments(ap, args, max_boxes=25):
    """The parsed flags of `add_arguments` -> None or the PersonCrops (format='jpeg'); a bad value ends the program through
    ap.error (status 2)."""
    own = dict(size=args.crop_size, pad=args.crop_pad, fit=args.crop_fit, jpeg_quality=args.crop_quality)
    if args.crops_out is None:
        if any(v is not None for v in own.values()):
            ap.error("--crop-size, --crop-pad, --crop-fit and --crop-quality need --crops-out DIR")
        return None
    try:
        return PersonCrops(format='jpeg', max_boxes=max_boxes, **{k: v for k, v in own.items() if v is not None})
    except ValueError as e:
        ap.error(str(e))


def crop_file_names(frame_name, track_ids, count):
    """The file names of a frame's crops: <frame name>_<k>.jpg, and <frame name>_id<track id>.jpg for a person with an id."""
    stem = frame_name.rsplit('.', 1)[0] if '.' in frame_name else frame_name
    names = []
    for k in range(count):
        tid = int(track_ids[k]) if track_ids is not None and k < len(track_ids) else 0
        names.append(f"{stem}_id{tid}.jpg" if tid > 0 else f"{stem}_{k}.jpg")
    return names


def unpack_info(rows):
    """mpn_person_crops_info rows (a structured array) -> the 'crop_info' dict of one image."""
    flags = rows['flags']
    return {'rect': np.ascontiguousarray(rows['rect']), 'placed': np.ascontiguousarray(rows['placed']),
            'empty': (flags & EMPTY) != 0, 'too_large': (flags & TOO_LARGE) != 0, 'clipped': (flags & CLIPPED) != 0}


class CropBuffers:
    """The device side of `mpn_person_crops` for b frames and b * max_boxes slots: descriptors (with their pinned staging),
    the crops [b * max_boxes, H, W, 3], the info block, the tap workspace and, with format='jpeg', a `JpegBatchEncoder`
    whose plan of b * max_boxes equal RGB images is placed once, here. The grids depend on (b, max_boxes, size) alone: the
    launch can be captured, and the graph follows whatever `place` uploads later and whatever the record holds."""

    def __init__(self, b, max_boxes, spec, device):
        import torch
        lib = _lib.lib()
        self.spec = check_spec(spec)
        self.b, self.max_boxes, self.slots = int(b), int(max_boxes), int(b) * int(max_boxes)
        height, width = spec.size
        work = lib.mpn_person_crops_workspace_bytes(self.b, self.max_boxes, height, width)
        info = lib.mpn_person_crops_info_bytes(self.b, self.max_boxes)
        if lib.mpn_person_crops_desc_bytes() != draw.DESC_WORDS * 4 or (info and info != self.slots * INFO.itemsize):
            raise _lib.MpnError("mpn_person_crops: the layout of the descriptors or the info rows is not the one this binding "
                                "was written against")
        if work == 0 or info == 0:
            raise ValueError(f"crops: {b} x {max_boxes} slots are more than mpn_person_crops takes in one launch "
                             f"(max_boxes <= {MAX_BOXES}, b * max_boxes <= 4096)")
        self.device = torch.device(device)
        self.desc_stage = torch.zeros((self.b, draw.DESC_WORDS), dtype=torch.int32).pin_memory()
        self.desc = torch.zeros((self.b, draw.DESC_WORDS), dtype=torch.int32, device=device)
        self.out = torch.empty(self.slots * spec.crop_bytes, dtype=torch.uint8, device=device)
        self.info = torch.empty(info, dtype=torch.uint8, device=device)
        self.work = torch.empty(work, dtype=torch.uint8, device=device)
        self.info_host = torch.zeros(info, dtype=torch.uint8).pin_memory()
        self.out_host = None
        self.encode = self.plan = None
        if spec.format == 'jpeg':
            self.plan = jpeg.EncodePlan([spec.size] * self.slots, [s * spec.crop_bytes for s in range(self.slots)], 3,
                                        spec.jpeg_quality, spec.jpeg_subsampling)
            self.encode = jpeg.JpegBatchEncoder(device)
            with torch.cuda.device(self.device):
                self.encode.reserve(self.slots, *self.plan.need)
                self.encode.upload(self.plan)
        else:
            self.out_host = torch.empty(self.slots * spec.crop_bytes, dtype=torch.uint8).pin_memory()

    def place(self, shapes, src_offsets):
        """This call's frames: the descriptors go to the device (one small copy, ordered before the launch on the stream)."""
        desc, _, _ = draw.layout(shapes, src_offsets)
        self.desc_stage.numpy()[...] = desc
        self.desc.copy_(self.desc_stage, non_blocking=True)

    def launch(self, sources, record):
        """sources: flat uint8 device tensor; record: mpn_pose_gather's (uint8 device tensor) -> the crops (and, with
        format='jpeg', their encode behind them on the same stream)."""
        spec = self.spec
        _lib.call("mpn_person_crops", _lib.ptr(sources), sources.numel(), _lib.ptr(self.desc), _lib.ptr(record), record.numel(),
                  self.b, self.max_boxes, spec.size[0], spec.size[1], spec.pad, FITS[spec.fit], spec.fill_word,
                  _lib.ptr(self.out), _lib.ptr(self.info), _lib.ptr(self.work), self.work.numel(), _lib.stream_ptr())
        if self.encode is not None:
            self.encode.launch(self.out)
        return self.out

    def fetch_info(self):
        """The fixed-size info block to pinned memory, asynchronously: the caller synchronises (with its record)."""
        self.info_host.copy_(self.info, non_blocking=True)

    def collect(self, counts):
        """Behind the caller's synchronise, which brought the info block: the first total = sum(counts) crops - exactly
        total * H * W * 3 bytes, or exactly the first total streams - in one more step, split by image: a list of
        (crops, crop_info) with crops a uint8 [n, H, W, 3] array or a list of n `bytes`."""
        import torch
        height, width = self.spec.size
        total = min(int(sum(int(c) for c in counts)), self.slots)
        info = self.info_host.numpy().view(INFO)[:total].copy()
        if self.encode is not None:
            files = self.encode.collect(self.plan, self.out, count=total) if total else []
        elif total:
            nb = total * self.spec.crop_bytes
            self.out_host[:nb].copy_(self.out[:nb], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            pixels = self.out_host.numpy()[:nb].reshape(total, height, width, 3).copy()
        out, s = [], 0
        for c in counts:
            e = min(s + int(c), total)
            if self.encode is not None:
                out.append((files[s:e], unpack_info(info[s:e])))
            elif total:
                out.append((pixels[s:e], unpack_info(info[s:e])))
            else:
                out.append((np.zeros((0, height, width, 3), np.uint8), unpack_info(info[s:e])))
            s = e
        return out


class PersonCropper:
    """`mpn_person_crops` for host frames and result dicts: one frame per call, buffers kept per (spec, capacity)."""

    def __init__(self, spec=None, device=None):
        self.spec = PersonCrops() if spec is None else check_spec(spec)
        self.device = _lib.current_device() if device is None else device
        self._buffers = {}

    def __call__(self, image, outputs):
        import torch
        from ..pose_metrics import fill_record
        image = np.asarray(image)
        if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8 or image.size == 0:
            raise ValueError(f"image must be uint8 [height, width, 3] (got {image.dtype} {image.shape})")
        h, w, _ = image.shape
        boxes = np.asarray(outputs['boxes'], np.float32).reshape(-1, 4)
        n = len(boxes)
        if n > self.spec.max_boxes:
            raise ValueError(f"person_crops: {n} persons, the PersonCrops was made for max_boxes = {self.spec.max_boxes}")
        capacity = 1 << max(int(image.size - 1).bit_length(), 12)
        if capacity not in self._buffers:
            self._buffers[capacity] = CropBuffers(1, self.spec.max_boxes, self.spec, self.device)
        buffers = self._buffers[capacity]
        record, counts = fill_record([{'boxes': boxes, 'scores': np.zeros(n, np.float32)}], 1, self.spec.max_boxes)
        with torch.cuda.device(self.device):
            sources = torch.zeros(capacity, dtype=torch.uint8, device=self.device)
            sources[:image.size].copy_(torch.from_numpy(np.ascontiguousarray(image).reshape(-1)))
            buffers.place([(h, w)], [0])
            buffers.launch(sources, torch.from_numpy(record).to(self.device))
            buffers.fetch_info()
            torch.cuda.current_stream(self.device).synchronize()
            return buffers.collect(counts)[0]


_croppers = {}


def person_crops(image, outputs, spec=None):
    """One uint8 [h, w, 3] host frame and its result dict ('boxes' [n, 4] normalised, as every predict method returns them) ->
    (crops, crop_info): what `Detector.predict_*(crops=spec)` returns as 'crops' and 'crop_info' for that frame, made by one
    mpn_person_crops on the device. spec: a `PersonCrops` (default: `PersonCrops()`)."""
    spec = PersonCrops() if spec is None else check_spec(spec)
    key = (spec, str(_lib.current_device()))
    if key not in _croppers:
        _croppers[key] = PersonCropper(spec)
    return _croppers[key](image, outputs)
