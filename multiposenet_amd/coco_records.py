"""COCO `person_keypoints_*.json` + an image directory -> the TFRecord shards the train scripts and `evaluate_pose
--val-dataset` read (the reference's data/create_tfrecords.py, without TensorFlow, pycocotools or OpenCV).

The pixel work - rasterising every person's segmentation, the loss and segmentation masks, the Lanczos4 reduction to quarter
size, threshold and bit packing - is one device call per batch of images (`CocoMaskRasterizer`, csrc/coco_masks.hip): only
vertices go up the link and only packed bits come back. The record rules (`apply_record_rules`, `to_example`) are host code.

DESIGN.md section 21 has the semantics; tests/coco_mask_ref.py is their definition. Equality with pycocotools' `annToMask` and
`cv2.resize` is the intent and has not been checked against the two libraries.
"""
import functools
import io
import json
import math
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .detector.input_pipeline import tfrecord

MAX_SIDE = 1024                 # MPN_COCO_MASKS_MAX_SIDE
DOWNSAMPLE = 4
MIN_NUM_KEYPOINTS = 2           # a person with fewer labelled keypoints, or a clipped box side below MIN_BOX_SIDE, is dropped:
MIN_BOX_SIDE = 5                # no box, no keypoints, and its mask is taken out of the loss
PART_DROPPED, PART_RLE = 1, 2   # MPN_COCO_PART_*
MAX_READERS = 16
_COEF_BITS = 11
_FLT_EPSILON = 1.1920928955078125e-07

_IMAGE_DESC = np.dtype([('plane_offset', '<i8'), ('packed_offset', '<i8'), ('full_offset', '<i8'),
                        ('h', '<i4'), ('w', '<i4'), ('tap_x', '<i4'), ('tap_y', '<i4')])
_PART_DESC = np.dtype([('offset', '<i8'), ('count', '<i4'), ('image', '<i4'), ('flags', '<i4'), ('reserved', '<i4')])
_TAP = np.dtype([('first', '<i4'), ('weights', '<i2', (8,))])


# ---------------------------------------------------------------- host tables
def rle_from_string(s):
    """COCO's compressed run-length string (maskApi rleFrString) -> a list of run lengths."""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts, p, n = [], 0, len(s)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise ValueError("compressed RLE: the string ends inside a number")
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        if not 0 <= x < (1 << 32):
            raise ValueError(f"compressed RLE: run length {x} is not a uint32")
        counts.append(x)
    return counts


def _lanczos4(x):
    """OpenCV's interpolateLanczos4: the eight float32 weights of the fraction x (float32)."""
    f32 = np.float32
    if x < f32(_FLT_EPSILON):
        return [f32(0), f32(0), f32(0), f32(1), f32(0), f32(0), f32(0), f32(0)]
    s45 = 0.70710678118654752440084436210485
    cs = ((1, 0), (-s45, -s45), (0, 1), (s45, -s45), (-1, 0), (s45, s45), (0, -1), (-s45, s45))
    y0 = -float(x + f32(3)) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    coeffs, total = [], f32(0)
    for i in range(8):
        y = -float(x + f32(3) - f32(i)) * math.pi * 0.25
        coeffs.append(f32((cs[i][0] * s0 + cs[i][1] * c0) / (y * y)))
        total = f32(total + coeffs[-1])
    total = f32(f32(1) / total)
    return [f32(c * total) for c in coeffs]


@functools.lru_cache(maxsize=256)
def lanczos_taps(src, dst):
    """One axis of OpenCV's resize(INTER_LANCZOS4) from `src` to `dst` pixels as mpn_coco_masks' tap entries: 'first' =
    floor of fx = (float)((d + .5) * scale - .5) with scale = 1 / (dst / src) in double, 'weights' = the eight Lanczos weights
    of the fraction as saturate_cast<short>(weight * 2048) (rounded half to even). Read-only, cached per (src, dst)."""
    scale = 1.0 / (float(dst) / float(src))
    taps = np.zeros(dst, _TAP)
    for d in range(dst):
        fx = np.float32((d + 0.5) * scale - 0.5)
        s = math.floor(float(fx))
        fx = np.float32(fx - np.float32(s))
        taps['first'][d] = s
        q = [int(np.rint(np.float32(c * np.float32(1 << _COEF_BITS)))) for c in _lanczos4(fx)]
        taps['weights'][d] = [max(-32768, min(32767, v)) for v in q]
    taps.setflags(write=False)
    return taps


def check_side(h, w):
    if not (1 <= int(h) <= MAX_SIDE and 1 <= int(w) <= MAX_SIDE):
        raise ValueError(f"an image of {h} x {w}: mpn_coco_masks takes sides of 1..{MAX_SIDE}")
    return int(h), int(w)


def mask_size(h, w):
    return -(-h // DOWNSAMPLE), -(-w // DOWNSAMPLE)


class _Batch:
    """The host tables of one call: descriptors, taps, vertices and runs in one byte block, every section 16-byte aligned."""

    def __init__(self, items, want_full):
        lib = _lib.lib()
        images = np.zeros(len(items), _IMAGE_DESC)
        parts, xy, runs, taps, tap_at = [], [], [], [], {}
        num_xy = num_runs = num_taps = 0
        plane_at = packed_at = full_at = 0
        self.sizes, self.max_side = [], 1

        def place(src, dst):
            nonlocal num_taps
            if (src, dst) not in tap_at:
                tap_at[(src, dst)] = num_taps
                taps.append(lanczos_taps(src, dst))
                num_taps += dst
            return tap_at[(src, dst)]

        for i, (h, w, annotations) in enumerate(items):
            h, w = check_side(h, w)
            mh, mw = mask_size(h, w)
            nbytes = lib.mpn_coco_masks_packed_bytes(h, w)
            images[i] = (plane_at, packed_at, full_at, h, w, place(w, mw), place(h, mh))
            self.sizes.append((h, w, packed_at, nbytes, full_at))
            self.max_side = max(self.max_side, h, w)
            plane_at += lib.mpn_coco_masks_plane_words(h, w)
            packed_at += (nbytes + 3) // 4 * 4
            full_at += h * w * 2 if want_full else 0
            for a in annotations:
                flag = PART_DROPPED if a['dropped'] else 0
                seg = a['segmentation']
                if isinstance(seg, dict):
                    counts = seg['counts']
                    if isinstance(counts, (str, bytes)):
                        counts = rle_from_string(counts)
                    r = np.asarray(counts, np.int64).reshape(-1)
                    if r.size and (r.min() < 0 or r.max() >= 1 << 32):
                        raise ValueError(f"image {i}: an RLE run length is not a uint32")
                    parts.append((num_runs, r.size, i, flag | PART_RLE, 0))
                    runs.append(r.astype(np.uint32))
                    num_runs += r.size
                    continue
                for poly in seg:
                    p = np.asarray(poly, np.float64).reshape(-1)
                    p = p[:p.size // 2 * 2]
                    if not np.all(np.isfinite(p)):
                        raise ValueError(f"image {i}: a polygon has a coordinate that is not finite")
                    px, py = p[0::2], p[1::2]
                    if p.size and (px.min() < -w or px.max() > 2 * w or py.min() < -h or py.max() > 2 * h):
                        raise ValueError(f"image {i} ({h} x {w}): a polygon vertex lies more than one image size outside the image")
                    parts.append((num_xy, p.size // 2, i, flag, 0))
                    xy.append(p)
                    num_xy += p.size
        self.num_images, self.num_parts = len(items), len(parts)
        self.num_xy, self.num_runs, self.num_taps = num_xy, num_runs, num_taps
        self.plane_bytes = max((plane_at * 4 + 15) // 16 * 16, 16)
        self.packed_bytes, self.full_bytes = max(packed_at, 4), max(full_at, 2)
        sections = [images, np.array(parts, _PART_DESC) if parts else np.zeros(0, _PART_DESC),
                    np.concatenate(xy) if xy else np.zeros(0, np.float64),
                    np.concatenate(runs) if runs else np.zeros(0, np.uint32), np.concatenate(taps)]
        self.at, size = [], 0
        for s in sections:
            self.at.append(size)
            size += (s.nbytes + 15) // 16 * 16
        self.nbytes = max(size, 16)
        self.sections = sections

    def write(self, host):
        """host: a uint8 array of at least `nbytes`."""
        for at, s in zip(self.at, self.sections):
            host[at:at + s.nbytes] = s.reshape(-1).view(np.uint8)


@_lib.device_guarded("rasterize", "upload", "launch")
class CocoMaskRasterizer:
    """`mpn_coco_masks` for host data: a pinned staging buffer and its device twin for the tables of a batch (one copy up),
    the workspace and the outputs on the device, and a pinned buffer the packed masks come back in. The buffers grow to the
    largest batch seen (powers of two) and are reused; a call takes at most `max_images` images."""

    def __init__(self, max_images=64, device=None):
        import torch
        if int(max_images) < 1:
            raise ValueError(f"max_images must be >= 1 (got {max_images})")
        lib = _lib.lib()
        if lib.mpn_coco_masks_image_desc_bytes() != _IMAGE_DESC.itemsize or lib.mpn_coco_masks_part_desc_bytes() != _PART_DESC.itemsize:
            raise _lib.MpnError("mpn_coco_masks: the descriptors are not the ones this binding was written against")
        self.max_images = int(max_images)
        self.device = torch.device(device) if device is not None else _lib.current_device()
        self._buffers = {}

    def _buffer(self, name, nbytes, pinned=False):
        import torch
        t = self._buffers.get(name)
        if t is None or t.numel() < nbytes:
            cap = 1 << max(int(nbytes) - 1, 4095).bit_length()
            t = torch.zeros(cap, dtype=torch.uint8).pin_memory() if pinned else torch.zeros(cap, dtype=torch.uint8, device=self.device)
            self._buffers[name] = t
        return t

    def upload(self, batch):
        """The tables of a `_Batch` go to the device: one pinned copy on the current stream."""
        stage = self._buffer('stage', batch.nbytes, pinned=True)
        self._tables = self._buffer('tables', batch.nbytes)
        batch.write(stage.numpy())
        self._tables[:batch.nbytes].copy_(stage[:batch.nbytes], non_blocking=True)

    def launch(self, batch, want_full=False):
        """mpn_coco_masks over the uploaded tables -> the device buffers (packed, full or None)."""
        work = self._buffer('work', batch.plane_bytes)
        packed = self._buffer('packed', batch.packed_bytes)
        full = self._buffer('full', batch.full_bytes) if want_full else None
        at = [_lib._P(self._tables.data_ptr() + a) for a in batch.at]
        _lib.call("mpn_coco_masks", at[0], batch.num_images, batch.max_side, at[1] if batch.num_parts else None, batch.num_parts,
                  at[2] if batch.num_xy else None, batch.num_xy, at[3] if batch.num_runs else None, batch.num_runs,
                  at[4], batch.num_taps, _lib.ptr(work), batch.plane_bytes, _lib.ptr(packed), batch.packed_bytes,
                  _lib.ptr(full), batch.full_bytes if want_full else 0, _lib.stream_ptr())
        return packed, full

    def rasterize(self, items, return_full=False):
        """items: [(h, w, annotations)], an annotation a dict with 'segmentation' (COCO's: a list of flat polygons, or a dict
        whose 'counts' is a list of run lengths or a compressed string) and 'dropped' (bool). Returns the packed masks, one
        uint8 array per image (`tfrecord.unpack_masks` reads them); with return_full=True also the list of uint8 [h, w, 2]
        arrays (loss mask, segmentation mask) at full resolution. Raises ValueError before any launch on a side above
        MAX_SIDE, a coordinate that is not finite and a vertex more than one image size outside the image."""
        items = list(items)
        if not 1 <= len(items) <= self.max_images:
            raise ValueError(f"a call takes 1..{self.max_images} images (got {len(items)})")
        batch = _Batch(items, return_full)
        self.upload(batch)
        packed, full = self.launch(batch, return_full)
        back = self._buffer('back', batch.packed_bytes, pinned=True)
        back[:batch.packed_bytes].copy_(packed[:batch.packed_bytes], non_blocking=True)
        full_host = full[:batch.full_bytes].cpu().numpy() if return_full else None
        import torch
        torch.cuda.current_stream().synchronize()
        host = back.numpy()
        out = [host[at:at + n].copy() for _, _, at, n, _ in batch.sizes]
        if not return_full:
            return out
        return out, [full_host[f:f + h * w * 2].reshape(h, w, 2).copy() for h, w, _, _, f in batch.sizes]


# ---------------------------------------------------------------- the record rules
def apply_record_rules(annotations, h, w):
    """COCO person annotations of one h x w image -> one dict per annotation, in order: 'dropped' (bool), 'segmentation', and
    for a kept person 'box' float64 (ymin, xmin, ymax, xmax) clipped to the image and 'keypoints' int64 [17, 3] = (y, x, v)
    clipped to [0, h - 1] and [0, w - 1]. A person is dropped when it has fewer than 2 labelled keypoints or a side of its
    clipped box is below 5 pixels; a dropped person has no box and masks the loss."""
    out = []
    for a in annotations:
        xmin, ymin, bw, bh = (float(v) for v in a['bbox'])
        xmax, ymax = xmin + bw, ymin + bh
        ymin, ymax = min(max(ymin, 0.0), float(h)), min(max(ymax, 0.0), float(h))
        xmin, xmax = min(max(xmin, 0.0), float(w)), min(max(xmax, 0.0), float(w))
        ymin, ymax = min(ymin, ymax), max(ymin, ymax)
        xmin, xmax = min(xmin, xmax), max(xmin, xmax)
        dropped = a['num_keypoints'] < MIN_NUM_KEYPOINTS or ymax - ymin < MIN_BOX_SIDE or xmax - xmin < MIN_BOX_SIDE
        person = {'dropped': bool(dropped), 'segmentation': a['segmentation']}
        if not dropped:
            points = np.array(a['keypoints'], dtype=np.int64).reshape(17, 3)
            x, y = np.clip(points[:, 0], 0, w - 1), np.clip(points[:, 1], 0, h - 1)
            person['box'] = (ymin, xmin, ymax, xmax)
            person['keypoints'] = np.stack([y, x, points[:, 2]], 1)
        out.append(person)
    return out


def read_image(path):
    """An image file -> (JPEG bytes, height, width), or None when it is not a JPEG. A grayscale JPEG is re-encoded as RGB by
    Pillow with its defaults; the size is the frame header's (`tfrecord.jpeg_shape`), no pixel is decoded otherwise."""
    with open(path, "rb") as f:
        data = f.read()
    try:
        h, w = tfrecord.jpeg_shape(data)
    except ValueError:
        return None
    if _jpeg_components(data) == 1:
        from PIL import Image
        with Image.open(io.BytesIO(data)) as im:
            out = io.BytesIO()
            im.convert("RGB").save(out, format="jpeg")
        data = out.getvalue()
        h, w = tfrecord.jpeg_shape(data)
    return data, h, w


def _jpeg_components(data):
    """The component count of the frame header that `tfrecord.jpeg_shape` found (1: grayscale)."""
    pos, n = 2, len(data)
    while pos + 4 <= n:
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
        elif m == 0x01 or 0xD0 <= m <= 0xD8:
            pos += 2
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return data[pos + 9] if pos + 9 < n else 0
        else:
            pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return 0


def to_example(jpeg_bytes, persons, packed_masks):
    """The serialized `tf.train.Example` of one image: `persons` as `apply_record_rules` returns them, `packed_masks` the
    image's packed masks from the rasteriser. None for an image without a kept person."""
    kept = [p for p in persons if not p['dropped']]
    if not kept:
        return None
    boxes = np.array([p['box'] for p in kept], np.float32)
    keypoints = np.stack([p['keypoints'] for p in kept]).astype(np.int64)
    return tfrecord.encode_example({'image': bytes(jpeg_bytes), 'num_persons': np.array([len(kept)], np.int64),
                                    'boxes': boxes.reshape(-1), 'keypoints': keypoints.reshape(-1),
                                    'masks': np.asarray(packed_masks, np.uint8).tobytes()})


def person_images(annotations_json):
    """-> [(file_name, annotations)] of the images that have person annotations, in ascending image id."""
    with open(annotations_json) as f:
        coco = json.load(f)
    person = {c['id'] for c in coco.get('categories', []) if c.get('name') == 'person'} or {1}
    by_image = {}
    for a in coco['annotations']:
        if a.get('category_id', 1) in person:
            by_image.setdefault(a['image_id'], []).append(a)
    names = {im['id']: im['file_name'] for im in coco['images']}
    return [(names[i], by_image[i]) for i in sorted(by_image) if i in names]


def write_shards(annotations_json, images_dir, out_dir, num_shards, seed=0, batch=64, rasterizer=None):
    """Writes `out_dir`/shard-%04d.tfrecords with ceil(n / num_shards) records each, n the number of images with person
    annotations, in an order shuffled by `seed`. An image that is not a JPEG or has no kept person is skipped.
    rasterizer: a callable [(h, w, persons)] -> packed masks (default: a `CocoMaskRasterizer` on the current device).
    Returns {'images', 'written', 'skipped', 'shards'}."""
    if int(num_shards) < 1 or int(batch) < 1:
        raise ValueError(f"num_shards and batch must be >= 1 (got {num_shards}, {batch})")
    entries = person_images(annotations_json)
    random.Random(seed).shuffle(entries)
    shard_size = max(1, math.ceil(len(entries) / int(num_shards)))
    if rasterizer is None:
        rasterizer = CocoMaskRasterizer(int(batch)).rasterize
    os.makedirs(out_dir, exist_ok=True)
    written = skipped = shards = in_shard = 0
    writer = None
    try:
        with ThreadPoolExecutor(max_workers=min(MAX_READERS, int(batch))) as pool:
            for s in range(0, len(entries), int(batch)):
                group = entries[s:s + int(batch)]
                files = pool.map(lambda e: read_image(os.path.join(images_dir, e[0])), group)
                todo = []
                for (name, annotations), image in zip(group, files):
                    if image is None:
                        skipped += 1
                        continue
                    data, h, w = image
                    persons = apply_record_rules(annotations, h, w)
                    if all(p['dropped'] for p in persons):
                        skipped += 1
                        continue
                    todo.append((data, h, w, persons))
                if not todo:
                    continue
                masks = rasterizer([(h, w, persons) for _, h, w, persons in todo])
                for (data, h, w, persons), packed in zip(todo, masks):
                    if writer is None:
                        writer = open(os.path.join(out_dir, 'shard-%04d.tfrecords' % shards), 'wb')
                    writer.write(tfrecord.frame_record(to_example(data, persons, packed)))
                    written += 1
                    in_shard += 1
                    if in_shard == shard_size:
                        writer.close()
                        writer, in_shard, shards = None, 0, shards + 1
    finally:
        if writer is not None:
            writer.close()
            shards += 1
    return {'images': len(entries), 'written': written, 'skipped': skipped, 'shards': shards}
