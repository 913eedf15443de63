"""`PoseResidualNetworkPipeline` - the reference's PRN input pipeline (detector/input_pipeline/prn_pipeline.py:9-156) with
its per-pixel work on the GPU.

    pipeline = PoseResidualNetworkPipeline(filenames, is_training=True, batch_size=32, max_keypoints=7)
    for crops, labels in pipeline.dataset: ...        # f32 [b, 56, 36, 17] device tensors, the input of prn_model.model_fn

A PRN example is a pure function of annotations - (the kept people of its source image, the person, flip) - so no pixel is
ever read: the JPEG of a record is not decoded, only its frame header is scanned for the size (`jpeg_shape`,
tf.image.extract_jpeg_shape at :63). Per batch:

  host     references to annotations travel through the reference's order - per-epoch shard shuffle, record shuffle buffer,
           per-person unbatch, person shuffle buffer, batches of `batch_size`, endless (:24-44); evaluation is one pass in
           record order that ENDS ON THE PARTIAL BATCH (`dataset.repeat(1).batch(b)`). Then, per batch, one uniform draw
           < 0.5 per person decides the flip (:196), and the batch's tables (people of its distinct source images,
           image sizes, one (image, person, flip) descriptor per example) go into a PINNED staging slot and are copied to
           the device on a side stream.
  device   on the CURRENT stream, ordered after the copy: `mpn_prn_examples` renders crops and labels directly into the
           batch (include/mpn.h, L3) - bit-identical to get_heatmaps + tf.image.crop_and_resize + the label maps + the flip.

Curriculum (:78-89): with `max_keypoints` only persons with at most that many visible keypoints are kept, and the heatmap
of an image is rendered from the KEPT persons only (the filter precedes get_heatmaps).

Skipped (the reference assumes neither occurs - data/create_tfrecords.py:97-122 writes neither -, so this only matters for
foreign data): records with num_persons == 0 and images without a kept person contribute nothing; persons whose box has
non-positive height or width are dropped (the reference divides by zero there).

Annotation cache. A training run makes about 40 passes over the data and builds 15 pipelines (one per curriculum stage);
rereading ~150 KB of JPEG per record for ~250 bytes of annotations each time would make the reader the bound stage. The
first read of a file keeps its parsed annotations (int32 keypoints, f32 boxes, int32 sizes) in an `AnnotationCache`; every
later pass, and every pipeline given the same cache (`annotations=`), is served from memory and opens no file. Measured
on the toy shards of tools/make_toy_tfrecords.py (2.5 persons per record): 226 bytes per person (220 of keypoints and box,
the rest the per-record size and offset), i.e. tens of MB for the COCO person set.

Buffers: with `buffers=(crops, labels)` ([batch_size, 56, 36, 17] f32 device tensors) every batch is written into them, so
a yielded batch is valid until the next one is requested. Otherwise the pipeline alternates between two owned sets: a
batch stays valid until the next-but-one is requested. A partial batch is the leading slice of its set.

`filenames` may also be an in-memory sequence of examples, dicts with 'boxes' (f32 [P,4] absolute), 'keypoints'
(int [P,17,3]) and either 'image' (an [H,W,...] array, only its shape is used) or 'height' / 'width'.
Single process: `PoseResidualNet` has no data-parallel path, so there is no rank sharding. Randomness follows the
reference's distributions, not TensorFlow's streams.
"""
import collections
import os

import numpy as np
import torch

from ... import _lib
from ..constants import DOWNSAMPLE, NUM_KEYPOINTS, SHUFFLE_BUFFER_SIZE
from .tfrecord import jpeg_shape, parse_example, read_records

CROP_SIZE = (56, 36)    # height and width (prn_pipeline.py:6-7)

# == mpn_prn_example_desc (include/mpn.h)
DESC_DTYPE = np.dtype([("image", "<i4"), ("person", "<i4"), ("flip", "<i4"), ("reserved", "<i4")])
assert DESC_DTYPE.itemsize == 16


def _align(n, a=256):
    return (n + a - 1) // a * a


class _FileAnnotations:
    """The annotations of one file, concatenated: persons of record k are first[k] .. first[k+1]-1."""
    __slots__ = ("keypoints", "boxes", "first", "heights", "widths")

    def __init__(self, records):
        kps = [r[0] for r in records]
        self.keypoints = (np.concatenate(kps) if kps else np.zeros((0, NUM_KEYPOINTS, 3))).astype(np.int32)
        self.boxes = (np.concatenate([r[1] for r in records]) if kps else np.zeros((0, 4))).astype(np.float32)
        self.first = np.cumsum([0] + [len(k) for k in kps]).astype(np.int64)
        self.heights = np.array([r[2] for r in records], np.int32)
        self.widths = np.array([r[3] for r in records], np.int32)

    def __len__(self):
        return len(self.heights)

    @property
    def nbytes(self):
        return sum(getattr(self, n).nbytes for n in self.__slots__)


def parse_annotations(data):
    """One serialized record (prn_pipeline.py:53-76) -> (keypoints int32 [P,17,3], boxes f32 [P,4], height, width).
    The image is not decoded."""
    f = parse_example(data)
    for k in ("image", "num_persons"):
        if f.get(k) is None:
            raise ValueError(f"record has no '{k}' feature")
    p = int(f["num_persons"][0])
    boxes, kps = f.get("boxes"), f.get("keypoints")
    boxes = np.zeros(0, np.float32) if boxes is None else boxes
    kps = np.zeros(0, np.int64) if kps is None else kps
    if boxes.size != p * 4 or kps.size != p * NUM_KEYPOINTS * 3:
        raise ValueError(f"record: num_persons={p} but {boxes.size} box values and {kps.size} keypoint values")
    height, width = jpeg_shape(f["image"][0])
    return kps.reshape(p, NUM_KEYPOINTS, 3).astype(np.int32), boxes.reshape(p, 4).astype(np.float32), height, width


class AnnotationCache:
    """Parsed annotations per file, filled on a file's first read and shared between pipelines (`annotations=`)."""

    def __init__(self):
        self.files = {}

    def load(self, path):
        ann = self.files.get(path)
        if ann is None:
            ann = self.files[path] = _FileAnnotations([parse_annotations(rec) for rec in read_records(path)])
        return ann

    @property
    def nbytes(self):
        return sum(a.nbytes for a in self.files.values())

    @property
    def num_persons(self):
        return sum(len(a.boxes) for a in self.files.values())


class _Image:
    """The kept people of one source image. `source` = (unit, record index in the unit), `persons` = the indices of the
    kept people among the record's."""
    __slots__ = ("keypoints", "boxes", "height", "width", "source", "persons")

    def __init__(self, keypoints, boxes, height, width, source, persons):
        self.keypoints, self.boxes, self.height, self.width = keypoints, boxes, int(height), int(width)
        self.source, self.persons = source, persons


class _Slot:
    """Pinned host staging + device copy of one batch's tables."""

    def __init__(self, device):
        self.device = device
        self.host = self.dev = None
        self.copied = torch.cuda.Event()
        self.consumed = None

    def reserve(self, nbytes):
        if self.host is None or self.host.numel() < nbytes:
            if self.dev is not None:
                torch.cuda.synchronize(self.device)   # (rare) growth: no queued copy or launch still uses the old buffers
            n = _align(max(nbytes, 16) * 5 // 4)
            self.host = torch.empty(n, dtype=torch.uint8).pin_memory()
            self.dev = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self.host.numpy()


class PoseResidualNetworkPipeline:
    def __init__(self, filenames, is_training, batch_size, max_keypoints=None, device=None, seed=0,
                 shuffle_buffer_size=SHUFFLE_BUFFER_SIZE, buffers=None, annotations=None, depth=2):
        """filenames: paths of TFRecord files, or a sequence of in-memory examples. max_keypoints: an integer or None
        (the curriculum filter). annotations: an `AnnotationCache` shared with other pipelines over the same files."""
        if not len(filenames):
            raise ValueError("PoseResidualNetworkPipeline: no input files")
        if depth < 2:
            raise ValueError("depth >= 2: one slot is copied while the next one is filled")
        self.is_training = bool(is_training)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.max_keypoints = None if max_keypoints is None else int(max_keypoints)
        self.seed = int(seed)
        self.shuffle_buffer_size = max(1, int(shuffle_buffer_size))
        self.depth = int(depth)
        self.device = device
        self.buffers = buffers
        self.annotations = annotations if annotations is not None else AnnotationCache()
        in_memory = not isinstance(filenames[0], (str, bytes, os.PathLike))
        self._examples = list(filenames) if in_memory else None
        self._files = None if in_memory else [os.fspath(f) for f in filenames]
        self._kept = {}      # unit -> [_Image]: this pipeline's filter applied to the unit's records, once

    def generators(self):
        """(shuffling, flip) generators: two streams of one seed sequence, so a seed fixes the batches."""
        a, b = np.random.SeedSequence([self.seed]).spawn(2)
        return np.random.default_rng(a), np.random.default_rng(b)

    # ---------------------------------------------------------------- records
    def _filter(self, keypoints, boxes, height, width, source):
        """prn_pipeline.py:78-89 plus the skips of the module docstring; None when nobody is kept."""
        if len(boxes) == 0:
            return None
        if height < 2 or width < 2:
            raise ValueError(f"record {source}: image size {height}x{width} (both must be >= 2)")
        good = (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])
        if self.max_keypoints is not None:
            good &= (keypoints[:, :, 2] > 0).sum(axis=1) <= self.max_keypoints
        persons = np.flatnonzero(good)
        if persons.size == 0:
            return None
        return _Image(np.ascontiguousarray(keypoints[persons]), np.ascontiguousarray(boxes[persons]), height, width,
                      source, persons)

    def _unit_images(self, u):
        kept = self._kept.get(u)
        if kept is not None:
            return kept
        kept = []
        if self._examples is not None:
            ex = self._examples[u]
            p = np.asarray(ex["boxes"]).size // 4
            if "image" in ex and ex["image"] is not None and not isinstance(ex["image"], (bytes, bytearray, memoryview)):
                h, w = np.asarray(ex["image"]).shape[:2]
            elif "height" in ex and "width" in ex:
                h, w = int(ex["height"]), int(ex["width"])
            else:
                h, w = jpeg_shape(ex["image"])
            img = self._filter(np.asarray(ex["keypoints"]).astype(np.int32).reshape(p, NUM_KEYPOINTS, 3),
                               np.asarray(ex["boxes"], np.float32).reshape(p, 4), h, w, (u, 0))
            if img is not None:
                kept.append(img)
        else:
            ann = self.annotations.load(u)
            for k in range(len(ann)):
                a, b = int(ann.first[k]), int(ann.first[k + 1])
                img = self._filter(ann.keypoints[a:b], ann.boxes[a:b], int(ann.heights[k]), int(ann.widths[k]), (u, k))
                if img is not None:
                    kept.append(img)
        self._kept[u] = kept
        return kept

    def _images(self, rng):
        """Kept images in the order the persons are drawn from."""
        units = list(range(len(self._examples))) if self._examples is not None else list(self._files)

        def one_pass():
            order = units
            if self.is_training:
                order = [units[i] for i in rng.permutation(len(units))]        # shard shuffle (:26-28)
            for u in order:
                yield from self._unit_images(u)

        if not self.is_training:
            yield from one_pass()
            return

        def stream():
            while True:
                n = 0
                for img in one_pass():
                    n += 1
                    yield img
                if n == 0:
                    raise ValueError("PoseResidualNetworkPipeline: no person is left after the filters "
                                     f"(max_keypoints={self.max_keypoints})")
        yield from _shuffled(stream(), self.shuffle_buffer_size, rng)       # record shuffle buffer (:33-34)

    def _persons(self, rng):
        """(image, person) references: the unbatch (:38) and, for training, the person shuffle buffer (:40-41)."""
        persons = ((img, k) for img in self._images(rng) for k in range(len(img.boxes)))
        if self.is_training:
            return _shuffled(persons, self.shuffle_buffer_size, rng)
        return persons

    # ---------------------------------------------------------------- host sampling
    def sample(self, rng, items):
        """The host-side tables of one batch of (image, person) references, flips drawn in batch order from `rng`
        (None: no flip). Returns a dict: 'keypoints' int32 [Q,17,3] and 'boxes' f32 [Q,4] (the kept people of the batch's
        R distinct source images, concatenated), 'first_person' int32 [R+1], 'width', 'height' int32 [R], 'examples'
        DESC_DTYPE [N] (image r, GLOBAL person q, flip), 'sources' (the R images' (unit, record) ids) and 'persons' (per
        image, the indices of its kept people among the record's)."""
        images, index = [], {}
        descs = np.zeros(len(items), DESC_DTYPE)
        first = [0]
        for n, (img, k) in enumerate(items):
            r = index.get(id(img))
            if r is None:
                r = index[id(img)] = len(images)
                images.append(img)
                first.append(first[-1] + len(img.boxes))
            flip = bool(rng.random() < 0.5) if (rng is not None and self.is_training) else False   # (:196)
            descs[n] = (r, first[r] + k, int(flip), 0)
        return {"keypoints": np.concatenate([i.keypoints for i in images]).astype(np.int32),
                "boxes": np.concatenate([i.boxes for i in images]).astype(np.float32),
                "first_person": np.array(first, np.int32),
                "width": np.array([i.width for i in images], np.int32),
                "height": np.array([i.height for i in images], np.int32),
                "examples": descs,
                "sources": [i.source for i in images], "persons": [i.persons for i in images]}

    def samples(self):
        """Generator of the `sample` tables of every batch, in the order `batches` yields them (no device needed)."""
        shuffle_rng, rng = self.generators()
        items = []
        for item in self._persons(shuffle_rng):
            items.append(item)
            if len(items) == self.batch_size:
                yield self.sample(rng, items)
                items = []
        if items:                                   # evaluation ends on the partial batch (training never ends)
            yield self.sample(rng, items)

    # ---------------------------------------------------------------- device
    def _outputs(self, n):
        if self.buffers is not None:
            crops, labels = self.buffers
            want = (self.batch_size,) + CROP_SIZE + (NUM_KEYPOINTS,)
            if tuple(crops.shape) != want or tuple(labels.shape) != want:
                raise ValueError(f"buffers hold {tuple(crops.shape)} / {tuple(labels.shape)}, a batch is {want}")
        else:
            if self._owned is None:
                shape = (self.batch_size,) + CROP_SIZE + (NUM_KEYPOINTS,)
                self._owned = [tuple(torch.empty(shape, dtype=torch.float32, device=self.device) for _ in range(2))
                               for _ in range(2)]
            self._turn ^= 1
            crops, labels = self._owned[self._turn]
        return crops[:n], labels[:n]

    def _launch(self, slot, tables):
        kp, bx, ex = tables["keypoints"], tables["boxes"], tables["examples"]
        N, Q, R = len(ex), len(bx), len(tables["width"])
        ex_off = 0
        kp_off = ex_off + _align(ex.nbytes)
        bx_off = kp_off + _align(kp.nbytes)
        fp_off = bx_off + _align(bx.nbytes)
        w_off = fp_off + _align((R + 1) * 4)
        h_off = w_off + _align(R * 4)
        total = h_off + _align(R * 4)
        slot.copied.synchronize()     # a slot's pinned array may be rewritten only once its previous copy has left it
        meta = slot.reserve(total)
        for off, a in ((ex_off, ex), (kp_off, kp), (bx_off, bx), (fp_off, tables["first_person"]),
                       (w_off, tables["width"]), (h_off, tables["height"])):
            meta[off:off + a.nbytes] = a.view(np.uint8).reshape(-1)
        main = torch.cuda.current_stream(self.device)
        cs = self._copy_stream
        if slot.consumed is not None:
            cs.wait_event(slot.consumed)            # the launch that read this slot's device copy has done so
        with torch.cuda.stream(cs):
            slot.dev[:total].copy_(slot.host[:total], non_blocking=True)
            slot.copied.record(cs)
        main.wait_event(slot.copied)
        need = _lib.lib().mpn_prn_examples_workspace_bytes(Q)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(_align(need * 5 // 4), dtype=torch.uint8, device=self.device)
        crops, labels = self._outputs(N)
        base = slot.dev.data_ptr()
        P = _lib._P
        _lib.call("mpn_prn_examples", P(base + kp_off), P(base + bx_off), Q, P(base + fp_off), P(base + w_off),
                  P(base + h_off), R, P(base + ex_off), N, CROP_SIZE[0], CROP_SIZE[1], DOWNSAMPLE, _lib.ptr(crops),
                  _lib.ptr(labels), _lib.ptr(self._workspace), self._workspace.numel(), _lib.stream_ptr())
        ev = torch.cuda.Event()
        ev.record(main)
        slot.consumed = ev
        return crops, labels

    def batches(self):
        """Generator of (crops, labels); endless for training, one pass ending on the partial batch for evaluation."""
        self.device = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._owned, self._turn, self._workspace = None, 0, None
        slots = collections.deque(_Slot(self.device) for _ in range(self.depth))
        with torch.cuda.device(self.device):
            for tables in self.samples():
                slot = slots[0]
                slots.rotate(-1)
                yield self._launch(slot, tables)

    @property
    def dataset(self):
        return self.batches()

    def __iter__(self):
        return self.batches()


def _shuffled(stream, size, rng):
    """tf.data's shuffle over an endless stream: fill a buffer of `size`, then swap each arrival with a random slot."""
    buf = []
    for item in stream:
        if len(buf) < size:
            buf.append(item)
            continue
        i = int(rng.integers(len(buf)))
        buf[i], item = item, buf[i]
        yield item
