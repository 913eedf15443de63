"""`KeypointPipeline` - the reference's input pipeline (detector/input_pipeline/keypoints_detector_pipeline.py:10-63) with
its pixels on the GPU.

    pipeline = KeypointPipeline(filenames, is_training=True, params=params)
    for features, labels in pipeline.dataset: ...

Per batch:
  host     read records (per-epoch shard shuffle, record shuffle buffer, repeat), parse + JPEG decode on a pool of
           NUM_PARALLEL_CALLS threads, then - in record order, from the pipeline's seeded generator - every random decision,
           box and keypoint (keypoint_augment.py); the decoded uint8 sources, packed masks and per-image descriptors go
           into a PINNED staging slot (at least two; a slot is refilled only after its copy has completed) and are
           copied to the device on a side stream.
  device   on the CURRENT stream, ordered after the copy: `mpn_keypoint_augment` (images + masks) and `HeatmapRenderer`
           (heatmaps), so a batch is written after the work already queued there - e.g. the step that read the last one.

Yields (features, labels) of device tensors in the contract of keypoints_detector_pipeline.py:104-110:
{'images': f32 [B,H,W,3]}, {'heatmaps': f32 [B,H/4,W/4,17], 'loss_masks', 'segmentation_masks': f32 [B,H/4,W/4],
'num_boxes': int32 [B]}. `num_boxes` may be 0 after pruning (the loss normalises by num_boxes + 1, keypoints_model.py:177).

Buffers: with `buffers=(features, labels)` (e.g. `Trainer.input_buffers(...)`) every batch is written into them, so a
yielded batch is valid until the next one is requested. Otherwise the pipeline alternates between two owned buffer sets:
a batch stays valid until the next-but-one is requested. Evaluation batches (batch size 1, size from
`resize_keeping_aspect_ratio`) get buffers per distinct image size.

`decode='device'` (default 'host') moves the pixel half of the JPEG decode to the device: the pool runs only the marker scan and
the Huffman decode (inference/jpeg.py), the coefficients are copied on the side stream and `mpn_jpeg_decode` writes the
uint8 sources there, byte for byte what PIL decodes - so a seed gives the same batches in both modes. Progressive and Adobe
CMYK files have all their scans decoded on the pool (`mpn_jpeg_scans_decode`); streams the device path does not support
(arithmetic coding, YCCK, ...) are decoded by PIL per image, inside the same batch.

`filenames` may also be an in-memory sequence of decoded examples, dicts with 'image' (uint8 [H,W,3]), 'boxes'
(f32 [P,4] absolute), 'keypoints' (int [P,17,3]) and 'masks' (np.packbits bytes of [ceil(H/4), ceil(W/4), 2]) - no PIL is
needed for those. Randomness follows the reference's distributions, not TensorFlow's streams (keypoint_augment.py).
"""
import collections
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import _lib
from ...inference import jpeg
from ..constants import DIVISOR, DOWNSAMPLE, NUM_KEYPOINTS, NUM_PARALLEL_CALLS, SHUFFLE_BUFFER_SIZE
from . import keypoint_augment as ka
from .heatmap_creation import HeatmapRenderer
from .tfrecord import decode_jpeg, decode_keypoint_example, read_records


DECODE_MODES = ('host', 'device')


def check_decode_mode(decode):
    if decode not in DECODE_MODES:
        raise ValueError(f"decode must be one of {DECODE_MODES} (got {decode!r})")
    return decode


def _align(n, a=256):
    return (n + a - 1) // a * a


class _Slot:
    """Pinned host staging + device copy of one batch's sources, masks, descriptors and labels."""

    def __init__(self, device):
        self.device = device
        self.host, self.dev = {}, {}
        self.copied = torch.cuda.Event()
        self.consumed = None
        self.jpeg = None                     # decode='device': this slot's JpegBatchDecoder (its own staging)

    def reserve(self, name, nbytes):
        if name not in self.host or self.host[name].numel() < nbytes:
            if name in self.dev:
                torch.cuda.synchronize(self.device)   # (rare) growth: no queued copy or launch still uses the old buffers
            n = _align(max(nbytes, 16) * 5 // 4)
            self.host[name] = torch.empty(n, dtype=torch.uint8).pin_memory()
            self.dev[name] = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self.host[name].numpy()


class KeypointPipeline:
    def __init__(self, filenames, is_training, params, device=None, buffers=None, num_threads=NUM_PARALLEL_CALLS,
                 depth=2, decode='host', entropy='host'):
        """filenames: paths of TFRecord files, or a sequence of decoded examples. params: 'batch_size', 'image_size'
        (width, height) for training, 'min_dimension' for evaluation; optional 'seed' (default 0) and
        'shuffle_buffer_size' (default SHUFFLE_BUFFER_SIZE). Under WORLD_SIZE > 1 rank r reads shards i with
        i % world == r (records i % world == r when there are fewer shards than ranks). decode: 'host' (PIL on the
        thread pool) or 'device' (Huffman decode on the pool, inverse DCT and colour on the device). entropy (with
        decode='device'): 'host', or 'device' - the pool only parses headers, the file's bytes are copied and the Huffman decode
        runs on the device too (mpn_jpeg_entropy_decode_device; an image it cannot settle falls back to the host decode)."""
        self.decode = check_decode_mode(decode)
        self.entropy = jpeg.check_entropy_mode(entropy)
        if self.entropy == 'device' and self.decode != 'device':
            raise ValueError("entropy='device' needs decode='device'")
        self.is_training = bool(is_training)
        if self.is_training:
            self.batch_size = int(params["batch_size"])
            width, height = params["image_size"]                      # (:33-36)
            if height % DIVISOR or width % DIVISOR:
                raise ValueError(f"image_size must be multiples of {DIVISOR}")
            self.image_size = (int(height), int(width))
        else:
            self.batch_size = 1
            self.min_dimension = int(params["min_dimension"])
            if self.min_dimension % DIVISOR:
                raise ValueError(f"min_dimension must be a multiple of {DIVISOR}")
        if depth < 2:
            raise ValueError("depth >= 2: one slot is copied while the next one is filled")
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.seed = int(params.get("seed", 0))
        self.shuffle_buffer_size = int(params.get("shuffle_buffer_size", SHUFFLE_BUFFER_SIZE))
        self.num_threads = max(1, int(num_threads))
        self.depth = int(depth)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.buffers = buffers
        in_memory = not (len(filenames) and isinstance(filenames[0], (str, bytes, os.PathLike)))
        self._examples = list(filenames) if in_memory else None
        self._files = None if in_memory else [os.fspath(f) for f in filenames]
        if not len(filenames):
            raise ValueError("KeypointPipeline: no input files")

    def generators(self):
        """(record shuffling, augmentation) generators: two streams of one seed sequence (params['seed'], rank), so the
        augmentation draws do not depend on how far ahead the records are read."""
        a, b = np.random.SeedSequence([self.seed, self.rank]).spawn(2)
        return np.random.default_rng(a), np.random.default_rng(b)

    # ---------------------------------------------------------------- records
    def _shard_items(self, items):
        return [x for i, x in enumerate(items) if i % self.world == self.rank]

    def _records(self, rng):
        """Raw records (bytes, or in-memory example dicts) in the order the batches consume them."""
        if self._examples is not None:
            units, stride_records = self._shard_items(range(len(self._examples))), False
        elif len(self._files) >= self.world:
            units, stride_records = self._shard_items(self._files), False
        else:
            units, stride_records = list(self._files), True

        def one_pass():
            order = list(units)
            if self.is_training:
                order = [order[i] for i in rng.permutation(len(order))]        # shard shuffle (:44-46)
            k = 0
            for u in order:
                it = [self._examples[u]] if self._examples is not None else read_records(u)
                for rec in it:
                    if not stride_records or k % self.world == self.rank:
                        yield rec
                    k += 1

        def stream():
            while True:
                yield from one_pass()
                if not self.is_training:
                    return
        if not self.is_training:
            yield from stream()
            return
        buf = []                                                            # record shuffle buffer (:51-52)
        for rec in stream():
            if len(buf) < self.shuffle_buffer_size:
                buf.append(rec)
                continue
            i = int(rng.integers(len(buf)))
            buf[i], rec = rec, buf[i]
            yield rec

    @staticmethod
    def _decode(rec, device=False, entropy='host'):
        """device: a JPEG stays coefficients (jpeg.Coefficients, which has the image's .shape; a jpeg.Scan with
        entropy='device') when the device path supports its stream."""
        if isinstance(rec, (bytes, bytearray, memoryview)):
            ex = decode_keypoint_example(rec, decode_image=not device)
        else:
            ex = dict(rec)
        img = ex["image"]
        if isinstance(img, (bytes, bytearray, memoryview)):
            img = jpeg.prepare(img, entropy, extended=True) if device else decode_jpeg(img)
        if not isinstance(img, (jpeg.Coefficients, jpeg.Scan)):
            img = np.ascontiguousarray(img, dtype=np.uint8)
            if img.ndim != 3 or img.shape[2] != 3:
                raise ValueError(f"image must be uint8 [H,W,3], got {img.shape}")
        p = np.asarray(ex["boxes"]).size // 4
        return {"image": img, "boxes": np.asarray(ex["boxes"], np.float32).reshape(p, 4),
                "keypoints": np.asarray(ex["keypoints"]).astype(np.int32).reshape(p, NUM_KEYPOINTS, 3),
                "masks": np.frombuffer(bytes(ex["masks"]), np.uint8) if not isinstance(ex["masks"], np.ndarray)
                else ex["masks"].astype(np.uint8).reshape(-1)}

    # ---------------------------------------------------------------- host sampling
    def sample(self, rng, examples):
        """Descriptors (offsets filled), boxes and keypoints of one batch of decoded examples, drawn in record order.
        Returns (descs, people, (H, W), src_bytes, mask_bytes)."""
        descs = np.zeros(len(examples), ka.DESC_DTYPE)
        people = []
        so = mo = 0
        size = None
        for i, ex in enumerate(examples):
            h, w = ex["image"].shape[:2]
            mh, mw = ka.mask_size(h, w)
            nbits = (mh * mw * 2 + 7) // 8
            if ex["masks"].size < nbits:
                raise ValueError(f"masks of a {h}x{w} image need {nbits} packed bytes, got {ex['masks'].size}")
            if self.is_training:
                d, boxes, kp = ka.sample_training(rng, h, w, ex["boxes"], ex["keypoints"], self.image_size)
                size = self.image_size
            else:
                d, boxes, kp, size = ka.sample_evaluation(h, w, ex["boxes"], ex["keypoints"], self.min_dimension)
            d["src_offset"], d["mask_offset"] = so, mo
            descs[i] = d
            so += _align(h * w * 3, 16)
            mo += _align(nbits, 16)
            people.append((boxes, kp))
        return descs, people, size, so, mo

    # ---------------------------------------------------------------- device
    def _outputs(self, H, W):
        if self.buffers is not None:
            feats, labels = self.buffers
            if tuple(feats["images"].shape) != (self.batch_size, H, W, 3):
                raise ValueError(f"buffers hold images {tuple(feats['images'].shape)}, batch is {(self.batch_size, H, W, 3)}")
            return feats, labels
        key = (H, W)
        sets = self._owned.get(key)
        if sets is None:
            B, h, w = self.batch_size, H // DOWNSAMPLE, W // DOWNSAMPLE
            dev = self.device

            def one():
                return ({"images": torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)},
                        {"heatmaps": torch.empty((B, h, w, NUM_KEYPOINTS), dtype=torch.float32, device=dev),
                         "loss_masks": torch.empty((B, h, w), dtype=torch.float32, device=dev),
                         "segmentation_masks": torch.empty((B, h, w), dtype=torch.float32, device=dev),
                         "num_boxes": torch.empty((B,), dtype=torch.int32, device=dev)})
            sets = self._owned[key] = [one(), one()]
        self._turn ^= 1
        return sets[self._turn]

    def _renderer(self, H, W):
        key = (H, W)
        if key not in self._renderers:
            self._renderers[key] = HeatmapRenderer(self.batch_size, W, H, DOWNSAMPLE, device=self.device)
        return self._renderers[key]

    def _launch(self, slot, descs, people, size, src_total, mask_total, examples):
        H, W = size
        B = len(descs)
        # a slot's pinned arrays may be rewritten only once its previous copy has left them
        slot.copied.synchronize()
        src = slot.reserve("src", src_total)
        msk = slot.reserve("masks", mask_total)
        for d, ex in zip(descs, examples):
            if self.decode == 'host':
                so, n = int(d["src_offset"]), ex["image"].size
                src[so:so + n] = ex["image"].reshape(-1)
            mo, nb = int(d["mask_offset"]), (int(d["mask_h"]) * int(d["mask_w"]) * 2 + 7) // 8
            msk[mo:mo + nb] = ex["masks"][:nb]
        ka.check_descriptors(descs, src_total, mask_total, H, W)
        counts = np.array([0] + [len(b) for b, _ in people], np.int64)
        P = int(counts.sum())
        desc_bytes = descs.nbytes
        kp_off = _align(desc_bytes)
        bx_off = kp_off + _align(P * NUM_KEYPOINTS * 3 * 4)
        fp_off = bx_off + _align(P * 16)
        nb_off = fp_off + _align((B + 1) * 4)
        meta = slot.reserve("meta", nb_off + _align(B * 4))
        meta[:desc_bytes] = descs.view(np.uint8)
        if P:
            meta[kp_off:kp_off + P * 204] = np.concatenate([k for _, k in people]).astype(np.int32).view(np.uint8).reshape(-1)
            meta[bx_off:bx_off + P * 16] = np.concatenate([b for b, _ in people]).astype(np.float32).view(np.uint8).reshape(-1)
        meta[fp_off:fp_off + (B + 1) * 4] = np.cumsum(counts).astype(np.int32).view(np.uint8)
        meta[nb_off:nb_off + B * 4] = counts[1:].astype(np.int32).view(np.uint8)

        main = torch.cuda.current_stream(self.device)
        cs = self._copy_stream
        if slot.consumed is not None:
            cs.wait_event(slot.consumed)            # the launch that read this slot's device copy has done so
        with torch.cuda.stream(cs):
            for name, n in (("src", src_total), ("masks", mask_total), ("meta", nb_off + B * 4)):
                if name != "src" or self.decode == 'host':
                    slot.dev[name][:max(n, 1)].copy_(slot.host[name][:max(n, 1)], non_blocking=True)
            if self.decode == 'device':
                self._decode_sources(slot, descs, examples, cs)
            slot.copied.record(cs)
        main.wait_event(slot.copied)
        feats, labels = self._outputs(H, W)
        dm = slot.dev["meta"]
        _lib.call("mpn_keypoint_augment", _lib.ptr(slot.dev["src"]), _lib.ptr(slot.dev["masks"]), _lib.ptr(dm), B, H, W,
                  _lib.ptr(feats["images"]), _lib.ptr(labels["loss_masks"]), _lib.ptr(labels["segmentation_masks"]),
                  _lib.stream_ptr())
        kp = dm[kp_off:kp_off + P * 204].view(torch.int32).view(P, NUM_KEYPOINTS, 3)
        bx = dm[bx_off:bx_off + P * 16].view(torch.float32).view(P, 4)
        fp = dm[fp_off:fp_off + (B + 1) * 4].view(torch.int32)
        self._renderer(H, W)(kp, bx, fp, out=labels["heatmaps"])
        labels["num_boxes"].copy_(dm[nb_off:nb_off + B * 4].view(torch.int32))
        ev = torch.cuda.Event()
        ev.record(main)
        slot.consumed = ev
        return feats, labels

    def _decode_sources(self, slot, descs, examples, stream):
        """decode='device': fills slot.dev["src"] on `stream` - mpn_jpeg_decode for the coefficient entries, a copy for the
        entries that are pixels already."""
        if slot.jpeg is None:
            slot.jpeg = jpeg.JpegBatchDecoder(self.device)
        slot.jpeg.decode([ex["image"] for ex in examples], slot.dev["src"], [int(d["src_offset"]) for d in descs], stream)

    def batches(self):
        """Generator of (features, labels); endless for training, one pass for evaluation (drop_remainder)."""
        shuffle_rng, rng = self.generators()
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._owned, self._turn, self._renderers = {}, 0, {}
        slots = collections.deque(_Slot(self.device) for _ in range(self.depth))
        records = self._records(shuffle_rng)
        with torch.cuda.device(self.device), ThreadPoolExecutor(max_workers=self.num_threads) as pool:
            def next_batch():
                raw = []
                for rec in records:
                    raw.append(rec)
                    if len(raw) == self.batch_size:
                        return [pool.submit(self._decode, r, self.decode == 'device', self.entropy) for r in raw]
                return None
            pending = next_batch()
            while pending is not None:
                examples = [f.result() for f in pending]          # record order, whatever order the threads finish in
                pending = next_batch()                            # decode of the next batch overlaps this one
                descs, people, size, so, mo = self.sample(rng, examples)
                slot = slots[0]
                slots.rotate(-1)
                yield self._launch(slot, descs, people, size, so, mo, examples)

    @property
    def dataset(self):
        return self.batches()

    def __iter__(self):
        return self.batches()
