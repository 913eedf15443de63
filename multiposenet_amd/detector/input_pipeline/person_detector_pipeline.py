"""`DetectorPipeline` - the reference's input pipeline of the person detector
(detector/input_pipeline/person_detector_pipeline.py:7-106) with its pixels on the GPU.

    pipeline = DetectorPipeline(filenames, is_training=True, params=params)
    for features, labels in pipeline.dataset: ...

Built on `KeypointPipeline`: the constructor contract (params['batch_size'], params['image_size'] = (width, height),
both multiples of 128; evaluation: batch 1, params['min_dimension']), the record order (per-epoch shard shuffle, record
shuffle buffer, repeat; sharding under WORLD_SIZE > 1) and the two seeded generators are inherited. Per batch:
  host     parse (`image`, `num_persons`, `boxes` only) + JPEG decode on a pool of NUM_PARALLEL_CALLS threads, then - in
           record order, from the pipeline's seeded generator - every random decision and box (detector_augment.py); the
           decoded uint8 sources, the descriptors and the zero-padded boxes go into a PINNED staging slot (at least two;
           a slot is refilled only after its copy has completed) and are copied to the device on a side stream.
  device   on the CURRENT stream, ordered after the copy: one `mpn_detector_augment` launch.

Yields ({'images': f32 [B,H,W,3]}, {'boxes': f32 [B,M,4] normalised, zero padded, 'num_boxes': int32 [B]}) on the device:
the labels `PersonDetectorNet.create_targets` takes as they are. M is the batch's largest box count (at least 1), as
`padded_batch` gives; `num_boxes` may be 0 after pruning (person_detector_pipeline.py:101-102).

Buffers: with `buffers=(features, labels)` every batch is written into them (M is then the buffer's; an image with more
boxes raises ValueError), so a yielded batch is valid until the next one is requested. Otherwise the pipeline alternates
between two owned buffer sets: a batch stays valid until the next-but-one is requested.

`filenames` may also be an in-memory sequence of decoded examples, dicts with 'image' (uint8 [h,w,3]) and 'boxes'
(f32 [P,4] absolute) - no PIL is needed for those.
"""
import collections
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import _lib
from ...inference import jpeg
from ..constants import NUM_PARALLEL_CALLS
from . import detector_augment as da
from .keypoints_detector_pipeline import DECODE_MODES, KeypointPipeline, _align, _Slot, check_decode_mode  # noqa: F401
from .tfrecord import decode_jpeg, parse_example, read_records


def decode_detector_example(data, decode_image=True):
    """One serialized record -> {'image': uint8 [h,w,3] (or the JPEG bytes), 'boxes': f32 [P,4] absolute}; the features
    person_detector_pipeline.py:72-76 reads, the rest of the record is ignored."""
    f = parse_example(data)
    for k in ("image", "num_persons"):
        if f.get(k) is None:
            raise ValueError(f"record has no '{k}' feature")
    p = int(f["num_persons"][0])
    boxes = f.get("boxes")
    boxes = np.zeros(0, np.float32) if boxes is None else boxes
    if boxes.size != p * 4:
        raise ValueError(f"record: num_persons={p} but {boxes.size} box values")
    image = f["image"][0]
    return {"image": decode_jpeg(image) if decode_image else image, "boxes": boxes.reshape(p, 4).astype(np.float32)}


class DetectorPipeline(KeypointPipeline):
    def __init__(self, filenames, is_training, params, device=None, buffers=None, num_threads=NUM_PARALLEL_CALLS, seed=0,
                 depth=2, decode='host', entropy='host'):
        """filenames: paths of TFRecord files, or a sequence of decoded examples. params: 'batch_size', 'image_size'
        (width, height) for training, 'min_dimension' for evaluation; optional 'seed' (overrides `seed`) and
        'shuffle_buffer_size'. decode: 'host' or 'device', entropy: 'host' or 'device', as for `KeypointPipeline`."""
        super().__init__(filenames, is_training, params, device=device, buffers=buffers, num_threads=num_threads,
                         depth=depth, decode=decode, entropy=entropy)
        self.seed = int(params.get("seed", seed))
        self._num_examples = None

    @property
    def num_examples(self):
        """The number of records in all files (person_detector_pipeline.py:23-30), counted on first use."""
        if self._num_examples is None:
            self._num_examples = (len(self._examples) if self._examples is not None
                                  else sum(sum(1 for _ in read_records(f)) for f in self._files))
        return self._num_examples

    @staticmethod
    def _decode(rec, device=False, entropy='host'):
        if isinstance(rec, (bytes, bytearray, memoryview)):
            ex = decode_detector_example(rec, decode_image=not device)
        else:
            ex = dict(rec)
        img = ex["image"]
        if isinstance(img, (bytes, bytearray, memoryview)):
            img = jpeg.prepare(img, entropy, extended=True) if device else decode_jpeg(img)
        if not isinstance(img, (jpeg.Coefficients, jpeg.Scan)):
            img = np.ascontiguousarray(img, dtype=np.uint8)
            if img.ndim != 3 or img.shape[2] != 3:
                raise ValueError(f"image must be uint8 [H,W,3], got {img.shape}")
        return {"image": img, "boxes": np.asarray(ex["boxes"], np.float32).reshape(-1, 4)}

    # ---------------------------------------------------------------- host sampling
    def sample(self, rng, examples):
        """Descriptors (offsets filled) and boxes of one batch of decoded examples, drawn in record order.
        Returns (descs, boxes per image, (H, W), src_bytes)."""
        descs = np.zeros(len(examples), da.DESC_DTYPE)
        boxes, so, size = [], 0, None
        for i, ex in enumerate(examples):
            h, w = ex["image"].shape[:2]
            if self.is_training:
                d, b = da.sample_training(rng, h, w, ex["boxes"], self.image_size)
                size = self.image_size
            else:
                d, b, size = da.sample_evaluation(h, w, ex["boxes"], self.min_dimension)
            d["src_offset"] = so
            descs[i] = d
            so += _align(h * w * 3, 16)
            boxes.append(b)
        return descs, boxes, size, so

    # ---------------------------------------------------------------- device
    def _outputs(self, H, W, M):
        B = self.batch_size
        if self.buffers is not None:
            feats, labels = self.buffers
            if tuple(feats["images"].shape) != (B, H, W, 3):
                raise ValueError(f"buffers hold images {tuple(feats['images'].shape)}, batch is {(B, H, W, 3)}")
            return feats, labels
        key = (H, W)
        sets = self._owned.get(key)
        if sets is None:
            sets = self._owned[key] = [{"images": torch.empty((B, H, W, 3), dtype=torch.float32, device=self.device),
                                        "num_boxes": torch.empty((B,), dtype=torch.int32, device=self.device),
                                        "boxes": None} for _ in range(2)]
        self._turn ^= 1
        s = sets[self._turn]
        if s["boxes"] is None or s["boxes"].numel() < B * M * 4:         # grown buffers are new memory: nothing queued uses them
            s["boxes"] = torch.empty(_align(B * M * 4 * 2, 64), dtype=torch.float32, device=self.device)
        return {"images": s["images"]}, {"boxes": s["boxes"][:B * M * 4].view(B, M, 4), "num_boxes": s["num_boxes"]}

    def _launch(self, slot, descs, boxes, size, src_total, examples):
        H, W = size
        B = len(descs)
        counts = np.array([len(b) for b in boxes], np.int32)
        if self.buffers is not None:
            M = int(self.buffers[1]["boxes"].shape[1])
            if counts.max() > M:
                raise ValueError(f"an image of this batch has {int(counts.max())} boxes, the label buffer holds {M}")
        else:
            M = max(1, int(counts.max()))
        # a slot's pinned arrays may be rewritten only once its previous copy has left them
        slot.copied.synchronize()
        src = slot.reserve("src", src_total)
        if self.decode == 'host':
            for d, ex in zip(descs, examples):
                so, n = int(d["src_offset"]), ex["image"].size
                src[so:so + n] = ex["image"].reshape(-1)
        da.check_descriptors(descs, src_total, H, W)
        padded = np.zeros((B, M, 4), np.float32)
        for i, b in enumerate(boxes):
            padded[i, :len(b)] = b
        desc_bytes = descs.nbytes
        bx_off = _align(desc_bytes)
        nb_off = bx_off + _align(padded.nbytes)
        meta = slot.reserve("meta", nb_off + _align(B * 4))
        meta[:desc_bytes] = descs.view(np.uint8)
        meta[bx_off:bx_off + padded.nbytes] = padded.view(np.uint8).reshape(-1)
        meta[nb_off:nb_off + B * 4] = counts.view(np.uint8)

        main = torch.cuda.current_stream(self.device)
        cs = self._copy_stream
        if slot.consumed is not None:
            cs.wait_event(slot.consumed)            # the launch that read this slot's device copy has done so
        with torch.cuda.stream(cs):
            for name, n in (("src", src_total), ("meta", nb_off + B * 4)):
                if name != "src" or self.decode == 'host':
                    slot.dev[name][:n].copy_(slot.host[name][:n], non_blocking=True)
            if self.decode == 'device':
                self._decode_sources(slot, descs, examples, cs)
            slot.copied.record(cs)
        main.wait_event(slot.copied)
        feats, labels = self._outputs(H, W, M)
        dm = slot.dev["meta"]
        _lib.call("mpn_detector_augment", _lib.ptr(slot.dev["src"]), _lib.ptr(dm), B, H, W, _lib.ptr(feats["images"]),
                  _lib.stream_ptr())
        labels["boxes"].copy_(dm[bx_off:bx_off + padded.nbytes].view(torch.float32).view(B, M, 4))
        labels["num_boxes"].copy_(dm[nb_off:nb_off + B * 4].view(torch.int32))
        ev = torch.cuda.Event()
        ev.record(main)
        slot.consumed = ev
        return feats, labels

    def batches(self):
        """Generator of (features, labels); endless for training, one pass for evaluation (drop_remainder)."""
        shuffle_rng, rng = self.generators()
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._owned, self._turn = {}, 0
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
                descs, boxes, size, so = self.sample(rng, examples)
                slot = slots[0]
                slots.rotate(-1)
                yield self._launch(slot, descs, boxes, size, so, examples)
