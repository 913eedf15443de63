"""GPU: mpn_image_resize against the numpy restatement of Pillow's resize (tests/pil_resize_ref.py, itself held to Pillow's own
outputs on the CPU) byte for byte, and mpn_pose_gather_sized against its restatement bit for bit. Pillow is not needed here."""
import os

import numpy as np
import pytest
import torch

import image_gather_ref as G
import pil_resize_ref as P
import pose_gather_ref as ref
from multiposenet_amd import _lib
from multiposenet_amd.inference import resample

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil_resize_goldens.npz")


def _golden_sources():
    with np.load(GOLDEN) as z:
        return [z[f"{n}/source"] for n in z["names"]], [z[f"{n}/resized"] for n in z["names"]]


def _seeded(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]


class _Buffers:
    """Device buffers of fixed capacity, reused between calls like the ones a captured graph holds."""

    def __init__(self, b, height, width, stage_bytes, meta_words, work_bytes):
        self.b, self.height, self.width = b, height, width
        self.sources = torch.zeros(stage_bytes, dtype=torch.uint8, device="cuda")
        self.meta = torch.zeros(meta_words, dtype=torch.int32, device="cuda")
        self.work = torch.full((work_bytes,), 0xAB, dtype=torch.uint8, device="cuda")
        self.out = torch.full((b, height, width, 3), 0xCD, dtype=torch.uint8, device="cuda")

    def run(self, images, keep):
        plan = resample.Plan([im.shape[:2] for im in images], self.height, self.width, keep)
        assert plan.stage_bytes <= self.sources.numel() and plan.meta_words <= self.meta.numel() and plan.work_bytes <= self.work.numel()
        packed = np.zeros(plan.stage_bytes, np.uint8)
        for im, at in zip(images, plan.src_offsets):
            packed[at:at + im.size] = im.reshape(-1)
        self.sources[:plan.stage_bytes].copy_(torch.from_numpy(packed))
        self.meta[:plan.meta_words].copy_(torch.from_numpy(plan.meta))
        b = self.b
        tables = self.meta[b * (resample.DESC_WORDS + 4):]
        _lib.call("mpn_image_resize", _lib.ptr(self.sources), _lib.ptr(tables), _lib.ptr(self.meta), b, self.height, self.width,
                  _lib.ptr(self.out), _lib.ptr(self.work), self.work.numel(), _lib.stream_ptr())
        torch.cuda.synchronize()
        return self.out.cpu().numpy(), plan


def _check(buffers, images, keep):
    got, plan = buffers.run(images, keep)
    for i, im in enumerate(images):
        want = P.canvas(im, buffers.height, buffers.width, keep)                  # zero padding included
        np.testing.assert_array_equal(got[i], want, err_msg=f"image {i} {im.shape} keep_aspect_ratio={keep}")
    return got, plan


def test_goldens_at_their_own_sizes(cuda):
    """Every golden case alone, canvas = Pillow's output size rounded up so that W*3 is a multiple of 16: the resized part
    equals PILLOW's bytes (not only the restatement's)."""
    sources, resized = _golden_sources()
    for src, want in zip(sources, resized):
        oh, ow = want.shape[:2]
        H, W = oh, (ow + 15) // 16 * 16
        # the descriptor asks for Pillow's oh x ow inside the (wider) canvas
        plan2 = resample.Plan([src.shape[:2]], oh, ow)
        buf = _Buffers(1, H, W, plan2.stage_bytes, plan2.meta_words, plan2.work_bytes)
        meta = plan2.meta
        packed = np.zeros(plan2.stage_bytes, np.uint8)
        packed[:src.size] = src.reshape(-1)
        buf.sources[:plan2.stage_bytes].copy_(torch.from_numpy(packed))
        buf.meta[:len(meta)].copy_(torch.from_numpy(meta))
        _lib.call("mpn_image_resize", _lib.ptr(buf.sources), _lib.ptr(buf.meta[resample.DESC_WORDS + 4:]), _lib.ptr(buf.meta), 1, H, W,
                  _lib.ptr(buf.out), _lib.ptr(buf.work), buf.work.numel(), _lib.stream_ptr())
        torch.cuda.synchronize()
        got = buf.out.cpu().numpy()[0]
        np.testing.assert_array_equal(got[:, :ow], want)
        assert not got[:, ow:].any()


@pytest.mark.parametrize("keep", [False, True])
def test_ragged_batch_equals_the_restatement_and_leaves_no_stale_bytes(cuda, keep):
    sources, _ = _golden_sources()
    big = _seeded([(1080, 1920), (720, 1280), (333, 1000), (256, 384), (97, 131), (1, 7)], 5)
    first = sources + big
    H, W = 256, 384
    # the same buffers serve other sizes in another order (large images where small ones were, and the reverse)
    second = _seeded([(1, 7), (50, 40), (700, 900), (31, 257), (256, 384), (1000, 333), (12, 12), (480, 640), (5, 300), (64, 64),
                      (800, 600), (129, 383), (3, 3), (1080, 1920), (40, 50), (200, 100), (90, 1600)], 6)
    plans = [resample.Plan([im.shape[:2] for im in batch], H, W, keep) for batch in (first, second)]
    buf = _Buffers(len(first), H, W, *(resample.capacity_for(max(getattr(p, f) for p in plans))
                                       for f in ("stage_bytes", "meta_words", "work_bytes")))
    got, plan = _check(buf, first, keep)
    assert any(n != (H, W) for n in plan.new_sizes) == keep
    assert sum(int(g.any()) for g in got) == len(first)
    assert len(second) == len(first)
    _check(buf, second, keep)
    _check(buf, first, keep)


def test_bad_descriptors_write_zeros_not_memory(cuda):
    """A descriptor whose intermediate does not fit the workspace, or whose size exceeds the canvas, gives a zero image."""
    images = _seeded([(60, 80), (60, 80)], 7)
    H, W = 128, 128
    plan = resample.Plan([im.shape[:2] for im in images], H, W)
    buf = _Buffers(2, H, W, plan.stage_bytes, plan.meta_words, plan.work_bytes)
    packed = np.zeros(plan.stage_bytes, np.uint8)
    for im, at in zip(images, plan.src_offsets):
        packed[at:at + im.size] = im.reshape(-1)
    meta = plan.meta.copy()
    meta[resample.DESC_WORDS:2 * resample.DESC_WORDS].view(np.int64)[1] = 1 << 40            # image 1: tmp_offset far outside the workspace
    buf.sources[:plan.stage_bytes].copy_(torch.from_numpy(packed))
    buf.meta[:len(meta)].copy_(torch.from_numpy(meta))
    _lib.call("mpn_image_resize", _lib.ptr(buf.sources), _lib.ptr(buf.meta[2 * (resample.DESC_WORDS + 4):]), _lib.ptr(buf.meta), 2, H, W,
              _lib.ptr(buf.out), _lib.ptr(buf.work), buf.work.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    got = buf.out.cpu().numpy()
    np.testing.assert_array_equal(got[0], P.canvas(images[0], H, W))
    assert not got[1].any()


def _gather_inputs(B, M, seed):
    rng = np.random.RandomState(seed)
    lo = rng.rand(B, M, 2).astype(np.float32) * 0.5
    boxes = np.concatenate([lo, lo + rng.rand(B, M, 2).astype(np.float32) * 0.5], -1).astype(np.float32)
    scores = rng.rand(B, M).astype(np.float32)
    num = rng.randint(0, M + 1, B).astype(np.int32)
    num[0], num[-1] = M, 0
    ks, kp = rng.rand(B * M, 17).astype(np.float32), rng.rand(B * M, 17, 2).astype(np.float32)
    return boxes, scores, num, ks, kp


def _run_gather(name, boxes, scores, num, ks, kp, thr, tail):
    B, M = scores.shape
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = [dev(a) for a in (boxes, scores, num, ks, kp)]
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = _lib.lib().mpn_pose_gather_record_bytes(B, M)
    rec = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device="cuda")
    _lib.call(name, *[_lib.ptr(a) for a in t], _lib.ptr(over), B, M, float(thr), *tail, _lib.ptr(rec), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rec.cpu().numpy()


@pytest.mark.parametrize("with_keypoints", [True, False])
def test_pose_gather_sized_equals_its_restatement_and_pose_gather(cuda, with_keypoints):
    B, M, H, W = 5, 25, 256, 384
    boxes, scores, num, ks, kp = _gather_inputs(B, M, 11)
    if not with_keypoints:
        ks = kp = None
    shapes = [(1080, 1920), (97, 131), (256, 384), (333, 1000), (50, 40)]
    ext = np.stack([resample.extent_of(h, w, *resample.resized_size(h, w, H, W, True), H, W) for h, w in shapes])
    assert len({tuple(e) for e in ext}) == B and (ext[:, :2] != 1).any()
    e_dev = torch.from_numpy(ext).cuda()
    got = _run_gather("mpn_pose_gather_sized", boxes, scores, num, ks, kp, 0.4, (_lib.ptr(e_dev),))
    want = G.pose_gather_sized(boxes, scores, num, ks, kp, 0, 0.4, ext)
    assert 0 < int(want[:4].view(np.int32)[0]) < B * M
    assert got.tobytes() == want.tobytes()
    # extents (1, 1, H, W): mpn_pose_gather's record
    unit = torch.tensor([[1.0, 1.0, H, W]] * B, dtype=torch.float32, device="cuda")
    sized = _run_gather("mpn_pose_gather_sized", boxes, scores, num, ks, kp, 0.4, (_lib.ptr(unit),))
    plain = _run_gather("mpn_pose_gather", boxes, scores, num, ks, kp, 0.4, (H, W))
    assert sized.tobytes() == plain.tobytes() == ref.pose_gather(boxes, scores, num, ks, kp, 0, 0.4, H, W).tobytes()
