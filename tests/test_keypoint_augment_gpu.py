"""GPU: mpn_keypoint_augment against tests/keypoint_augment_ref.py, and KeypointPipeline end to end (in-memory sources)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoint_augment_ref as ref  # noqa: E402

from multiposenet_amd.detector.input_pipeline import keypoint_augment as ka  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(97, 131), (480, 640), (203, 157), (256, 256), (331, 479), (120, 200)]


def _sources(rng):
    imgs, masks = [], []
    for h, w in SIZES:
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([xx * 255 // w, yy * 255 // h, (xx + 2 * yy) % 256], 2)
        imgs.append(np.clip(smooth + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8))
        mh, mw = ka.mask_size(h, w)
        masks.append(np.packbits(rng.integers(0, 2, (mh, mw, 2)).astype(np.uint8)))
    return imgs, masks


def _pack(imgs, masks, descs):
    src, msk = bytearray(), bytearray()
    for d, im, m in zip(descs, imgs, masks):
        d["src_offset"], d["mask_offset"] = len(src), len(msk)
        src += im.tobytes() + bytes((-im.size) % 16)
        msk += m.tobytes() + bytes((-m.size) % 16)
    return np.frombuffer(bytes(src), np.uint8), np.frombuffer(bytes(msk), np.uint8)


def _run(src, msk, descs, H, W):
    import torch
    from multiposenet_amd import _lib
    ka.check_descriptors(descs, src.size, msk.size, H, W)
    dev = "cuda"
    s, m = torch.from_numpy(src.copy()).to(dev), torch.from_numpy(msk.copy()).to(dev)
    d = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
    B = len(descs)
    img = torch.full((B, H, W, 3), float("nan"), device=dev)
    loss = torch.full((B, H // 4, W // 4), float("nan"), device=dev)
    seg = torch.full((B, H // 4, W // 4), float("nan"), device=dev)
    _lib.call("mpn_keypoint_augment", _lib.ptr(s), _lib.ptr(m), _lib.ptr(d), B, H, W, _lib.ptr(img), _lib.ptr(loss),
              _lib.ptr(seg), _lib.stream_ptr())
    torch.cuda.synchronize()
    return img.cpu().numpy(), loss.cpu().numpy(), seg.cpu().numpy()


def _descs(rng, imgs, H, W):
    """Explicit descriptors: identity, rotation, crop, rotation + crop, flip, colour, grayscale, pixel scale, all."""
    out = []
    boxes = lambda h, w: np.array([[0.2 * h, 0.3 * w, 0.8 * h, 0.6 * w]], np.float32)  # noqa: E731
    kp = np.zeros((1, 17, 3), np.int32)
    cases = ["identity", "rotate", "crop", "rotate_crop", "flip", "color", "gray", "scale", "all"]
    for i, case in enumerate(cases):
        h, w = SIZES[i % len(SIZES)]
        d = None
        while d is None:
            d0, _, _ = ka.sample_training(rng, h, w, boxes(h, w), kp, (H, W))
            want_rot = case in ("rotate", "rotate_crop", "all")
            want_crop = case in ("crop", "rotate_crop", "all")
            has_crop = (int(d0["crop_h"]), int(d0["crop_w"])) != (h, w)
            if bool(d0["flags"] & ka.ROTATE) == want_rot and has_crop == want_crop:
                d = d0
        flags = int(d["flags"]) & ka.ROTATE
        if case in ("flip", "all"):
            flags |= ka.FLIP
        if case in ("color", "all"):
            d["color"] = np.array([0.08, -0.05, 0.11], np.float32)
            flags |= ka.COLOR
        if case in ("gray", "all"):
            flags |= ka.GRAYSCALE
        if case in ("scale", "all"):
            d["seed"] = np.uint32(123456789 + i)
            flags |= ka.PIXEL_SCALE
        d["flags"] = flags
        out.append((d, i % len(SIZES)))
    return out


def test_kernel_matches_reference_training():
    rng = np.random.default_rng(0)
    imgs, masks = _sources(rng)
    H, W = 256, 192
    picks = _descs(rng, imgs, H, W)
    descs = np.stack([d for d, _ in picks])
    src, msk = _pack([imgs[j] for _, j in picks], [masks[j] for _, j in picks], descs)
    got = _run(src, msk, descs, H, W)
    want = ref.augment_batch(src, msk, descs, H, W)
    diff = float(np.abs(got[0] - want[0]).max())
    print(f"max |image - reference| = {diff:.3g}")
    assert np.isfinite(got[0]).all()
    assert diff <= 1e-6
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    assert got[1].sum() > 0 and got[2].sum() > 0


def test_kernel_matches_reference_evaluation_pad():
    rng = np.random.default_rng(1)
    imgs, masks = _sources(rng)
    descs, sizes = [], []
    for j in (0, 1):
        h, w = SIZES[j]
        d, _, _, size = ka.sample_evaluation(h, w, np.zeros((0, 4), np.float32), np.zeros((0, 17, 3), np.int32),
                                             min_dimension=256)
        descs.append(d)
        sizes.append(size)
    for j, (d, (H, W)) in enumerate(zip(descs, sizes)):
        assert H != W
        dd = np.stack([d])
        src, msk = _pack([imgs[j]], [masks[j]], dd)
        got = _run(src, msk, dd, H, W)
        want = ref.augment_batch(src, msk, dd, H, W)
        print(f"eval {SIZES[j]} -> {H}x{W}: max diff {float(np.abs(got[0] - want[0]).max()):.3g}")
        assert float(np.abs(got[0] - want[0]).max()) <= 1e-6
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
        assert np.all(got[0][:, int(d["valid_h"]):] == 0) and np.all(got[0][:, :, int(d["valid_w"]):] == 0)


def test_kernel_is_deterministic_and_seeded():
    rng = np.random.default_rng(2)
    imgs, masks = _sources(rng)
    d = ka.sample_training(rng, *SIZES[1], np.array([[100, 100, 300, 300]], np.float32), np.zeros((1, 17, 3), np.int32),
                           (128, 128))[0]
    d["flags"] = int(d["flags"]) | ka.PIXEL_SCALE
    d["seed"] = np.uint32(7)
    descs = np.stack([d])
    src, msk = _pack([imgs[1]], [masks[1]], descs)
    a, b = _run(src, msk, descs, 128, 128), _run(src, msk, descs, 128, 128)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    descs["seed"] = 8
    c = _run(src, msk, descs, 128, 128)
    assert c[0].tobytes() != a[0].tobytes()


def _examples(rng, n):
    exs = []
    for i in range(n):
        h, w = SIZES[i % len(SIZES)]
        y0, x0 = rng.uniform(0, h * 0.5, 3), rng.uniform(0, w * 0.5, 3)
        boxes = np.stack([y0, x0, y0 + rng.uniform(30, h * 0.5, 3), x0 + rng.uniform(30, w * 0.5, 3)], 1)
        kp = np.stack([rng.integers(0, h, (3, 17)), rng.integers(0, w, (3, 17)), rng.integers(0, 3, (3, 17))], 2)
        mh, mw = ka.mask_size(h, w)
        exs.append({"image": rng.integers(0, 256, (h, w, 3)).astype(np.uint8), "boxes": boxes.astype(np.float32),
                    "keypoints": kp.astype(np.int32),
                    "masks": np.packbits(rng.integers(0, 2, (mh, mw, 2)).astype(np.uint8))})
    return exs


def _take(pipe, n):
    out = []
    it = pipe.batches()
    for _ in range(n):
        f, l = next(it)
        out.append(({k: v.cpu().numpy() for k, v in f.items()}, {k: v.cpu().numpy() for k, v in l.items()}))
    return out


def test_pipeline_training_batches():
    import torch
    from multiposenet_amd.detector.input_pipeline import KeypointPipeline, get_heatmaps
    exs = _examples(np.random.default_rng(3), 10)
    params = {"batch_size": 4, "image_size": (256, 128), "seed": 11, "shuffle_buffer_size": 6}
    a = _take(KeypointPipeline(exs, True, params), 3)
    b = _take(KeypointPipeline(exs, True, params, num_threads=1), 3)
    for (fa, la), (fb, lb) in zip(a, b):
        assert fa["images"].shape == (4, 128, 256, 3) and fa["images"].dtype == np.float32
        assert la["heatmaps"].shape == (4, 32, 64, 17) and la["loss_masks"].shape == (4, 32, 64)
        assert la["segmentation_masks"].shape == (4, 32, 64) and la["num_boxes"].dtype == np.int32
        assert 0 <= fa["images"].min() and fa["images"].max() <= 1
        for k in la:
            assert la[k].tobytes() == lb[k].tobytes(), k
        assert fa["images"].tobytes() == fb["images"].tobytes()
    # the heatmaps are those of the batch's boxes / keypoints: re-derive them from the host sampler
    pipe = KeypointPipeline(exs, True, params)
    shuffle_rng, rng = pipe.generators()
    recs = pipe._records(shuffle_rng)
    decoded = [pipe._decode(next(recs)) for _ in range(4)]
    descs, people, size, _, _ = pipe.sample(rng, decoded)
    assert [len(b) for b, _ in people] == a[0][1]["num_boxes"].tolist()
    for i, (boxes, kp) in enumerate(people):
        np.testing.assert_array_equal(a[0][1]["heatmaps"][i], get_heatmaps(kp, boxes, 256, 128, 4))
    assert torch.cuda.is_available()


def test_pipeline_evaluation_feeds_model_fn():
    from multiposenet_amd.detector.input_pipeline import KeypointPipeline
    from multiposenet_amd.keypoints_model import ModeKeys, model_fn
    exs = _examples(np.random.default_rng(4), 2)
    params = {"min_dimension": 128, "backbone": "mobilenet", "depth_multiplier": 1.0, "weight_decay": 0.0,
              "dtype": "f32", "initial_learning_rate": 3e-4, "num_steps": 10, "model_dir": "unused"}
    n = 0
    for f, l in KeypointPipeline(exs, False, params).batches():
        B, H, W, _ = f["images"].shape
        assert B == 1 and H % 128 == 0 and W % 128 == 0 and H != W
        assert l["heatmaps"].shape == (1, H // 4, W // 4, 17)
        spec = model_fn(f, l, ModeKeys.EVAL, params)
        assert all(np.isfinite(float(v)) for v in spec.eval_metric_ops.values())
        n += 1
    assert n == 2


def test_pipeline_writes_into_trainer_buffers_and_trains():
    import torch
    from multiposenet_amd.detector.input_pipeline import KeypointPipeline
    from multiposenet_amd.keypoints_model import get_trainer
    from multiposenet_amd.synthetic import synthetic_batch
    params = {"batch_size": 2, "image_size": (128, 128), "backbone": "mobilenet", "depth_multiplier": 1.0,
              "weight_decay": 0.0, "dtype": "bf16", "initial_learning_rate": 3e-4, "num_steps": 10,
              "model_dir": "unused", "seed": 5, "shuffle_buffer_size": 4}
    trainer = get_trainer(params)
    bufs = trainer.input_buffers(*synthetic_batch(2, 128, 128))
    pipe = KeypointPipeline(_examples(np.random.default_rng(5), 6), True, params, buffers=bufs)
    it = pipe.batches()
    for _ in range(3):
        f, l = next(it)
        assert f["images"].data_ptr() == bufs[0]["images"].data_ptr()
        losses = trainer.step(f, l)
        assert torch.isfinite(losses).all()
