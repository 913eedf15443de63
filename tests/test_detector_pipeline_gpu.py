"""GPU: mpn_detector_augment against tests/detector_augment_ref.py (bit for bit, every pixel), DetectorPipeline end to end
(in-memory sources and toy records), and the train / evaluate loop of multiposenet_amd.train_person_detector."""
import io
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detector_augment_ref as ref  # noqa: E402

from multiposenet_amd.detector.input_pipeline import detector_augment as da  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(97, 131), (480, 640), (203, 157), (256, 256), (331, 479), (120, 200), (700, 900), (33, 21)]


def _image(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([xx * 255 // w, yy * 255 // h, (xx + 2 * yy) % 256], 2)
    return np.clip(smooth + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def _pack(imgs, descs):
    src = bytearray()
    for d, im in zip(descs, imgs):
        d["src_offset"] = len(src)
        src += im.tobytes() + bytes((-im.size) % 16)
    return np.frombuffer(bytes(src), np.uint8)


def _run(src, descs, H, W):
    import torch
    from multiposenet_amd import _lib
    da.check_descriptors(descs, src.size, H, W)           # (the kernel also guards every read by the descriptor's own sizes)
    s = torch.from_numpy(src.copy()).to("cuda")
    d = torch.from_numpy(descs.view(np.uint8).copy()).to("cuda")
    img = torch.full((len(descs), H, W, 3), float("nan"), device="cuda")
    _lib.call("mpn_detector_augment", _lib.ptr(s), _lib.ptr(d), len(descs), H, W, _lib.ptr(img), _lib.stream_ptr())
    torch.cuda.synchronize()
    return img.cpu().numpy()


def _desc(h, w, H, W, crop=None, valid=None, pad=None, flags=0, seed=0):
    cy, cx, ch, cw = crop or (0, 0, h, w)
    vh, vw = valid or (H, W)
    d = np.zeros((), da.DESC_DTYPE)
    d["src_h"], d["src_w"] = h, w
    d["crop_y"], d["crop_x"], d["crop_h"], d["crop_w"] = cy, cx, ch, cw
    d["valid_h"], d["valid_w"] = vh, vw
    d["scale_y"], d["scale_x"] = F(ch) / F(vh), F(cw) / F(vw)
    if pad is not None:
        py, px, ph, pw = pad
        d["pad_y"], d["pad_x"], d["pad_h"], d["pad_w"] = py, px, ph, pw
        d["pad_scale_y"], d["pad_scale_x"] = F(H) / F(ph), F(W) / F(pw)
        flags |= da.PAD
    d["color"] = np.array([0.08, -0.05, 0.11], F)
    d["minval"], d["maxval"], d["seed"] = 0.8, 1.2, seed
    d["flags"] = flags
    return d


def _handmade(H, W):
    """(name, source size, descriptor): each flag alone and all together, the padded rectangle at each canvas edge, crops of
    one row / one column / one pixel, sources smaller and larger than the output, evaluation with bottom and right pad."""
    ALL = da.COLOR | da.GRAYSCALE | da.PIXEL_SCALE | da.FLIP
    ph, pw = int(0.6 * H), int(0.7 * W)
    cases = [
        ("identity", (H, W), {}),
        ("small_source", (33, 21), {}),
        ("large_source", (700, 900), {}),
        ("crop", (480, 640), dict(crop=(37, 101, 390, 420))),
        ("color", (203, 157), dict(flags=da.COLOR)),
        ("gray", (331, 479), dict(flags=da.GRAYSCALE)),
        ("scale", (120, 200), dict(flags=da.PIXEL_SCALE, seed=0xDEADBEEF)),
        ("flip", (97, 131), dict(flags=da.FLIP)),
        ("pad_inside", (256, 256), dict(pad=(H // 10, W // 10, ph, pw))),
        ("pad_top_left", (480, 640), dict(pad=(0, 0, ph, pw))),
        ("pad_bottom_right", (203, 157), dict(pad=(H - ph, W - pw, ph, pw))),
        ("pad_top_right", (331, 479), dict(pad=(0, W - pw, ph, pw), crop=(5, 9, 300, 401))),
        ("pad_bottom_left", (120, 200), dict(pad=(H - ph, 0, ph, pw))),
        ("pad_full_canvas", (97, 131), dict(pad=(0, 0, H, W))),
        ("pad_one_pixel", (97, 131), dict(pad=(H // 2, W // 3, 1, 1))),
        ("pad_color_on_the_padding", (256, 256), dict(pad=(7, 5, ph, pw), flags=da.COLOR)),
        ("crop_one_row", (203, 157), dict(crop=(100, 3, 1, 150))),
        ("crop_one_column", (203, 157), dict(crop=(2, 77, 190, 1))),
        ("crop_one_pixel", (203, 157), dict(crop=(202, 156, 1, 1), flags=da.COLOR)),
        ("all", (480, 640), dict(crop=(40, 60, 400, 500), pad=(H // 16, W // 8, ph, pw), flags=ALL, seed=12345)),
        ("all_with_one_pixel_crop", (33, 21), dict(crop=(32, 0, 1, 1), pad=(1, 2, ph, pw), flags=ALL, seed=7)),
        ("eval_bottom_pad", (480, 640), dict(valid=(H - H // 5, W), flags=da.EVAL)),
        ("eval_right_pad", (640, 480), dict(valid=(H, W - W // 3), flags=da.EVAL)),
        ("eval_all_together", (331, 479), dict(valid=(H - 3, W - 5), pad=(2, 3, ph, pw), flags=ALL | da.EVAL, seed=99)),
    ]
    return cases


@pytest.mark.parametrize("size", [(256, 384), (640, 640), (128, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement_on_handmade_descriptors(cuda, size):
    H, W = size
    rng = np.random.default_rng(H + W)
    cases = _handmade(H, W)
    ph, pw = int(0.6 * H), int(0.7 * W)
    imgs = [_image(rng, *shape) for _, shape, _ in cases]
    descs = np.zeros(len(cases), da.DESC_DTYPE)
    for i, (name, (h, w), kw) in enumerate(cases):
        descs[i] = _desc(h, w, H, W, **kw)
    src = _pack(imgs, descs)
    got = _run(src, descs, H, W)
    want = ref.augment_batch(src, descs, H, W)
    assert got.dtype == F and not np.isnan(got).any()
    for i, (name, _, _) in enumerate(cases):
        bad = int((got[i].view(np.uint32) != want[i].view(np.uint32)).sum()) if not np.array_equal(got[i], want[i]) else 0
        print(f"{H}x{W} {name}: {bad} of {got[i].size} elements differ")
        np.testing.assert_array_equal(got[i], want[i], err_msg=name)
    # the cases do what their names say
    by = {name: i for i, (name, _, _) in enumerate(cases)}
    assert np.all(got[by["pad_inside"]][:H // 10] == 0) and np.all(got[by["pad_inside"]][:, :W // 10] == 0)
    assert got[by["pad_inside"]][H // 10:H // 10 + ph, W // 10:W // 10 + pw].any()
    assert got[by["pad_color_on_the_padding"]][0, 0].tolist() == [F(0.08), 0, F(0.11)]       # zero + offset, clipped
    assert np.all(got[by["eval_bottom_pad"]][H - H // 5:] == 0) and got[by["eval_bottom_pad"]][:H - H // 5].any()
    assert np.all(got[by["eval_right_pad"]][:, W - W // 3:] == 0)
    plain = descs[by["pad_full_canvas"]:by["pad_full_canvas"] + 1].copy()       # a pad over the whole canvas is the identity
    plain["flags"] = 0
    np.testing.assert_array_equal(got[by["pad_full_canvas"]], _run(src, plain, H, W)[0])
    one = got[by["crop_one_pixel"]]
    assert np.all(one == one[0, 0])


@pytest.mark.parametrize("seed,B,size", [(0, 32, (640, 640)), (1, 32, (256, 384)), (2, 17, (384, 256)), (3, 8, (128, 128))])
def test_kernel_equals_the_restatement_on_sampled_batches(cuda, seed, B, size):
    H, W = size
    rng = np.random.default_rng(seed)
    imgs, descs, seen = [], np.zeros(B, da.DESC_DTYPE), 0
    for i in range(B):
        h, w = int(rng.integers(300, 481)), int(rng.integers(400, 641))
        imgs.append(_image(rng, h, w))
        boxes = np.array([[0.2 * h, 0.3 * w, 0.8 * h, 0.6 * w], [0.1 * h, 0.1 * w, 0.5 * h, 0.9 * w]], F)
        descs[i], _ = da.sample_training(rng, h, w, boxes, size)
        if i % 4 == 3:                                # the rare decisions, more often than the sampler takes them
            descs[i]["flags"] |= da.PIXEL_SCALE | (da.GRAYSCALE if i % 8 == 7 else 0)
            descs[i]["minval"], descs[i]["maxval"], descs[i]["seed"] = 0.8, 1.2, rng.integers(1 << 32)
        if i % 5 == 4 and not descs[i]["flags"] & da.PAD:
            _, _, (oy, ox, sh, sw) = da.random_pad(rng, np.zeros((0, 4), F), H, W)
            for k, v in (("pad_y", oy), ("pad_x", ox), ("pad_h", sh), ("pad_w", sw),
                         ("pad_scale_y", F(H) / F(sh)), ("pad_scale_x", F(W) / F(sw))):
                descs[i][k] = v
            descs[i]["flags"] |= da.PAD
        seen |= int(descs[i]["flags"])
    assert seen & da.PAD and seen & da.PIXEL_SCALE and seen & da.FLIP and seen & da.COLOR
    src = _pack(imgs, descs)
    got = _run(src, descs, H, W)
    want = ref.augment_batch(src, descs, H, W)
    for i in range(B):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"image {i}, flags {int(descs[i]['flags'])}")
    assert got.min() >= 0 and got.max() <= 1
    # determinism: the same launch twice; another pixel-scale seed changes the pixel-scaled images and no other
    np.testing.assert_array_equal(_run(src, descs, H, W), got)
    other = descs.copy()
    other["seed"] ^= np.uint32(0x5BD1E995)
    again = _run(src, other, H, W)
    for i in range(B):
        same = np.array_equal(again[i], got[i])
        assert same != bool(descs[i]["flags"] & da.PIXEL_SCALE), i


def test_entry_point_checks_its_arguments(cuda):
    import torch
    from multiposenet_amd import _lib
    d = torch.zeros(112, dtype=torch.uint8, device="cuda")
    s = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 8, 8, 3), device="cuda")
    for B, H, W in ((0, 8, 8), (1, 6, 8), (1, 8, 0), (1, 16388, 8), (70000, 8, 8)):
        with pytest.raises(ValueError, match="BAD_SHAPE"):
            _lib.call("mpn_detector_augment", _lib.ptr(s), _lib.ptr(d), B, H, W, _lib.ptr(out), _lib.stream_ptr())
    with pytest.raises(ValueError, match="BAD_ARG"):
        _lib.call("mpn_detector_augment", None, _lib.ptr(d), 1, 8, 8, _lib.ptr(out), _lib.stream_ptr())
    with pytest.raises(ValueError, match="BAD_ALIGN"):
        _lib.call("mpn_detector_augment", _lib.ptr(s), _lib.ptr(d), 1, 8, 8, _lib.ptr(out.view(-1)[1:]), _lib.stream_ptr())


# ---------------------------------------------------------------------------------------------------- pipeline
def _examples(rng, n, crowd_at=None):
    out = []
    for i in range(n):
        h, w = int(rng.integers(200, 481)), int(rng.integers(240, 641))
        p = 9 if i == crowd_at else int(rng.integers(1, 5))
        bh, bw = rng.uniform(0.2, 0.8, p) * h, rng.uniform(0.1, 0.5, p) * w
        y0, x0 = rng.uniform(0, 1, p) * (h - bh), rng.uniform(0, 1, p) * (w - bw)
        out.append({"image": _image(rng, h, w), "boxes": np.stack([y0, x0, y0 + bh, x0 + bw], 1).astype(F)})
    return out


def test_training_batches_equal_restatement_and_sampler(cuda):
    import torch
    from multiposenet_amd.detector.input_pipeline import DetectorPipeline
    examples = _examples(np.random.default_rng(21), 11, crowd_at=4)
    params = {"batch_size": 4, "image_size": (384, 256), "shuffle_buffer_size": 6}
    pipe = DetectorPipeline(examples, True, params, seed=3)
    assert pipe.num_examples == 11
    # the host half on its own, from the same seed: records -> sampler -> restatement
    host = DetectorPipeline(examples, True, params, seed=3, num_threads=1)
    shuffle_rng, rng = host.generators()
    records = host._records(shuffle_rng)
    a, b = pipe.batches(), DetectorPipeline(examples, True, params, seed=3, num_threads=8).batches()
    held = []
    for step in range(6):
        ex = [host._decode(next(records)) for _ in range(4)]
        descs, boxes, size, total = host.sample(rng, ex)
        assert size == (256, 384)
        want = ref.augment_batch(_pack([e["image"] for e in ex], descs), descs, 256, 384)
        (fa, la), (fb, lb) = next(a), next(b)
        torch.cuda.synchronize()
        M = max(1, max(len(x) for x in boxes))
        assert fa["images"].dtype == torch.float32 and tuple(fa["images"].shape) == (4, 256, 384, 3)
        assert la["boxes"].dtype == torch.float32 and tuple(la["boxes"].shape) == (4, M, 4) and la["boxes"].is_contiguous()
        assert la["num_boxes"].dtype == torch.int32 and la["num_boxes"].tolist() == [len(x) for x in boxes]
        np.testing.assert_array_equal(fa["images"].cpu().numpy(), want)
        got = la["boxes"].cpu().numpy()
        for i, x in enumerate(boxes):
            np.testing.assert_array_equal(got[i, :len(x)], x)
            assert np.all(got[i, len(x):] == 0)                          # padding rows
        assert torch.equal(fa["images"], fb["images"]) and torch.equal(la["boxes"], lb["boxes"])     # 1 and 8 threads
        held.append((fa["images"], want))
        if len(held) >= 2:                     # a batch stays valid until the next-but-one is requested
            np.testing.assert_array_equal(held[-2][0].cpu().numpy(), held[-2][1])
    other = next(DetectorPipeline(examples, True, params, seed=4).batches())
    assert not torch.equal(other[0]["images"], held[0][0])


def test_caller_buffers_and_too_many_boxes(cuda):
    import torch
    from multiposenet_amd.detector.input_pipeline import DetectorPipeline
    examples = _examples(np.random.default_rng(22), 6)
    params = {"batch_size": 2, "image_size": (128, 128)}

    def buffers(M):
        return ({"images": torch.empty((2, 128, 128, 3), device="cuda")},
                {"boxes": torch.full((2, M, 4), 7.0, device="cuda"), "num_boxes": torch.empty(2, dtype=torch.int32, device="cuda")})
    buf = buffers(12)
    feats, labels = next(DetectorPipeline(examples, True, params, buffers=buf, seed=1).batches())
    want = next(DetectorPipeline(examples, True, params, seed=1).batches())
    assert feats["images"] is buf[0]["images"] and labels["boxes"] is buf[1]["boxes"]
    assert torch.equal(feats["images"], want[0]["images"]) and torch.equal(labels["num_boxes"], want[1]["num_boxes"])
    m = want[1]["boxes"].shape[1]
    assert torch.equal(labels["boxes"][:, :m], want[1]["boxes"]) and bool((labels["boxes"][:, m:] == 0).all())
    crowd = [dict(e, boxes=np.repeat(e["boxes"][:1], 40, 0)) for e in examples]     # 40 copies survive or fall together
    with pytest.raises(ValueError, match=r"40 boxes.* holds 3\b"):
        for _ in zip(range(8), DetectorPipeline(crowd, True, params, buffers=buffers(3), seed=1).batches()):
            pass
    with pytest.raises(ValueError, match="buffers hold images"):
        next(DetectorPipeline(examples, True, {"batch_size": 2, "image_size": (256, 128)}, buffers=buf).batches())


def _params(tmp_path, name, **kw):
    from multiposenet_amd import train_person_detector as tpd
    return dict(dict(tpd.PARAMS, model_dir=str(tmp_path / name), pretrained_checkpoint="", batch_size=4,
                     image_size=(256, 256), min_dimension=256, dtype="bf16"), **kw)


def test_evaluation_batches_feed_model_fn(cuda, tmp_path):
    import torch
    from multiposenet_amd import person_detector_model as pdm
    from multiposenet_amd.detector.input_pipeline import DetectorPipeline
    from multiposenet_amd.detector.input_pipeline.keypoint_augment import evaluation_size
    from multiposenet_amd.keypoints_model import ModeKeys
    rng = np.random.default_rng(23)
    examples = _examples(rng, 3) + [{"image": _image(rng, 300, 200), "boxes": np.zeros((0, 4), F)}]
    params = _params(tmp_path, "e")
    pdm.reset_registry()
    n = 0
    for (feats, labels), ex in zip(DetectorPipeline(examples, False, params).batches(), examples):
        h, w = ex["image"].shape[:2]
        new_h, new_w, hp, wp = evaluation_size(h, w, 256)
        d, boxes, size = da.sample_evaluation(h, w, ex["boxes"], 256)
        d = np.atleast_1d(d)
        want = ref.augment_batch(_pack([ex["image"]], d), d, hp, wp)
        assert size == (hp, wp) and tuple(feats["images"].shape) == (1, hp, wp, 3)
        np.testing.assert_array_equal(feats["images"].cpu().numpy(), want)
        assert not want[0, new_h:].any() and not want[0, :, new_w:].any()
        assert labels["num_boxes"].tolist() == [len(ex["boxes"])] and labels["boxes"].shape[1] == max(1, len(ex["boxes"]))
        np.testing.assert_array_equal(labels["boxes"][0, :len(boxes)].cpu().numpy(), boxes)
        spec = pdm.model_fn(feats, labels, ModeKeys.EVAL, params)
        assert set(spec.eval_metric_ops) == {"boxes", "scores", "num_boxes"} and np.isfinite(float(spec.loss))
        n += 1
    assert n == 4
    pdm.reset_registry()


def test_a_batch_with_an_image_without_boxes_trains(cuda, tmp_path):
    """Images left without boxes (num_boxes 0, person_detector_pipeline.py:101-102: every box pruned, or a record without
    persons) go through anchor matching and the TRAIN step, alone in a row of the batch and next to images with boxes."""
    import torch
    from multiposenet_amd import person_detector_model as pdm
    from multiposenet_amd.detector.input_pipeline import DetectorPipeline
    from multiposenet_amd.keypoints_model import ModeKeys
    rng = np.random.default_rng(24)
    examples = _examples(rng, 8)
    for e in examples[:3]:
        e["boxes"] = np.zeros((0, 4), F)
    params = _params(tmp_path, "z", shuffle_buffer_size=4)
    pdm.reset_registry()
    seen_empty = 0
    for _, (feats, labels) in zip(range(6), DetectorPipeline(examples, True, params, seed=5).batches()):
        nb = labels["num_boxes"].tolist()
        seen_empty += nb.count(0)
        spec = pdm.model_fn(feats, labels, ModeKeys.TRAIN, params)
        assert all(np.isfinite(float(v)) for v in spec.losses.values()), (nb, spec.losses)
    assert seen_empty > 0
    pdm.reset_registry()


# ---------------------------------------------------------------------------------------------------- train / evaluate
def _toy_shards(tmp_path, seed=0, shards=2, records=6):
    """Records in the contract of tools/make_toy_tfrecords.py (a real small JPEG; the keypoint features are left out: the
    detector's pipeline reads `image`, `num_persons` and `boxes` only)."""
    from PIL import Image
    from multiposenet_amd.detector.input_pipeline.tfrecord import encode_example, frame_record
    rng = np.random.default_rng(seed)
    paths = []
    for s in range(shards):
        paths.append(str(tmp_path / f"shard-{s:04d}.tfrecords"))
        with open(paths[-1], "wb") as f:
            for e in _examples(rng, records):
                buf = io.BytesIO()
                Image.fromarray(e["image"]).save(buf, format="JPEG", quality=90)
                f.write(frame_record(encode_example({"image": buf.getvalue(), "num_persons": np.array([len(e["boxes"])], np.int64),
                                                     "boxes": e["boxes"].reshape(-1)})))
    return paths


def _sources(tmp_path):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return _examples(np.random.default_rng(0), 12)
    return _toy_shards(tmp_path)


def test_train_loop_checkpoints_resumes_and_keeps_the_backbone(cuda, tmp_path):
    """`train()` on toy records: finite losses every step, head variables move, every MobilenetV1/* variable and moving
    statistic stays bit-identical (frozen backbone), a checkpoint is written, and a second call resumes at the saved
    global_step; the resumed run logs the same losses, bit for bit, as an uninterrupted one (the step has no float atomics
    and no run-to-run freedom, tests/test_retinanet_gpu.py::test_detector_step_replays_from_a_hipgraph)."""
    import torch
    from multiposenet_amd import checkpoint
    from multiposenet_amd import person_detector_model as pdm
    from multiposenet_amd import train_person_detector as tpd
    from multiposenet_amd.detector.input_pipeline import DetectorPipeline
    from multiposenet_amd.net import KeypointNet
    sources = _sources(tmp_path)
    pre = str(tmp_path / "pretrained.npz")
    checkpoint.save_npz(pre, KeypointNet(dtype=torch.bfloat16, seed=9), with_optimizer=False)
    pretrained = {k: v for k, v in np.load(pre).items() if k.startswith("MobilenetV1/")}
    steps, cut = 24, 10
    cfg = {"save_summary_steps": 1, "log_step_count_steps": 8}

    def batches(skip=0):
        def open_():
            it = DetectorPipeline(sources, True, base, seed=6).batches()
            for _ in range(skip):
                next(it)
            return it
        return open_

    def summaries(p):
        return [json.loads(l) for l in open(os.path.join(p["model_dir"], "summaries.jsonl"))]
    base = _params(tmp_path, "unused", pretrained_checkpoint=pre)
    logs = []
    pdm.reset_registry()
    a = dict(base, model_dir=str(tmp_path / "a"))
    head0 = pdm.get_detector(a).state_dict()
    assert tpd.train(a, batches(), run_config=cfg, max_steps=steps, log=logs.append) == steps
    assert any("warm start" in l for l in logs) and os.path.exists(os.path.join(a["model_dir"], f"model.ckpt-{steps}.npz"))
    net = pdm.get_detector(a)
    assert int(net.global_step.item()) == steps
    recs_a = summaries(a)
    assert [r["step"] for r in recs_a] == list(range(1, steps + 1))
    assert all(np.isfinite(v) for r in recs_a for v in r.values())
    head = net.state_dict()
    moved = [k for k in head if not np.array_equal(head[k], head0[k])]
    assert {"class_net/logits/kernel", "box_net/encoded_boxes/kernel", "fpn/lateral5/kernel"} <= set(moved)
    assert len(moved) > len(head) // 2, sorted(set(head) - set(moved))[:5]
    backbone = {k: v for k, v in net.backbone.state_dict().items() if k.startswith("MobilenetV1/")}
    assert len(backbone) == len(pretrained) > 100
    for k, v in backbone.items():                            # variables AND moving statistics, as the warm start left them
        np.testing.assert_array_equal(v, pretrained[k], err_msg=k)
    saved = np.load(os.path.join(a["model_dir"], f"model.ckpt-{steps}.npz"))
    assert int(saved["global_step"]) == steps and set(pretrained) <= set(saved.files) and set(head) <= set(saved.files)
    assert not any(k.startswith("MobilenetV1/") and k.endswith("/Adam") for k in saved.files)
    # interrupted run: `cut` steps, then a fresh process (registry cleared; no pretrained file any more) resumes
    pdm.reset_registry()
    b = dict(base, model_dir=str(tmp_path / "b"))
    assert tpd.train(b, batches(), run_config=cfg, max_steps=cut, log=logs.append) == cut
    pdm.reset_registry()
    b2 = dict(b, pretrained_checkpoint=str(tmp_path / "missing.npz"))
    assert tpd.train(b2, batches(skip=cut), run_config=cfg, max_steps=steps, log=logs.append) == steps
    assert any(f"model.ckpt-{cut}.npz (global_step {cut})" in l for l in logs)
    recs_b = summaries(b)
    assert [r["step"] for r in recs_b] == list(range(1, steps + 1))
    assert recs_b == recs_a                                  # the logged losses of every step, bit for bit
    got = pdm.get_detector(b2).state_dict()
    for k in head:
        np.testing.assert_array_equal(got[k], head[k], err_msg=k)
    pdm.reset_registry()


def test_evaluate_returns_the_metrics_of_the_collected_detections(cuda, tmp_path):
    import torch
    from multiposenet_amd import metrics
    from multiposenet_amd import person_detector_model as pdm
    from multiposenet_amd import train_person_detector as tpd
    from multiposenet_amd.detector.input_pipeline import DetectorPipeline
    from multiposenet_amd.keypoints_model import ModeKeys
    sources = _sources(tmp_path)
    # a score threshold low enough for a barely trained head to detect something
    params = _params(tmp_path, "m", score_threshold=0.005)
    pdm.reset_registry()
    tpd.train(params, lambda: DetectorPipeline(sources, True, params, seed=6).batches(), max_steps=6, log=lambda s: None)

    def val():
        return DetectorPipeline(sources, False, params).batches()
    logs = []
    out = tpd.evaluate(params, val, log=logs.append, step=6)
    names = {"metrics/" + k for k in metrics.METRIC_NAMES}
    assert names <= set(out) and {"localization_loss", "classification_loss", "regularization_loss", "total_loss"} <= set(out)
    assert all(np.isfinite(v) for v in out.values()) and 0 <= out["metrics/AP"] <= 1 and len(logs) == 1
    groundtruth, detections, losses = {}, [], []
    for i, (feats, labels) in enumerate(val()):
        spec = pdm.model_fn(feats, labels, ModeKeys.EVAL, params)
        pred = {k: v.cpu().numpy() for k, v in spec.eval_metric_ops.items()}
        n, m = int(labels["num_boxes"][0]), int(pred["num_boxes"][0])
        groundtruth[str(i)] = labels["boxes"][0, :n].cpu().numpy()
        detections += [(str(i), b, s) for b, s in zip(pred["boxes"][0, :m], pred["scores"][0, :m])]
        losses.append(float(spec.loss))
    assert len(groundtruth) == 12
    want = metrics.evaluate_detector(groundtruth, detections, 0.5)
    print(out, len(detections))
    assert len(detections) > 0
    for k, v in want.items():
        assert out["metrics/" + k] == v, k
    assert abs(out["total_loss"] - np.mean(losses)) <= 1e-6 * abs(np.mean(losses))
    pdm.reset_registry()
