"""GPU: mpn_draw_detections and the `annotate=True` paths of the Detector against the numpy restatement tests/draw_ref.py
(proven against Pillow on the CPU, tests/test_draw_host.py). Equality is every byte of every frame; nothing here reads Pillow
or anything outside the repository. Run it in a process of its own under a time limit, e.g.

    timeout -k 10 900 python -m pytest -m gpu tests/test_draw_gpu.py
"""
import numpy as np
import pytest
import torch

import draw_ref as R
import pose_gather_ref as G
from test_detector_batch_gpu import IMAGE_SEEDS, _assert_same, _detector, _images, _variables, models  # noqa: F401
from test_draw_host import goldens
from test_predict_images_gpu import SHAPES_A, SHAPES_B, _sources

pytestmark = pytest.mark.gpu

F = np.float32
H, W = 256, 384
MAX_BOXES = 25


def _record(persons, max_boxes):
    """mpn_pose_gather's record for b images whose kept persons are `persons` [(boxes, keypoint_positions)]."""
    b = len(persons)
    rec = np.zeros(G.record_bytes(b, max_boxes), np.uint8)
    header = rec[:G.header_words(b) * 4].view(np.int32)
    rows = rec[G.header_words(b) * 4:].view(G.ROW)
    at = 0
    for i, (boxes, pos) in enumerate(persons):
        n = len(boxes)
        assert n <= max_boxes
        rows["image_index"][at:at + n] = i
        rows["box"][at:at + n] = boxes
        rows["keypoint_positions"][at:at + n] = pos
        header[1 + i] = header[1 + b + i] = n
        at += n
    header[0] = at
    return rec


def _draw(images, persons, max_boxes=MAX_BOXES, with_keypoints=True):
    """The kernel on a ragged batch packed as predict_images packs it -> the frames."""
    from multiposenet_amd.inference import draw
    dev = torch.device("cuda:0")
    offsets = np.concatenate([[0], np.cumsum([im.size for im in images])]).astype(np.int64)
    packed = np.concatenate([im.reshape(-1) for im in images] + [np.zeros(4, np.uint8)])
    buffers = draw.Buffers(len(images), max_boxes, packed.size, dev)
    buffers.out.fill_(7)                                            # every byte of a frame is written
    buffers.place([im.shape[:2] for im in images], offsets[:-1].tolist())
    out = buffers.launch(torch.from_numpy(packed).to(dev), torch.from_numpy(_record(persons, max_boxes)).to(dev), with_keypoints)
    torch.cuda.synchronize()
    return buffers.unpack(out.cpu().numpy())


def _want(image, boxes, pos):
    return R.draw_everything(image, {"boxes": boxes, "keypoint_positions": pos})


def test_kernel_equals_the_restatement_on_every_golden_case(cuda):
    cases = goldens()
    images = [img for _, img, _, _ in cases]
    persons = [(o["boxes"], o["keypoint_positions"]) for _, _, o, _ in cases]
    got = _draw(images, persons)                                    # ONE ragged batch of all cases
    for (name, img, o, golden), frame in zip(cases, got):
        assert frame.dtype == np.uint8 and frame.shape == golden.shape
        np.testing.assert_array_equal(frame, _want(img, o["boxes"], o["keypoint_positions"]), err_msg=name)
        np.testing.assert_array_equal(frame, golden, err_msg=name)  # and what the notebook drew under Pillow
    # one by one (b = 1, another packing) and boxes only
    for name, img, o, golden in cases[:5]:
        np.testing.assert_array_equal(_draw([img], [(o["boxes"], o["keypoint_positions"])])[0], golden, err_msg=name)
        only = _draw([img], [(o["boxes"], o["keypoint_positions"])], with_keypoints=False)[0]
        np.testing.assert_array_equal(only, _want(img, o["boxes"], np.zeros((0, 17, 2), F)), err_msg=name)


def _random_persons(rng, n):
    """Boxes partly outside the frame, positions partly outside the box, some persons pushed to the top-left corner so
    that dots fall at x, y < 2 and below zero."""
    y = np.sort(rng.uniform(-0.15, 1.15, (n, 2)), axis=1)
    x = np.sort(rng.uniform(-0.15, 1.15, (n, 2)), axis=1)
    boxes = np.stack([y[:, 0], x[:, 0], y[:, 1], x[:, 1]], axis=1).astype(F)
    pos = rng.uniform(-0.4, 1.4, (n, 17, 2)).astype(F)
    for i in range(0, n, 4):
        boxes[i] = (boxes[i] * F(0.02)).astype(F)
        boxes[i, :2] = np.minimum(boxes[i, :2], 0)
        pos[i] = rng.uniform(-0.2, 1.0, (17, 2)).astype(F)
    return boxes, pos


@pytest.mark.parametrize("seed,shapes", [
    (1, [(1080, 1920), (97, 131), (480, 640), (1, 1), (1080, 1919), (33, 1025), (720, 1280), (5, 3),
         (300, 500), (299, 501), (64, 64), (1023, 7), (2, 2047), (121, 121), (600, 800), (17, 4099)]),
    (2, [(111, 77), (1, 33), (250, 3), (480, 641), (37, 53)]),
    (3, [(1079, 1921)]),
])
def test_kernel_equals_the_restatement_on_seeded_random_batches(cuda, seed, shapes):
    rng = np.random.RandomState(seed)
    counts = ([0, 25, 1] + [int(v) for v in rng.randint(0, 26, len(shapes))])[:len(shapes)] if len(shapes) > 1 else [25]
    images, persons = [], []
    for (h, w), n in zip(shapes, counts):
        images.append(rng.randint(0, 255, (h, w, 3)).astype(np.uint8))
        persons.append(_random_persons(rng, n))
    got = _draw(images, persons)
    for i, (img, (boxes, pos), frame) in enumerate(zip(images, persons, got)):
        want = _want(img, boxes, pos)
        diff = (frame != want).any(axis=2)
        assert not diff.any(), (seed, i, img.shape, len(boxes), int(diff.sum()), np.argwhere(diff)[:5].tolist())
    again = _draw(images, persons)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)                         # bit-identical from run to run


def _check_annotated(outs, frames, msg):
    drawn = 0
    for i, (o, frame) in enumerate(zip(outs, frames)):
        a = o["annotated"]
        assert a.dtype == np.uint8 and a.shape == frame.shape[:2] + (4,), (msg, i)
        np.testing.assert_array_equal(a, R.draw_everything(frame, o), err_msg=f"{msg} image {i}")
        drawn += int((a[..., :3] != frame).any(axis=2).sum())
    return drawn


def _same_but_annotated(with_a, without, msg):
    for a, b in zip(with_a, without):
        a = dict(a)
        a.pop("annotated")
        _assert_same(a, b, msg)


def test_predict_batch_annotate(cuda, models):
    det, eager = _detector(models), _detector(models, graph=False)
    images, images2 = _images(), _images((4, 5, 8, 9))
    plain = det.predict_batch(images, score_threshold=0.05)
    n0 = len(det._graphs)
    got = det.predict_batch(images, score_threshold=0.05, annotate=True)
    assert len(det._graphs) == n0 + 1 and set(got[0]) == set(plain[0]) | {"annotated"}
    assert _check_annotated(got, images, "predict_batch") > 1000 and all(len(o["boxes"]) >= 3 for o in got)
    _same_but_annotated(got, plain, "annotate=True vs False:")
    got2 = det.predict_batch(images2, score_threshold=0.05, annotate=True)          # replay on other images
    _check_annotated(got2, images2, "predict_batch replay")
    again = det.predict_batch(images, score_threshold=0.05, annotate=True)          # two replays are equal
    for a, b, c in zip(got, again, eager.predict_batch(images, score_threshold=0.05, annotate=True)):
        _assert_same(a, b, "replay vs replay:")
        _assert_same(a, c, "replay vs eager:")
    assert len(det._graphs) == n0 + 1 and not eager._graphs
    for a, b in zip(det.predict_batch(images, score_threshold=0.05), plain):        # annotate=False is what it was
        _assert_same(a, b, "annotate=False after annotate=True:")
    assert len(det._graphs) == n0 + 1
    # no PRN: boxes only; no detector: the frames with alpha 255
    noprn = _detector(models, prn=False).predict_batch(images, score_threshold=0.05, annotate=True)
    assert _check_annotated(noprn, images, "no PRN") > 100 and noprn[0]["keypoint_positions"].shape == (0, 17, 2)
    for o, img in zip(_detector(models, detector=False, prn=False).predict_batch(images, annotate=True), images):
        np.testing.assert_array_equal(o["annotated"][..., :3], img)
        assert (o["annotated"][..., 3] == 255).all()


@pytest.mark.parametrize("keep", [False, True])
def test_predict_images_annotate(cuda, models, keep):
    det = _detector(models)
    sources = _sources(SHAPES_A, (1, 2, 3), 1)
    plain = det.predict_images(sources, size=(H, W), keep_aspect_ratio=keep)
    got = det.predict_images(sources, size=(H, W), keep_aspect_ratio=keep, annotate=True)
    assert set(got[0]) == set(plain[0]) | {"annotated"}
    assert _check_annotated(got, sources, f"predict_images keep={keep}") > 1000 and all(len(o["boxes"]) >= 3 for o in got)
    _same_but_annotated(got, plain, "annotate=True vs False:")
    with_maps = det.predict_images(sources, size=(H, W), keep_aspect_ratio=keep, annotate=True, return_heatmaps=True)
    for a, b in zip(with_maps, got):
        np.testing.assert_array_equal(a["annotated"], b["annotated"])
        assert "keypoint_heatmaps" in a


def test_predict_images_annotate_graph_behaviour(cuda, models):
    det, eager = _detector(models), _detector(models, graph=False)
    a, b = _sources(SHAPES_A, (1, 2, 3), 1), _sources(SHAPES_B, (4, 5, 6), 3)
    plain_a = det.predict_images(a, size=(H, W))
    n0 = len(det._graphs)
    got_a = det.predict_images(a, size=(H, W), annotate=True)
    assert len(det._graphs) == n0 + 1
    _check_annotated(got_a, a, "first call")
    got_b = det.predict_images(b, size=(H, W), annotate=True)                       # other sizes, same capacity: the same graph
    assert len(det._graphs) == n0 + 1
    _check_annotated(got_b, b, "second call, same graph")
    for x, y in zip(det.predict_images(a, size=(H, W), annotate=True), got_a):      # two replays are equal
        _assert_same(x, y, "back to the first sizes:")
    for x, y in zip(eager.predict_images(b, size=(H, W), annotate=True), got_b):    # eager equals replay
        _assert_same(x, y, "graph vs eager:")
    assert not eager._graphs
    big = [np.random.RandomState(9).randint(0, 256, (1080, 1920, 3)).astype(np.uint8)] + a[1:]
    keys_before = set(det._graphs)
    got_big = det.predict_images(big, size=(H, W), annotate=True)                   # exceeds the capacity: a new graph
    added, dropped = set(det._graphs) - keys_before, keys_before - set(det._graphs)
    assert len(added) == 1 and len(dropped) == 1
    assert next(iter(added))[-1] == next(iter(dropped))[-1] == "annotate" and next(iter(added))[:5] == ("images", 4, H, W, 0.05)
    _check_annotated(got_big, big, "larger capacity")
    _check_annotated(det.predict_images(a, size=(H, W), annotate=True), a, "small batch through the larger buffers")
    assert len(det._graphs) == n0 + 1
    for x, y in zip(det.predict_images(a, size=(H, W)), plain_a):                   # annotate=False is what it was
        _assert_same(x, y, "annotate=False after annotate=True:")
    assert len(det._graphs) == n0 + 1


def test_draw_everything_on_a_call_result(cuda, models):
    from multiposenet_amd.inference import draw_everything
    det = _detector(models)
    image = _images()[0]
    outputs = det(image, score_threshold=0.05)
    assert len(outputs["boxes"]) >= 3 and outputs["keypoint_positions"].shape[0] == len(outputs["boxes"])
    got = draw_everything(image, outputs)
    assert got.dtype == np.uint8 and got.shape == (H, W, 4)
    np.testing.assert_array_equal(got, R.draw_everything(image, outputs))
    assert (got[..., :3] != image).any()
    for name, img, o, golden in goldens():
        np.testing.assert_array_equal(draw_everything(img, o), golden, err_msg=name)
    np.testing.assert_array_equal(draw_everything(image, {"boxes": outputs["boxes"], "keypoint_positions": np.zeros((0, 17, 2), F)}),
                                  R.draw_everything(image, {"boxes": outputs["boxes"], "keypoint_positions": np.zeros((0, 17, 2), F)}))
