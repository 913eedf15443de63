"""GPU: Detector.predict_images - ragged frames resized on the device inside the captured graph - against predict_batch on the
restatement-resized batch (tests/pil_resize_ref.py) with the numpy mapping to source coordinates, and its hipGraph behaviour.

Sources: one IMAGE_SEEDS image already at the network size (an identity resize is an exact copy: it keeps the 12 boxes that
test_detector_batch_gpu.py documents) and seeded random images of other sizes. Their seeds were checked with the oracle chain
alone (on the CPU, `_oracle_image` of that file on the restatement-resized image, as its header describes): for every size used
here and seeds 1-6, with and without keep_aspect_ratio, the resized image keeps 12 to 14 boxes, the weakest score 0.34 - none on
the 0.3 edge of the NMS."""
import numpy as np
import pytest
import torch

import image_gather_ref as G
import pil_resize_ref as P
from multiposenet_amd.inference import resample
from test_detector_batch_gpu import IMAGE_SEEDS, _assert_same, _detector, _images, _variables, models  # noqa: F401

pytestmark = pytest.mark.gpu

H, W = 256, 384
SHAPES_A = [(300, 500), (97, 131), (480, 640)]
SHAPES_B = [(120, 100), (470, 650), (310, 490)]       # fits the capacity of A: fewer bytes, rows and table words


def _sources(shapes, seeds, identity_at):
    out = [np.random.RandomState(s).randint(0, 256, (h, w, 3)).astype(np.uint8) for (h, w), s in zip(shapes, seeds)]
    out.insert(identity_at, _images(IMAGE_SEEDS[:1])[0])
    return out


def _expected(det, sources, keep, thr, heat=False):
    """predict_batch on the restatement-resized batch (same b: the same split-K order in the PRN), mapped with numpy."""
    batch = np.stack([P.canvas(s, H, W, keep) for s in sources])
    outs = det.predict_batch(batch, score_threshold=thr, return_heatmaps=heat)
    want = []
    for s, o in zip(sources, outs):
        nh, nw = resample.resized_size(s.shape[0], s.shape[1], H, W, keep)
        m = G.map_person(o, resample.extent_of(s.shape[0], s.shape[1], nh, nw, H, W))
        if heat:
            m["resized_size"] = (nh, nw)
        want.append(m)
    return want


def _compare(got, want, msg):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = dict(a), dict(b)
        assert a.pop("resized_size", None) == b.pop("resized_size", None)
        _assert_same(a, b, f"{msg} image {i}:")
        assert len(a["boxes"]) >= 3, (msg, i, len(a["boxes"]))
        assert a["keypoints"].shape == (len(a["boxes"]), 17, 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("keep", [False, True])
def test_predict_images_equals_predict_batch_on_the_resized_batch(cuda, models, dtype, keep):
    det, ref_det = _detector(models, dtype=dtype), _detector(models, dtype=dtype)
    sources = _sources(SHAPES_A, (1, 2, 3), 1)
    got = det.predict_images(sources, size=(H, W), keep_aspect_ratio=keep, score_threshold=0.05)
    want = _expected(ref_det, sources, keep, 0.05)
    assert set(got[0]) == {"boxes", "scores", "num_boxes", "keypoint_scores", "keypoint_positions", "keypoints"}
    _compare(got, want, f"{dtype} keep={keep}")
    # the identity-sized source is an exact copy: its boxes are those of predict_batch on the image itself, unscaled
    np.testing.assert_array_equal(got[1]["boxes"], ref_det.predict_batch(np.stack([P.canvas(s, H, W, keep) for s in sources]),
                                                                         score_threshold=0.05)[1]["boxes"])
    if keep:
        assert any(not np.array_equal(a["boxes"], b["boxes"]) for a, b in
                   zip(got, ref_det.predict_batch(np.stack([P.canvas(s, H, W, keep) for s in sources]), score_threshold=0.05)))
    with_maps = det.predict_images(sources, size=(H, W), keep_aspect_ratio=keep, score_threshold=0.05, return_heatmaps=True)
    _compare(with_maps, _expected(ref_det, sources, keep, 0.05, heat=True), "heatmaps")
    assert with_maps[0]["keypoint_heatmaps"].shape == (H // 4, W // 4, 17) and with_maps[0]["resized_size"] == \
        resample.resized_size(300, 500, H, W, keep)


def test_predict_images_graph_behaviour(cuda, models):
    det, eager, ref_det = _detector(models), _detector(models, graph=False), _detector(models)
    a, b = _sources(SHAPES_A, (1, 2, 3), 1), _sources(SHAPES_B, (4, 5, 6), 3)
    fixed = _images()
    batch_before = det.predict_batch(fixed, score_threshold=0.0)
    call_before = det(fixed[0], score_threshold=0.0)
    n0 = len(det._graphs)
    got_a = det.predict_images(a, size=(H, W))
    assert len(det._graphs) == n0 + 1
    _compare(got_a, _expected(ref_det, a, False, 0.05), "first call")
    got_b = det.predict_images(b, size=(H, W))                                    # other sizes, same capacity: the same graph
    assert len(det._graphs) == n0 + 1
    _compare(got_b, _expected(ref_det, b, False, 0.05), "second call, same graph")
    _compare(det.predict_images(a, size=(H, W)), got_a, "back to the first sizes")
    for x, y in zip(eager.predict_images(b, size=(H, W)), got_b):                 # use_graph False: identical results
        _assert_same(x, y, "graph vs eager:")
    assert not eager._graphs
    big = [np.random.RandomState(9).randint(0, 256, (1080, 1920, 3)).astype(np.uint8)] + a[1:]
    keys_before = set(det._graphs)
    got_big = det.predict_images(big, size=(H, W))                                # exceeds the capacity: a new graph
    added, dropped = set(det._graphs) - keys_before, keys_before - set(det._graphs)
    assert len(added) == 1 and len(dropped) == 1                                  # one new graph; the superseded one is freed
    assert next(iter(added))[:5] == next(iter(dropped))[:5] == ("images", 4, H, W, 0.05)
    want_big = _expected(ref_det, big, False, 0.05)
    _assert_same(got_big[0], want_big[0], "larger capacity, the 1080 x 1920 source:")   # (its seed was not chosen for boxes)
    _compare(got_big[1:], want_big[1:], "larger capacity")
    _compare(det.predict_images(a, size=(H, W)), got_a, "small batch through the larger buffers")
    assert len(det._graphs) == n0 + 1
    for x, y in zip(det.predict_batch(fixed, score_threshold=0.0), batch_before):
        _assert_same(x, y, "predict_batch after predict_images:")
    _assert_same(det(fixed[0], score_threshold=0.0), call_before, "__call__ after predict_images:")


def test_ragged_paths_follow_reloaded_variables(cuda, models):
    """predict_images and predict_jpegs replay a captured graph whose batch-norm affines and operand casts are cached on the host:
    after load_state_dict the same graph must give, exactly, what a fresh eager Detector on the new variables gives. Needs no
    detections (canvas 128 x 128, class bias -6): the heatmaps and num_boxes carry the comparison."""
    from multiposenet_amd.inference import Detector
    from test_jpeg_host import goldens
    g = goldens()
    jpegs = [g[name][0] for name in ("1x1_420", "8x8_444")]       # the smallest 4:2:0 and the smallest 4:4:4 decode golden
    frames = [np.random.RandomState(s).randint(0, 256, (h, w, 3)).astype(np.uint8) for s, (h, w) in ((1, (128, 128)), (2, (97, 131)))]
    bb2, hp2, _ = _variables(seed=47, class_seed=47)
    fresh = Detector(bb2, dtype=torch.float32, detector_path=hp2, prn_path=models["paths"]["p"])
    fresh.use_graph = False
    kwargs = dict(size=(128, 128), return_heatmaps=True, score_threshold=0.0)
    # (a Detector per method: both share the graph entry, and each first call must be a capture)
    for method, sources in (("predict_images", frames), ("predict_jpegs", jpegs)):
        det = _detector(models, dtype=torch.float32)
        first = getattr(det, method)(sources, **kwargs)
        keys = set(det._graphs)
        det.net.load_state_dict(bb2)
        own = set(det.retinanet.vars) | set(det.retinanet.stats)
        det.retinanet.load_state_dict({k: v for k, v in hp2.items() if k in own})
        got = getattr(det, method)(sources, **kwargs)
        assert set(det._graphs) == keys and len(keys) == 1                         # the same graph, refreshed caches
        want = getattr(fresh, method)(sources, **kwargs)
        assert len(got) == len(want) == 2
        for a, b in zip(got, want):
            _assert_same(a, b, f"{method} after load_state_dict:")
        assert not np.array_equal(got[0]["keypoint_heatmaps"], first[0]["keypoint_heatmaps"])
