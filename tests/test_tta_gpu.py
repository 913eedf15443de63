"""GPU: test-time augmentation on the device. mpn_mirror_images and mpn_tta_merge against tests/tta_ref.py bit for bit, and
`flip=` / `scales=` of the Detector against the same merge of plain calls: in inference an image's heatmaps do not depend on
its neighbours in the batch (test_detector_batch_gpu.py::test_batch_equals_single_image_calls), so a pass over the batch and
its mirrors is two plain passes, and nothing here needs a tolerance except what lies behind the PRN's split-K contraction."""
import ctypes

import numpy as np
import pytest
import torch

import pil_resize_ref
import plot_maps_ref
import pose_gather_ref
import tta_ref
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, _oracle_prn, models  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape", [(2, 3, 5, 3), (1, 4, 1, 3), (3, 2, 8, 3)])      # odd width; width 1; the batch stride (and
def test_mirror_images(cuda, shape):                                                # the whole-dword path of widths 4k)
    from multiposenet_amd import _lib
    img = np.random.RandomState(sum(shape)).randint(0, 256, shape).astype(np.uint8)
    src = torch.from_numpy(img).to(cuda)
    dst = torch.full(shape, 7, dtype=torch.uint8, device=cuda)
    n, h, w, _ = shape
    _lib.call("mpn_mirror_images", _lib.ptr(src), n, h, w, _lib.ptr(dst), _lib.stream_ptr())
    np.testing.assert_array_equal(dst.cpu().numpy(), img[:, :, ::-1])
    np.testing.assert_array_equal(dst.cpu().numpy(), tta_ref.mirror_images(img))
    np.testing.assert_array_equal(src.cpu().numpy(), img)


def _values(rng, shape):
    """Finite f32 of both signs, magnitudes 1e-6 .. 1e3."""
    return (np.where(rng.rand(*shape) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6, 3, shape)).astype(np.float32)


MERGE_CASES = {
    # name: (batch, [(h_k, w_k, mirrored)]); the first source's size is the output's
    "odd width, plain + mirrored": (2, [(5, 7, False), (5, 7, True)]),
    "up, down and clamp, three sources": (2, [(5, 7, False), (3, 4, False), (9, 13, True)]),
    "eight sources": (1, [(4, 4, False), (4, 4, True), (2, 2, False), (2, 2, True), (8, 8, False), (8, 8, True), (6, 6, False),
                          (6, 6, True)]),
    "one mirrored pixel": (1, [(1, 1, True)]),
}


@pytest.mark.parametrize("name", list(MERGE_CASES))
def test_tta_merge_equals_the_numpy_definition(cuda, name):
    from multiposenet_amd import _lib
    from multiposenet_amd.inference import tta
    b, shapes = MERGE_CASES[name]
    rng = np.random.RandomState(len(name))
    host = [(_values(rng, (b, h, w, 17)), _values(rng, (b, h, w)), m) for h, w, m in shapes]
    assert all(np.isfinite(h).all() and np.isfinite(s).all() and (h < 0).any() and (h > 0).any() for h, s, _ in host)
    dev = [(torch.from_numpy(h).to(cuda), torch.from_numpy(s).to(cuda), m) for h, s, m in host]
    h0, w0 = shapes[0][:2]
    heat = torch.full((b, h0, w0, 17), float("nan"), device=cuda)
    seg = torch.full((b, h0, w0), float("nan"), device=cuda)
    table = (tta.Source * len(dev))()
    for row, (h, s, m) in zip(range(len(dev)), dev):
        table[row].heat, table[row].seg = h.data_ptr(), s.data_ptr()
        table[row].h, table[row].w, table[row].mirrored = h.shape[1], h.shape[2], int(m)
    _lib.call("mpn_tta_merge", ctypes.cast(table, ctypes.c_void_p), len(dev), b, h0, w0, _lib.ptr(heat), _lib.ptr(seg),
              _lib.stream_ptr())
    want_heat, want_seg = tta_ref.merge(host)
    got_heat, got_seg = heat.cpu().numpy(), seg.cpu().numpy()
    assert np.isfinite(want_heat).all() and np.isfinite(want_seg).all()
    np.testing.assert_array_equal(got_heat.view(np.uint32), want_heat.view(np.uint32))
    np.testing.assert_array_equal(got_seg.view(np.uint32), want_seg.view(np.uint32))
    # the module's own launcher is the same call
    heat2, seg2 = torch.empty_like(heat), torch.empty_like(seg)
    tta.merge(dev, heat2, seg2)
    assert torch.equal(heat2, heat) and torch.equal(seg2, seg)


# ------------------------------------------------------------------ the Detector, f32 build, graph on
THR = 0.0


def _maps_of(outs):
    return np.stack([o["keypoint_heatmaps"] for o in outs]), np.stack([o["segmentation_masks"] for o in outs])


def _assert_maps(outs, want, msg):
    heat, seg = _maps_of(outs)
    assert heat.dtype == np.float32 and heat.shape == want[0].shape and seg.shape == want[1].shape, msg
    np.testing.assert_array_equal(heat.view(np.uint32), want[0].view(np.uint32), err_msg=f"{msg} heatmaps")
    np.testing.assert_array_equal(seg.view(np.uint32), want[1].view(np.uint32), err_msg=f"{msg} mask")


@pytest.fixture(scope="module")
def runs(cuda, models):
    """One Detector and the calls the flip tests share: A plain, B plain on the mirrored images, T with flip, then a plain
    call again and a flip call on the reversed batch (both replays)."""
    det = _detector(models)
    images = _images()
    mirrored = np.ascontiguousarray(images[:, :, ::-1])
    r = {"det": det, "images": images}
    r["A"] = det.predict_batch(images, score_threshold=THR)
    r["B"] = det.predict_batch(mirrored, score_threshold=THR)
    n0 = len(det._graphs)
    r["T"] = det.predict_batch(images, score_threshold=THR, flip=True)
    r["flip_graphs"] = len(det._graphs) - n0
    r["A_again"] = det.predict_batch(images, score_threshold=THR)
    r["T_reversed"] = det.predict_batch(np.ascontiguousarray(images[::-1]), score_threshold=THR, flip=True)
    r["graphs_after"] = len(det._graphs) - n0
    return r


def test_flip_equals_the_merge_of_two_plain_calls(runs, models):
    from test_api_gpu import _decided_prn_positions
    det, A, B, T = runs["det"], runs["A"], runs["B"], runs["T"]
    ha, sa = _maps_of(A)
    hb, sb = _maps_of(B)
    _assert_maps(T, tta_ref.merge([(ha, sa, False), (hb, sb, True)]), "flip:")
    for i, (a, t) in enumerate(zip(A, T)):
        assert set(t) == set(a)
        # not vacuous: the averaged maps are not the plain ones (the CPU oracle chain, merged by tta_ref, says so for these
        # seeds: merged and plain heatmaps differ in every value of every image, by up to 0.46; the masks by up to 0.8 - 1.0)
        assert not np.array_equal(t["keypoint_heatmaps"], a["keypoint_heatmaps"]), i
        assert not np.array_equal(t["segmentation_masks"], a["segmentation_masks"]), i
        _assert_same({k: a[k] for k in ("boxes", "scores", "num_boxes")}, {k: t[k] for k in ("boxes", "scores", "num_boxes")},
                     f"flip, image {i}: the boxes are the plain pass's")
        n = len(t["boxes"])
        assert n >= 3
        want = pose_gather_ref.pixel_keypoints(t["boxes"], t["keypoint_scores"], t["keypoint_positions"], H, W)
        assert t["keypoints"].shape == (n, 17, 3) and t["keypoints"].tobytes() == want.tobytes()
        # the PRN read the MERGED maps: the oracle PRN on them, within _compare_batch_with_single's bounds
        crops, wlogits, wsc, wpos = _oracle_prn(models["pvals"], t["keypoint_heatmaps"], t["boxes"])
        assert t["keypoint_scores"].shape == (n, 17) and t["keypoint_positions"].shape == (n, 17, 2)
        np.testing.assert_allclose(t["keypoint_scores"], wsc, rtol=5e-3)
        decided, err = _decided_prn_positions(det, crops, wlogits)
        print(f"\n[flip, image {i}] n {n}, PRN decided {int(decided.sum())} of {decided.size} channels, max |logit diff| {err:.2e}")
        assert err < 1e-3 and np.any(crops != 0) and decided.mean() >= 0.5
        assert np.all(t["keypoint_positions"] == wpos, axis=-1)[decided].all()


def test_flip_has_a_graph_of_its_own_and_replays(runs):
    assert runs["flip_graphs"] == 1 and runs["graphs_after"] == 1
    for i, (a, b) in enumerate(zip(runs["A_again"], runs["A"])):
        _assert_same(a, b, f"plain after flip, image {i}:")
    for i, (a, b) in enumerate(zip(runs["T_reversed"], runs["T"][::-1])):
        _assert_same(a, b, f"flip on the reversed batch, image {i}:")


def _scale_sources(det, x0, scales, flip):
    """The merge sources of the stated construction: plain predict_batch on x0, on its mirror, on x0 resized by Pillow's
    bicubic to each (width, height) of scales, on that one's mirror, ..."""
    sources = []
    for wk, hk in [(x0.shape[2], x0.shape[1])] + list(scales):
        xk = x0 if (hk, wk) == x0.shape[1:3] else np.stack([pil_resize_ref.resize(im, hk, wk) for im in x0])
        sources.append(_maps_of(det.predict_batch(xk, score_threshold=THR)) + (False,))
        if flip:
            sources.append(_maps_of(det.predict_batch(np.ascontiguousarray(xk[:, :, ::-1]), score_threshold=THR)) + (True,))
    return sources


def test_scales_and_flip_through_predict_images(cuda, models):
    det = _detector(models)
    rng = np.random.RandomState(3)
    frames = [rng.randint(0, 256, (200, 300, 3)).astype(np.uint8), rng.randint(0, 256, (333, 250, 3)).astype(np.uint8)]
    scales = [(128, 128), (384, 384)]
    got = det.predict_images(frames, size=(256, 256), scales=scales, flip=True, return_heatmaps=True, score_threshold=THR)
    x0 = np.stack([pil_resize_ref.resize(f, 256, 256) for f in frames])
    sources = _scale_sources(det, x0, scales, True)
    assert [s[0].shape[1:3] for s in sources] == [(64, 64)] * 2 + [(32, 32)] * 2 + [(96, 96)] * 2
    _assert_maps(got, tta_ref.merge(sources), "predict_images, scales + flip:")
    plain = det.predict_images(frames, size=(256, 256), return_heatmaps=True, score_threshold=THR)
    for i, (a, t) in enumerate(zip(plain, got)):
        assert set(t) == set(a) and t["resized_size"] == a["resized_size"]
        assert not np.array_equal(t["keypoint_heatmaps"], a["keypoint_heatmaps"]), i
        _assert_same({k: a[k] for k in ("boxes", "scores", "num_boxes")}, {k: t[k] for k in ("boxes", "scores", "num_boxes")},
                     f"scales + flip, image {i}: the boxes are the plain pass's")


def test_scales_through_predict_batch(runs):
    """The batch is 384 x 256 (width x height): the nearest other size with that aspect ratio whose sides are multiples of
    128 is 768 x 512 (a smaller one does not exist: 192 x 128 is no network input)."""
    det, images = runs["det"], runs["images"]
    got = det.predict_batch(images, score_threshold=THR, scales=[(768, 512)])
    sources = _scale_sources(det, images, [(768, 512)], False)
    assert [s[0].shape[1:3] for s in sources] == [(64, 96), (128, 192)]
    _assert_maps(got, tta_ref.merge(sources), "predict_batch, scales:")
    for i, (a, t) in enumerate(zip(runs["A"], got)):
        _assert_same({k: a[k] for k in ("boxes", "scores", "num_boxes")}, {k: t[k] for k in ("boxes", "scores", "num_boxes")},
                     f"scales, image {i}: the boxes are the plain pass's")
    with pytest.raises(ValueError, match="aspect"):
        det.predict_batch(images, scales=[(128, 128)])
    with pytest.raises(ValueError, match="multiples of 128"):
        det.predict_batch(images, scales=[(192, 128)])


def test_plot_maps_reads_the_merged_maps(runs):
    from multiposenet_amd.inference import plot_maps
    det, images, T = runs["det"], runs["images"], runs["T"]
    got = det.predict_batch(images, score_threshold=THR, flip=True, plot_maps=True)
    for i, (o, t) in enumerate(zip(got, T)):
        _assert_same({k: v for k, v in o.items() if k != "maps"}, t, f"plot_maps + flip vs flip, image {i}:")
        want = plot_maps(images[i], plot_maps_ref.normalise(t["keypoint_heatmaps"]), t["segmentation_masks"])
        assert o["maps"].shape == want.shape and np.array_equal(o["maps"], want), i
        plain = plot_maps(images[i], plot_maps_ref.normalise(runs["A"][i]["keypoint_heatmaps"]), runs["A"][i]["segmentation_masks"])
        assert not np.array_equal(o["maps"], plain), i


def test_models_without_a_detector_or_without_heatmaps(runs, models):
    images, T = runs["images"], runs["T"]
    bare = _detector(models, detector=False, prn=False)
    for i, o in enumerate(bare.predict_batch(images, flip=True)):
        assert o["num_boxes"] == 0 and o["boxes"].shape == (0, 4)
        np.testing.assert_array_equal(o["keypoint_heatmaps"], T[i]["keypoint_heatmaps"])
        np.testing.assert_array_equal(o["segmentation_masks"], T[i]["segmentation_masks"])
    bare._has_heatmaps = lambda: False                                  # a graph without the heatmap head
    for kw in ({"flip": True}, {"scales": [(768, 512)]}):
        with pytest.raises(ValueError, match="heatmap"):
            bare.predict_batch(images, **kw)
    with pytest.raises(ValueError, match="heatmap"):
        bare.predict_images(list(images), size=(256, 256), flip=True)
