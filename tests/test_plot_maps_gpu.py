"""GPU: mpn_plot_maps, `plot_maps` / `MapPlotter` and the `plot_maps=True` paths of the Detector against the golden pictures
the reference notebook made under Pillow and matplotlib and against the numpy restatement tests/plot_maps_ref.py (proven
against them on the CPU, tests/test_plot_maps_host.py). Equality is every byte of every picture. Run it in a process of its
own under a time limit, e.g.

    timeout -k 10 600 python -m pytest -m gpu tests/test_plot_maps_gpu.py
"""
import numpy as np
import pytest
import torch

import pil_resize_ref as P
import plot_maps_ref as R
from test_detector_batch_gpu import _assert_same, _detector, _images, _variables, models  # noqa: F401
from test_plot_maps_host import goldens

pytestmark = pytest.mark.gpu

F = np.float32
SIZE = (128, 128)


def test_plot_maps_equals_every_golden(cuda):
    from multiposenet_amd.inference import MapPlotter, plot_maps
    for name, img, heat, mask, want in goldens():
        with np.errstate(invalid="ignore"):
            got = plot_maps(img, heat, mask)
        assert got.dtype == np.uint8 and got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int((got != want).any(-1).sum()), np.argwhere((got != want).any(-1))[:5].tolist())
        plotter = MapPlotter(1, *img.shape[:2], *heat.shape[:2])
        plotter.out.fill_(7)                                        # every byte of the output is written
        assert np.array_equal(plotter(img[None], heat[None], mask[None])[0], want), name


def test_normalised_heatmaps_equal_the_restatement(cuda):
    """normalise=True is notebook cell 20 on the device: (h - m) / (M - m) per frame and channel; a flat channel is NaN."""
    from multiposenet_amd.inference import MapPlotter
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (2, 72, 88, 3)).astype(np.uint8)
    heat = (1 / (1 + np.exp(-rng.randn(2, 18, 22, 17) * 3))).astype(F)
    heat[0, ..., 3] = F(0.25)                                       # M == m
    mask = rng.randn(2, 18, 22).astype(F)
    got = MapPlotter(2, 72, 88, 18, 22)(img, heat, mask, normalise=True)
    for i in range(2):
        assert np.array_equal(got[i], R.plot_maps(img[i], R.normalise(heat[i]), mask[i])), i


def test_a_batch_equals_single_calls_and_runs_are_bit_identical(cuda):
    from multiposenet_amd.inference import MapPlotter, plot_maps
    rng = np.random.RandomState(11)
    img = rng.randint(0, 256, (3, 70, 1030, 3)).astype(np.uint8)    # w = 515: more than one block per row, no multiple of 4
    heat = (rng.uniform(0, 1, (3, 18, 258, 17)) ** 2).astype(F)
    mask = rng.uniform(-0.2, 1.2, (3, 18, 258)).astype(F)
    plotter = MapPlotter(3, 70, 1030, 18, 258)
    got = plotter(img, heat, mask)
    assert got.shape == (3, 18 * 35, 515, 4)
    assert np.array_equal(got, plotter(img, heat, mask))
    for i in range(3):
        assert np.array_equal(got[i], plot_maps(img[i], heat[i], mask[i])), i
    assert np.array_equal(got[1], R.plot_maps(img[1], heat[1], mask[1]))
    assert not np.array_equal(got[0], got[1])


def _check_maps(outs, frames, msg):
    for i, (o, frame) in enumerate(zip(outs, frames)):
        assert o["maps"].dtype == np.uint8 and o["maps"].shape == (18 * SIZE[0] // 2, SIZE[1] // 2, 4), (msg, i)
        want = R.plot_maps(frame, R.normalise(o["keypoint_heatmaps"]), o["segmentation_masks"])
        assert np.array_equal(o["maps"], want), (msg, i, int((o["maps"] != want).any(-1).sum()))


def _without(outs, *keys):
    return [{k: v for k, v in o.items() if k not in keys} for o in outs]


def test_predict_batch_plot_maps(cuda, models):
    det, eager = _detector(models), _detector(models, graph=False)
    images = _images((12, 15), *SIZE)
    plain = det.predict_batch(images, score_threshold=0.05)
    n0 = len(det._graphs)
    got = det.predict_batch(images, score_threshold=0.05, plot_maps=True, return_heatmaps=True)
    assert len(det._graphs) == n0 + 1 and set(got[0]) == set(plain[0]) | {"maps"}
    _check_maps(got, images, "predict_batch")
    assert not np.array_equal(got[0]["maps"], got[1]["maps"])
    for a, b in zip(_without(got, "maps"), plain):
        _assert_same(a, b, "plot_maps=True vs False:")
    bare = det.predict_batch(images, score_threshold=0.05, plot_maps=True, return_heatmaps=False)     # a replay
    assert "keypoint_heatmaps" not in bare[0] and len(det._graphs) == n0 + 1
    for a, b, c in zip(bare, got, eager.predict_batch(images, score_threshold=0.05, plot_maps=True)):
        np.testing.assert_array_equal(a["maps"], b["maps"])
        _assert_same(c, b, "eager vs replay:")
    assert not eager._graphs
    both = det.predict_batch(images, score_threshold=0.05, plot_maps=True, annotate=True)
    drawn = det.predict_batch(images, score_threshold=0.05, annotate=True)
    for a, b, c in zip(both, got, drawn):
        np.testing.assert_array_equal(a["maps"], b["maps"])
        np.testing.assert_array_equal(a["annotated"], c["annotated"])
        _assert_same({k: v for k, v in a.items() if k != "maps"}, c, "plot_maps + annotate vs annotate:")
    for a, b in zip(det.predict_batch(images, score_threshold=0.05), plain):        # plot_maps=False is what it was
        _assert_same(a, b, "plot_maps=False after plot_maps=True:")


def test_predict_images_and_jpegs_plot_maps(cuda, models):
    from multiposenet_amd.inference import jpeg as J
    from test_jpeg_host import goldens as jpeg_goldens
    det = _detector(models)
    sources = [np.random.RandomState(s).randint(0, 256, (h, w, 3)).astype(np.uint8) for s, (h, w) in ((1, (96, 70)), (2, (40, 128)))]
    kwargs = {"size": SIZE, "keep_aspect_ratio": True, "score_threshold": 0.05}
    plain = det.predict_images(sources, return_heatmaps=True, **kwargs)
    got = det.predict_images(sources, plot_maps=True, return_heatmaps=True, **kwargs)
    assert set(got[0]) == set(plain[0]) | {"maps"}
    _check_maps(got, [P.canvas(s, *SIZE, True) for s in sources], "predict_images")
    for a, b in zip(_without(got, "maps"), plain):
        _assert_same(a, b, "plot_maps=True vs False:")
    for a, b in zip(det.predict_images(sources, plot_maps=True, **kwargs), got):
        assert "keypoint_heatmaps" not in a
        np.testing.assert_array_equal(a["maps"], b["maps"])
    for a, b in zip(det.predict_images(sources, return_heatmaps=True, **kwargs), plain):
        _assert_same(a, b, "plot_maps=False after plot_maps=True:")
    g = jpeg_goldens()
    files = [g["120x160_422_checker"][0], g["37x53_gray"][0]]
    frames = [J.pillow_decode(j) for j in files]
    plain = det.predict_jpegs(files, return_heatmaps=True, **kwargs)
    got = det.predict_jpegs(files, plot_maps=True, return_heatmaps=True, **kwargs)
    _check_maps(got, [P.canvas(f, *SIZE, True) for f in frames], "predict_jpegs")
    for a, b in zip(_without(got, "maps"), plain):
        _assert_same(a, b, "plot_maps=True vs False:")
    for a, b in zip(det.predict_jpegs(files, return_heatmaps=True, **kwargs), plain):
        _assert_same(a, b, "plot_maps=False after plot_maps=True:")
