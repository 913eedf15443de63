"""CPU: `inference.Anonymize`, the keys of the Detector's entries with `anonymize=`, the argument checks, the reference
tests/anonymize_ref.py against Pillow where Pillow draws the same thing and its own properties, and the argument checks of the C
entry point, which run before any HIP call."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import anonymize_cases as C
import anonymize_ref as R
from multiposenet_amd import _lib
from multiposenet_amd.inference import Anonymize, Detector, PoseNms
from multiposenet_amd.inference import anonymize_stage
from test_detector_options_host import B, CAP, H, SERIAL, STYLE, THR, W, _detector, _key_of, _table, _tracker

F = np.float32
DEFAULTS = dict(region='head', mode='pixelate', shape='ellipse', blocks=8, radius=8, color=(0, 0, 0), scale=2.0, min_size=0.1,
                fallback=0.25, min_keypoint_score=0.0, overlay=True)


# ------------------------------------------------------------------ the parameter class
def test_defaults_repr_equality_and_immutability():
    a = Anonymize()
    assert list(Anonymize.__slots__) == list(DEFAULTS) and a.astuple() == tuple(DEFAULTS.values())
    assert list(inspect.signature(Anonymize).parameters) == list(DEFAULTS)
    assert repr(a) == ("Anonymize(region='head', mode='pixelate', shape='ellipse', blocks=8, radius=8, color=(0, 0, 0), scale=2.0, "
                       "min_size=0.1, fallback=0.25, min_keypoint_score=0.0, overlay=True)")
    assert not hasattr(a, '__dict__')
    assert a == Anonymize(**DEFAULTS) and hash(a) == hash(Anonymize(**DEFAULTS)) and a != a.astuple()
    changed = dict(region='box', mode='blur', shape='rectangle', blocks=9, radius=3, color=(0, 0, 1), scale=2.5, min_size=0.0,
                   fallback=1.0, min_keypoint_score=0.5, overlay=False)
    for name, value in changed.items():
        other = Anonymize(**{name: value})
        assert other != a and getattr(other, name) == value, name
    assert len({a, Anonymize(), Anonymize(blocks=9)}) == 2
    assert Anonymize(color=[1, 2, 3]).color == (1, 2, 3) and Anonymize(color=np.array([4, 5, 6])).color == (4, 5, 6)
    assert Anonymize(min_keypoint_score=0.1).min_keypoint_score == float(np.float32(0.1))      # what the launch compares against
    assert Anonymize(min_keypoint_score=-3).min_keypoint_score == -3.0
    for change in (lambda: setattr(a, 'blocks', 4), lambda: setattr(a, 'other', 1), lambda: delattr(a, 'blocks')):
        with pytest.raises(AttributeError, match="^Anonymize is immutable$"):
            change()
    assert "NOT tuned" in Anonymize.__doc__
    p = Anonymize(color=(1, 2, 3), mode='fill', region='box', shape='rectangle', min_keypoint_score=0.25).params()
    assert (p.region, p.mode, p.shape, p.blocks, p.radius, p.color) == (1, 2, 1, 8, 8, 1 | 2 << 8 | 3 << 16)
    assert (p.min_keypoint_score, p.scale, p.min_size, p.fallback) == (0.25, 2.0, 0.1, 0.25)


@pytest.mark.parametrize("name,bad", [
    ('region', 'face'), ('region', 0), ('mode', 'mosaic'), ('mode', None), ('shape', 'circle'), ('shape', 1),
    ('blocks', 1), ('blocks', 33), ('blocks', 8.0), ('blocks', True), ('radius', 0), ('radius', 13), ('radius', 2.5),
    ('color', (0, 0)), ('color', (0, 0, 256)), ('color', (-1, 0, 0)), ('color', (0.5, 0, 0)), ('color', 7), ('color', 'red'),
    ('scale', 0), ('scale', -1.0), ('scale', float('inf')), ('scale', float('nan')), ('scale', 'big'),
    ('min_size', -0.1), ('min_size', float('nan')), ('fallback', 0), ('fallback', 1.5), ('fallback', float('inf')),
    ('min_keypoint_score', float('nan')), ('min_keypoint_score', float('inf')), ('min_keypoint_score', 1e39),
    ('min_keypoint_score', 'x'), ('overlay', 1), ('overlay', None),
])
def test_every_range_error_names_the_argument_and_the_value(name, bad):
    with pytest.raises(ValueError, match="^Anonymize: " + name + " must .*" + re.escape(f"(got {bad!r})") + "$"):
        Anonymize(**{name: bad})


# ------------------------------------------------------------------ the Detector's keys and checks
def test_signatures_and_exports():
    from multiposenet_amd import inference
    assert inference.Anonymize is anonymize_stage.Anonymize and inference.Anonymizer is anonymize_stage.Anonymizer
    assert inference.anonymize is anonymize_stage.anonymize
    assert list(inspect.signature(inference.anonymize).parameters) == ['image', 'outputs', 'spec']
    for method in ('predict_batch', 'predict_images', 'predict_jpegs'):
        parameter = inspect.signature(getattr(Detector, method)).parameters['anonymize']
        assert parameter.default is None, method
        assert "anonymize:" in getattr(Detector, method).__doc__ or "anonymize" in getattr(Detector, method).__doc__
    assert "network's input" in Detector.predict_batch.__doc__


@pytest.mark.parametrize("use_graph", [True, False])
def test_entry_keys_are_the_literal_tuples(use_graph):
    det = _detector(use_graph)
    batch = np.zeros((B, H, W, 3), np.uint8)
    frames = [np.zeros((50, 70, 3), np.uint8), np.zeros((64, 33, 3), np.uint8)]
    base = (B, H, W, THR) if use_graph else ('eager', B, H, W)
    spec, nms = Anonymize(mode='blur', radius=3), PoseNms(0.8)
    for options, tail in _table():                                  # anonymize=None: the keys every other test pins
        assert _key_of(det.predict_batch, batch, score_threshold=THR, anonymize=None, **options) == base + tail
        assert _key_of(det.predict_images, frames, size=(H, W), score_threshold=THR, anonymize=None, **options) == \
            ('images', B, H, W, THR, CAP) + tail
    trk = _tracker()
    table = [
        (dict(annotate=True), ('annotate', 'anonymize', spec)),
        (dict(annotate='jpeg'), ('annotate', 'jpeg', '4:2:0', 'anonymize', spec)),
        (dict(annotate=True, plot_maps=True, flip=True), ('annotate', 'maps', 'tta', True, (), 'anonymize', spec)),
        (dict(annotate=True, track=trk, track_style=STYLE.__class__(), pose_nms=nms),
         ('annotate', 'track', SERIAL, B, 'style', STYLE.__class__(), 'pose_nms', nms, 'anonymize', spec)),
    ]
    for options, tail in table:
        key = _key_of(det.predict_batch, batch, score_threshold=THR, anonymize=spec, **options)
        assert key == base + tail and key[-2:] == ('anonymize', spec), options
        key = _key_of(det.predict_images, frames, size=(H, W), score_threshold=THR, anonymize=spec, **options)
        assert key == ('images', B, H, W, THR, CAP) + tail, options
        # an equal spec finds the same entry
        again = _key_of(det.predict_batch, batch, score_threshold=THR, anonymize=Anonymize(mode='blur', radius=3), **options)
        assert again == base + tail and hash(again) == hash(base + tail)
    other = _key_of(det.predict_batch, batch, score_threshold=THR, annotate=True, anonymize=Anonymize(mode='blur', radius=4))
    assert other != base + table[0][1]


def test_options_field_and_tail():
    det = _detector(True)
    spec = Anonymize()
    given = dict(score_threshold=THR, return_heatmaps=True, annotate=True, jpeg_quality=75, jpeg_subsampling='4:2:0',
                 plot_maps=False, groundtruth=None, flip=False, scales=None, track=None, track_style=None)
    opts, _ = det._options(lambda: (B, H, W), **given)              # `anonymize` may be absent
    assert opts.anonymize is None and opts.tail(B) == ('annotate',)
    opts, _ = det._options(lambda: (B, H, W), anonymize=spec, **given)
    assert opts.anonymize is spec and opts.tail(B) == ('annotate', 'anonymize', spec)
    assert opts._fields[-2:] == ('anonymize', 'pose_nms')


def test_argument_checks_and_their_order():
    det = _detector(True)
    batch, frames = np.zeros((B, H, W, 3), np.uint8), [np.zeros((50, 70, 3), np.uint8)] * B
    spec = Anonymize()
    for method, first in ((det.predict_batch, batch), (det.predict_images, frames)):
        with pytest.raises(ValueError, match="anonymize must be None or an inference.Anonymize"):
            method(first, annotate=True, anonymize='head')
        with pytest.raises(ValueError, match="anonymize must be None or an inference.Anonymize"):
            method(first, annotate=True, anonymize=dict(mode='blur'))
        for annotate in (False, None, 0):
            with pytest.raises(ValueError, match="anonymize= .* needs annotate=True or 'jpeg'"):
                method(first, annotate=annotate, anonymize=spec)
        with pytest.raises(ValueError, match="overlay=False"):
            method(first, annotate=True, track=_tracker(), track_style=STYLE.__class__(), anonymize=Anonymize(overlay=False))
        # checked last: behind flip, pose_nms and track_eval
        with pytest.raises(ValueError, match="flip must be"):
            method(first, flip=1, anonymize='head')
        with pytest.raises(ValueError, match="pose_nms must be"):
            method(first, pose_nms='x', anonymize='head')
        with pytest.raises(ValueError, match="track_eval must be"):
            method(first, track_eval='x', anonymize='head')
    with pytest.raises(ValueError, match="empty batch"):
        det.predict_jpegs([], anonymize='head')
    nodet = _detector(True)
    nodet.retinanet = None
    with pytest.raises(ValueError, match="anonymize= needs the person detector"):
        nodet.predict_batch(batch, annotate=True, anonymize=spec)
    many = _detector(True)
    many.params = {'max_boxes': 129}
    with pytest.raises(ValueError, match=r"anonymize: max_boxes must be in 1..128 \(got 129\)"):
        many.predict_batch(batch, annotate=True, anonymize=spec)
    key = _key_of(det.predict_batch, batch, annotate=True, anonymize=Anonymize(overlay=False))      # overlay=False alone is fine
    assert key[-2] == 'anonymize'


def test_command_line_flags():
    import argparse
    ap = argparse.ArgumentParser()
    anonymize_stage.add_arguments(ap)
    assert anonymize_stage.from_arguments(ap, ap.parse_args([])) is None
    assert anonymize_stage.from_arguments(ap, ap.parse_args(["--anonymize"])) == Anonymize()
    got = anonymize_stage.from_arguments(ap, ap.parse_args(["--anonymize", "box", "--anonymize-mode", "blur", "--anonymize-shape",
                                                             "rectangle", "--anonymize-radius", "3", "--anonymize-blocks", "4",
                                                             "--anonymize-no-overlay"]))
    assert got == Anonymize(region='box', mode='blur', shape='rectangle', radius=3, blocks=4, overlay=False)
    with pytest.raises(SystemExit):
        anonymize_stage.from_arguments(ap, ap.parse_args(["--anonymize", "--anonymize-blocks", "99"]))
    with pytest.raises(SystemExit):
        ap.parse_args(["--anonymize", "face"])


# ------------------------------------------------------------------ the reference
@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.mark.parametrize("region", C.REGIONS)
def test_fill_rectangle_is_what_pillow_draws(cases, region):
    from PIL import Image, ImageDraw
    spec = Anonymize(region=region, mode='fill', shape='rectangle', color=(200, 30, 7))
    painted = 0
    for name, image, boxes, kps, with_kp in cases:
        h, w, _ = image.shape
        im = Image.fromarray(image)
        pen = ImageDraw.Draw(im)
        for box, kp in zip(boxes, kps):
            r = R.region_of(box, kp, h, w, spec, with_kp)
            if r is not None:
                x0, y0, x1, y1 = r
                pen.rectangle((x0, y0, x1 - 1, y1 - 1), fill=spec.color)
        got = R.anonymize(image, boxes, kps, spec, with_kp)
        np.testing.assert_array_equal(got, np.asarray(im), err_msg=name)
        painted += int((got != image).any(axis=2).sum())
    assert painted > 10000


def test_regions_of_the_handmade_cases(cases):
    by_name = {c[0]: c for c in cases}
    head, box = Anonymize(), Anonymize(region='box')
    # by hand, on a 64 x 128 frame where the normalised box is exact in float32: box rows 16..48, columns 16..64
    b, kp = C.person(64, 128, (16, 16, 48, 64), (30, 24), 3.0)
    # nose (30, 24), eyes 1.5 beside and 1 above, ears 3 beside: mean (30, 23.6), e = 3, s = max(3 * 2, 32 * 0.1) = 6
    assert R.region_of(b, kp, 64, 128, box) == (16, 16, 64, 48) and R.region_of(b, kp, 64, 128, head) == (24, 17, 36, 30)
    assert R.region_of(b, kp, 64, 128, Anonymize(scale=0.5)) == (26, 20, 34, 27)      # s = 32 * 0.1: min_size decides
    b, kp = C.person(64, 128, (16, 16, 48, 64), (30, 24), 3.0, 0.5, 1)      # the nose alone: e = 0, s = 3.2 around it
    assert R.region_of(b, kp, 64, 128, head) == (26, 20, 34, 28)
    b, kp = C.person(64, 128, (16, 16, 48, 64), (30, 24), 3.0, 0.5, 0)      # no face joint: the top quarter of the box
    assert R.region_of(b, kp, 64, 128, head) == (16, 16, 64, 24) and R.region_of(b, kp, 64, 128, Anonymize(fallback=1.0)) == (16, 16, 64, 48)
    b, kp = C.person(64, 128, (16, 16, 48, 64), (30, 24), 3.0)
    assert R.region_of(b, kp, 64, 128, head, False) == (16, 16, 64, 24) and R.region_of(b, None, 64, 128, head) == (16, 16, 64, 24)
    assert R.region_of(b, kp, 64, 128, Anonymize(min_keypoint_score=0.6)) == (16, 16, 64, 24)      # every joint scores 0.5
    assert by_name["boxes_only"][4] is False
    _, _, boxes, kps, _ = by_name["not_finite"]
    assert [R.region_of(b, k, 70, 90, box) is None for b, k in zip(boxes, kps)] == [True, True, False, False, False]
    assert [R.region_of(b, k, 70, 90, head) is None for b, k in zip(boxes, kps)] == [False, False, True, True, False]
    _, _, boxes, kps, _ = by_name["zero_area_box"]
    assert R.region_of(boxes[0], kps[0], 70, 90, box) is None and R.region_of(boxes[0], kps[0], 70, 90, head) is not None
    assert R.region_of(boxes[1], kps[1], 70, 90, head) is None      # F empty and a box without width
    _, _, boxes, kps, _ = by_name["entirely_outside"]
    assert all(R.coverage(R.region_of(b, k, 70, 90, s), 'ellipse', 70, 90) is None for b, k in zip(boxes, kps) for s in (head, box))
    huge = np.array([-1e30, -1e30, 1e30, 1e30], F)
    assert R.region_of(huge, kps[0], 70, 90, box) == (-2 ** 20, -2 ** 20, 2 ** 20, 2 ** 20)     # clamped; a rectangle beyond 32768
    assert R.covered(0, 0, (-2 ** 20, -2 ** 20, 2 ** 20, 2 ** 20), 'ellipse') and not R.covered(0, 0, (0, 0, 90, 70), 'ellipse')


@pytest.mark.parametrize("mode,shape,region", C.GRID)
def test_pixels_outside_every_region_are_the_sources(cases, mode, shape, region):
    spec = Anonymize(region=region, mode=mode, shape=shape, color=(9, 9, 9))
    for name, image, boxes, kps, with_kp in cases:
        h, w, _ = image.shape
        got = R.anonymize(image, boxes, kps, spec, with_kp)
        regions = [R.region_of(b, k, h, w, spec, with_kp) for b, k in zip(boxes, kps)]
        regions = [r for r in regions if r is not None]
        if h * w <= 97 * 131:                                       # pixel by pixel with the scalar test
            inside = np.array([[any(R.covered(x, y, r, shape) for r in regions) for x in range(w)] for y in range(h)], bool).reshape(h, w)
            np.testing.assert_array_equal(got[~inside], image[~inside], err_msg=name)
            for r in regions:                                       # the vectorised coverage is the scalar one
                c = R.coverage(r, shape, h, w)
                if c is not None:
                    ya, xa, mask = c
                    np.testing.assert_array_equal(mask, inside[ya:ya + mask.shape[0], xa:xa + mask.shape[1]] &
                                                  np.array([[R.covered(xa + i, ya + j, r, shape) for i in range(mask.shape[1])]
                                                            for j in range(mask.shape[0])], bool), err_msg=name)
            if mode == 'fill':
                assert (got[inside] == 9).all(), name
        if name == "nobody" or name == "entirely_outside":
            np.testing.assert_array_equal(got, image)


def test_pixelate_properties(cases):
    constant = np.full((70, 90, 3), (17, 130, 255), np.uint8)
    for name, image, boxes, kps, with_kp in cases[:12]:
        for region in C.REGIONS:
            np.testing.assert_array_equal(R.anonymize(constant, boxes, kps, Anonymize(region=region), with_kp), constant, err_msg=name)
    # blocks bounds the distinct cells per side: one person, a rectangle, on a noise image
    name, image, boxes, kps, _ = cases[1]
    for blocks in (2, 5, 8, 32):
        spec = Anonymize(region='box', shape='rectangle', blocks=blocks)
        x0, y0, x1, y1 = R.region_of(boxes[0], kps[0], 70, 90, spec)
        got = R.anonymize(image, boxes, kps, spec)[y0:y1, x0:x1]
        c = -(-max(x1 - x0, y1 - y0) // blocks)
        runs_x = 1 + int((np.diff(got.astype(int), axis=1) != 0).any(axis=(0, 2)).sum())
        runs_y = 1 + int((np.diff(got.astype(int), axis=0) != 0).any(axis=(1, 2)).sum())
        assert runs_x <= -(-(x1 - x0) // c) <= blocks and runs_y <= -(-(y1 - y0) // c) <= blocks, blocks
        cell = image[y0:y0 + c, x0:x0 + c].astype(np.int64).reshape(-1, 3)
        np.testing.assert_array_equal(got[0, 0], (2 * cell.sum(axis=0) + len(cell)) // (2 * len(cell)))


@pytest.mark.parametrize("mode", C.MODES)
def test_the_later_person_wins_and_both_read_the_original(cases, mode):
    name, image, boxes, kps, _ = next(c for c in cases if c[0] == "three_overlapping")
    spec = Anonymize(region='box', mode=mode, shape='ellipse', color=(1, 2, 3))
    h, w, _ = image.shape
    alone = [R.anonymize(image, boxes[i:i + 1], kps[i:i + 1], spec) for i in range(3)]
    masks = []
    for i in range(3):
        m = np.zeros((h, w), bool)
        ya, xa, part = R.coverage(R.region_of(boxes[i], kps[i], h, w, spec), 'ellipse', h, w)
        m[ya:ya + part.shape[0], xa:xa + part.shape[1]] = part
        masks.append(m)
    assert (masks[0] & masks[1] & masks[2]).sum() > 50
    want = image.copy()
    for i in range(3):                                              # each person's own picture of the ORIGINAL, the last on top
        want[masks[i]] = alone[i][masks[i]]
    np.testing.assert_array_equal(R.anonymize(image, boxes, kps, spec), want)


def test_blur_window_is_the_blurred_frame(cases):
    image = C.frame(40, 61, 83)
    for radius in (1, 5, 12):
        whole = R.blur(image, radius)
        for ya, yb, xa, xb in ((0, 61, 0, 83), (20, 30, 40, 50), (0, 5, 70, 83), (55, 61, 0, 9), (30, 31, 41, 42)):
            np.testing.assert_array_equal(R.blur_window(image, radius, ya, yb, xa, xb), whole[ya:yb, xa:xb])
    # a constant frame stays itself; one pass of radius 1 by hand
    np.testing.assert_array_equal(R.blur(np.full((4, 6, 3), 201, np.uint8), 12), np.full((4, 6, 3), 201, np.uint8))
    row = np.array([[[0, 0, 0], [10, 10, 10], [255, 255, 255]]], np.uint8)
    np.testing.assert_array_equal(R.blur(row, 1, passes=1)[0, :, 0], [(2 * 10 + 3) // 6, (2 * 265 + 3) // 6, (2 * 520 + 3) // 6])


# ------------------------------------------------------------------ the C ABI, without a GPU
def test_workspace_bytes_and_the_parameter_struct():
    l = _lib.lib()
    assert l.mpn_anonymize_params_bytes() == ctypes.sizeof(anonymize_stage.Params) == 56
    assert l.mpn_anonymize_workspace_bytes(16, 25) >= 16 * 25 * (32 + 4 * 32 * 32)
    for b, m in ((0, 25), (1, 0), (1, 129), (-1, 25), (4097, 1), (64, 65), (33, 128)):
        assert l.mpn_anonymize_workspace_bytes(b, m) == 0, (b, m)
    assert l.mpn_anonymize_workspace_bytes(32, 128) > 0 and l.mpn_anonymize_workspace_bytes(4096, 1) > 0


def test_every_argument_check_runs_before_any_hip_call():
    l = _lib.lib()
    P, Q = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    b, m = 2, 25
    record, work = l.mpn_pose_gather_record_bytes(b, m), l.mpn_anonymize_workspace_bytes(b, m)
    good = Anonymize().params()

    def call(sources=P, sources_bytes=1000, descs=P, rec=P, record_bytes=record, B_=b, M=m, params=good, out=P, out_bytes=1000,
             workspace=P, workspace_bytes=work):
        params = ctypes.byref(params) if params is not None else None
        return _lib.call("mpn_anonymize", sources, sources_bytes, descs, rec, record_bytes, B_, M, 1, params, out, out_bytes,
                         workspace, workspace_bytes, None)
    for null in ('sources', 'descs', 'rec', 'params', 'out', 'workspace'):
        with pytest.raises(ValueError, match="BAD_ARG: anonymize: null pointer"):
            call(**{null: None})
    for bad in (dict(B_=0), dict(B_=65536), dict(M=0), dict(M=129), dict(B_=64, M=65)):
        with pytest.raises(ValueError, match="BAD_SHAPE: anonymize"):
            call(**bad)
    for name in ('descs', 'rec', 'workspace'):
        with pytest.raises(ValueError, match="BAD_ALIGN: anonymize"):
            call(**{name: Q})
    for bad in (dict(record_bytes=record - 1), dict(workspace_bytes=work - 1), dict(sources_bytes=2), dict(out_bytes=2)):
        with pytest.raises(_lib.MpnError, match="WORKSPACE: anonymize"):
            call(**bad)
    call_ok_until_launch = dict(sources=Q, out=Q)                   # sources and out_rgb need no alignment: not refused for it
    for field, values in (('region', (-1, 2)), ('mode', (-1, 3)), ('shape', (-1, 2)), ('blocks', (1, 33)), ('radius', (0, 13)),
                          ('color', (-1, 1 << 24)), ('scale', (0.0, -1.0, float('inf'), float('nan'))),
                          ('min_size', (-0.5, float('nan'))), ('fallback', (0.0, 1.5, float('nan'))),
                          ('min_keypoint_score', (float('nan'), float('inf')))):
        for v in values:
            p = Anonymize().params()
            setattr(p, field, v)
            with pytest.raises(ValueError, match="BAD_ARG: anonymize: " + field):
                call(params=p, **call_ok_until_launch)
