"""CPU: the drawing of `Detector.predict_images(..., annotate=True)` - the numpy restatement tests/draw_ref.py against the
golden frames the reference notebook drew under Pillow, against Pillow itself where it is importable (every line up to 48
pixels in every direction, rectangles and dots over all truncation cases), the dot stamps compiled into the library, and every
argument check of the new entry points, none of which needs a device. Equality is every byte of every frame."""
import ctypes
import os

import numpy as np
import pytest

import draw_ref as R
from multiposenet_amd import _lib
from multiposenet_amd.inference import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw_cases.npz")
F = np.float32


def goldens():
    with np.load(GOLDEN) as z:
        return [(str(n), z[f"{n}/image"], {"boxes": z[f"{n}/boxes"], "keypoint_positions": z[f"{n}/keypoint_positions"]},
                 z[f"{n}/annotated"]) for n in z["names"]]


def test_restatement_equals_every_golden_exactly():
    cases = goldens()
    assert len(cases) >= 12
    counts = set()
    for name, img, outputs, want in cases:
        assert img.shape[0] <= 160 and img.shape[1] <= 200 and want.shape == img.shape[:2] + (4,)
        got = R.draw_everything(img, outputs)
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert (want[..., 3] == 255).all()
        counts.add(len(outputs["boxes"]))
        if len(outputs["boxes"]):
            assert (want[..., :3] != img).any(), name                 # something was drawn
        else:
            np.testing.assert_array_equal(want[..., :3], img)
    assert {0, 1, 3, 25} <= counts


def test_golden_cases_cover_what_they_claim():
    by_name = {name: (img, o) for name, img, o, _ in goldens()}
    img, o = by_name["dots_below_two"]
    dots = [p for p in R.primitives(o["boxes"], o["keypoint_positions"], *img.shape[:2]) if p[0] == R.DOT]
    assert {(p[3] - p[1], p[4] - p[2]) for p in dots} == {(3, 3), (3, 4), (4, 3), (4, 4)}   # every stamp occurs
    img, o = by_name["coincident_keypoints"]
    lines = [p for p in R.primitives(o["boxes"], o["keypoint_positions"], *img.shape[:2]) if p[0] == R.LINE]
    assert sum(p[1:3] == p[3:5] for p in lines) >= 16                                       # zero-length lines
    img, o = by_name["keypoints_outside_frame"]
    h, w = img.shape[:2]
    prims = R.primitives(o["boxes"], o["keypoint_positions"], h, w)
    assert any(p[1] < 0 for p in prims) and any(p[3] >= w for p in prims) and any(p[2] < 0 for p in prims) and any(p[4] >= h for p in prims)
    img, o = by_name["flat_boxes"]
    rects = [p for p in R.primitives(o["boxes"], o["keypoint_positions"], *img.shape[:2]) if p[0] == R.RECT]
    assert any(p[2] == p[4] for p in rects) and any(p[1] == p[3] for p in rects)
    assert len({img.shape[:2] for img, _ in by_name.values()}) >= 10 and any(img.shape[1] % 2 for img, _ in by_name.values())


def _mask(pixels, h, w):
    m = np.zeros((h, w), bool)
    for x, y in pixels:
        if 0 <= x < w and 0 <= y < h:
            m[y, x] = True
    return m


def test_lines_equal_pillow_exhaustively():
    Image, ImageDraw = pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageDraw")
    n = 0
    for dx in range(-48, 49):              # all 8 octants, horizontal, vertical, the diagonals and the single point
        for dy in range(-48, 49):
            im = Image.new("L", (101, 101))
            ImageDraw.Draw(im).line([(50, 50), (50 + dx, 50 + dy)], fill=255)
            got = _mask(R.line_pixels(50, 50, 50 + dx, 50 + dy), 101, 101)
            assert np.array_equal(got, np.asarray(im) > 0), (dx, dy)
            n += 1
    assert n == 97 * 97
    # float end points are truncated toward zero; pixels outside the frame are dropped one by one
    rng = np.random.RandomState(0)
    for _ in range(300):
        x0, y0, x1, y1 = (F(v) for v in rng.uniform(-30, 70, 4))
        im = Image.new("L", (40, 33))
        ImageDraw.Draw(im).line([(x0, y0), (x1, y1)], fill=255)
        got = _mask(R.line_pixels(R.trunc(x0), R.trunc(y0), R.trunc(x1), R.trunc(y1)), 33, 40)
        assert np.array_equal(got, np.asarray(im) > 0), (x0, y0, x1, y1)


def test_rectangles_equal_pillow_over_all_truncation_cases():
    Image, ImageDraw = pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageDraw")
    values = [-3.0, -1.5, -0.9, -0.0, 0.0, 0.4, 0.99, 1.0, 1.6, 2.0, 5.5, 9.0, 10.9, 11.0, 11.3, 14.0]    # frame 12 x 11
    n = 0
    for x0 in values:
        for x1 in values:
            if x1 < x0:
                continue
            for y0 in values:
                for y1 in values:
                    if y1 < y0:
                        continue
                    im = Image.new("L", (12, 11))
                    ImageDraw.Draw(im).rectangle([(x0, y0), (x1, y1)], outline=255)
                    got = _mask(R.rect_pixels(R.trunc(x0), R.trunc(y0), R.trunc(x1), R.trunc(y1)), 11, 12)
                    assert np.array_equal(got, np.asarray(im) > 0), (x0, y0, x1, y1)
                    n += 1
    assert n > 15000


def test_dots_equal_pillow_over_all_truncation_cases():
    Image, ImageDraw = pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageDraw")
    values = [F(v) for v in np.arange(-5.0, 5.01, 0.25)] + [F(1e-9), F(-1e-9), F(1.9999999), F(2.0000002), F(-1.9999999),
                                                            F(8.5), F(11.75), F(12.0), F(14.2)]             # frame 12 x 13
    seen = set()
    for x in values:
        for y in values:
            im = Image.new("L", (12, 13))
            s = 2
            ImageDraw.Draw(im).ellipse([(x - s, y - s), (x + s, y + s)], fill=255)      # the notebook's expression
            c = (R.trunc(F(x) - F(2)), R.trunc(F(y) - F(2)), R.trunc(F(x) + F(2)), R.trunc(F(y) + F(2)))
            seen.add((c[2] - c[0], c[3] - c[1]))
            assert np.array_equal(_mask(R.dot_pixels(*c), 13, 12), np.asarray(im) > 0), (x, y)
    assert seen == set(R.STAMPS)                                                         # 3 or 4 on either axis, nothing else


def test_dot_stamps_of_the_library_equal_the_restatement():
    lib = _lib.lib()
    for (dw, dh), rows in R.STAMPS.items():
        assert tuple(lib.mpn_draw_dot_stamp(dw, dh, j) for j in range(dh + 1)) == rows
    for bad in ((2, 3, 0), (5, 4, 0), (3, 2, 0), (4, 5, 0), (3, 3, 4), (4, 4, 5), (3, 3, -1)):
        assert lib.mpn_draw_dot_stamp(*bad) == -1


def test_draw_entry_points_validate_before_any_hip_call():
    lib = _lib.lib()
    P16 = ctypes.c_void_p(4096)
    call = _lib.call
    assert hasattr(lib, "mpn_draw_detections") and "mpn_draw_detections" in _lib.SIGNATURES
    assert lib.mpn_draw_desc_bytes() == draw.DESC_WORDS * 4 == 32
    assert lib.mpn_draw_detections_workspace_bytes(16, 25) == 16 * 25 * 34 * 32          # 1 box + 16 lines + 17 dots, 32 bytes each
    assert lib.mpn_draw_detections_workspace_bytes(0, 25) == 0 and lib.mpn_draw_detections_workspace_bytes(1, draw.MAX_BOXES + 1) == 0
    assert lib.mpn_draw_detections_workspace_bytes(200, 25) == 0
    rec, work = lib.mpn_pose_gather_record_bytes(2, 25), lib.mpn_draw_detections_workspace_bytes(2, 25)
    good = [P16, 1 << 20, P16, P16, rec, 2, 25, 1, P16, 1 << 20, P16, work, None]

    def args(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return a

    for i in (0, 2, 3, 8, 10):                                        # sources, descs, record, out_rgba, workspace
        with pytest.raises(ValueError, match="null"):
            call("mpn_draw_detections", *args(**{f"a{i}": None}))
    with pytest.raises(ValueError, match="B must"):
        call("mpn_draw_detections", *args(a5=0))
    with pytest.raises(ValueError, match="max_boxes must"):
        call("mpn_draw_detections", *args(a6=0))
    with pytest.raises(ValueError, match="max_boxes must"):
        call("mpn_draw_detections", *args(a6=draw.MAX_BOXES + 1))
    with pytest.raises(ValueError, match="rows"):
        call("mpn_draw_detections", *args(a5=200))
    for i in (2, 3, 8, 10):
        with pytest.raises(ValueError, match="aligned"):
            call("mpn_draw_detections", *args(**{f"a{i}": ctypes.c_void_p(4100)}))
    with pytest.raises(_lib.MpnError, match="record of"):
        call("mpn_draw_detections", *args(a4=rec - 1))
    with pytest.raises(_lib.MpnError, match="workspace of"):
        call("mpn_draw_detections", *args(a11=work - 1))
    with pytest.raises(_lib.MpnError, match="out_rgba of"):
        call("mpn_draw_detections", *args(a9=0))


def test_annotate_is_an_argument_of_both_batch_calls():
    """Without the feature these raise TypeError (an unexpected keyword); with it the argument checks answer first."""
    from multiposenet_amd.inference.detector import Detector
    det = object.__new__(Detector)
    with pytest.raises(ValueError, match="empty"):
        det.predict_images([], annotate=True)
    with pytest.raises(ValueError, match="empty"):
        det.predict_batch([], annotate=True)


def test_output_layout_and_capacity():
    desc, frames, nbytes = draw.layout([(3, 5), (2, 2), (1, 1)], [0, 45, 57])
    assert desc.dtype == np.int32 and desc.shape == (3, draw.DESC_WORDS)
    assert desc.view(np.int64)[:, :2].tolist() == [[0, 0], [45, 64], [57, 80]] and desc[:, 4:6].tolist() == [[3, 5], [2, 2], [1, 1]]
    assert frames == [(0, 3, 5), (64, 2, 2), (80, 1, 1)] and nbytes == 96 and not desc[:, 6:].any()
    # any frames whose RGB bytes fit a source capacity fit the output capacity derived from it
    rng = np.random.RandomState(1)
    for _ in range(200):
        shapes = [tuple(int(v) for v in rng.randint(1, 40, 2)) for _ in range(rng.randint(1, 9))]
        src = sum(h * w * 3 for h, w in shapes) + 4
        assert draw.layout(shapes, [0] * len(shapes))[2] <= draw.out_capacity(src, len(shapes))
    assert draw.out_capacity(1 << 20, 4) % 16 == 0


def test_draw_everything_argument_errors_need_no_device():
    from multiposenet_amd.inference import draw_everything
    ok = {"boxes": np.zeros((2, 4), F), "keypoint_positions": np.zeros((2, 17, 2), F)}
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), F), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="image must be"):
            draw_everything(bad, ok)
    with pytest.raises(ValueError, match="rows of keypoint_positions"):
        draw_everything(np.zeros((4, 4, 3), np.uint8), {"boxes": np.zeros((2, 4), F), "keypoint_positions": np.zeros((1, 17, 2), F)})
    with pytest.raises(ValueError, match="at most"):
        draw_everything(np.zeros((4, 4, 3), np.uint8), {"boxes": np.zeros((200, 4), F), "keypoint_positions": np.zeros((200, 17, 2), F)})
