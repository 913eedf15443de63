"""CPU: the host side of `Detector.predict_images` - Pillow's resize restated on `resample_tables`, the table cache, the
letterbox geometry, the packing of a ragged batch, and every argument error, none of which needs a device."""
import os

import numpy as np
import pytest

import pil_resize_ref as P
from multiposenet_amd.inference import resample

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil_resize_goldens.npz")


def _goldens():
    with np.load(GOLDEN) as z:
        return [(str(n), z[f"{n}/source"], z[f"{n}/resized"]) for n in z["names"]]


def test_restatement_equals_every_golden_exactly():
    cases = _goldens()
    assert len(cases) >= 10
    kinds = set()
    for name, src, want in cases:
        assert max(src.shape[:2]) <= 160
        got = P.resize(src, want.shape[0], want.shape[1])
        assert got.dtype == np.uint8 and got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=name)
        kinds.add((np.sign(src.shape[0] - want.shape[0]), np.sign(src.shape[1] - want.shape[1])))
    # reductions, an upscale, an identity and the two single-pass cases are all present
    assert {(1, 1), (-1, -1), (0, 0), (0, 1), (1, 0)} <= kinds


def test_restatement_equals_live_pillow_on_a_seeded_sweep():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(2024)
    for _ in range(30):
        h, w, oh, ow = (int(v) for v in rng.randint(1, 200, 4))
        src = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        want = np.asarray(Image.fromarray(src).resize((ow, oh)))
        np.testing.assert_array_equal(P.resize(src, oh, ow), want, err_msg=f"{h}x{w} -> {oh}x{ow}")


def test_tables_shape_cache_and_range():
    bounds, coeffs = resample.resample_tables(1920, 640)
    assert bounds.shape == (640, 2) and coeffs.shape == (640, 13) and bounds.dtype == coeffs.dtype == np.int32
    assert resample.resample_tables(1920, 640)[1] is coeffs                       # cached per (in, out)
    assert not coeffs.flags.writeable
    assert resample.resample_tables(160, 20)[1].shape[1] == 33                    # an 8x reduction
    assert resample.resample_tables(20, 160)[1].shape[1] == 5                     # upscale: support 2
    for i, o in ((1920, 640), (160, 20), (7, 128), (1, 128), (333, 128)):
        b, c = resample.resample_tables(i, o)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= i).all()
        assert (np.abs(c.astype(np.int64)).sum(axis=1) * 255 < 2 ** 31).all()     # int32 accumulation is safe
        assert (np.abs(c.sum(axis=1) - (1 << 22)) <= c.shape[1]).all()            # normalised weights
    with pytest.raises(ValueError):
        resample.resample_tables(0, 4)


def test_letterbox_geometry_hand_computed():
    # 1080 x 1920 on 640 x 640: s = min(640/1080, 640/1920) = 1/3 -> 360 x 640
    assert resample.resized_size(1080, 1920, 640, 640, True) == (360, 640)
    assert resample.resized_size(1080, 1920, 640, 640, False) == (640, 640)
    # 100 x 50 on 256 x 384: s = min(2.56, 7.68) = 2.56 -> 256 x 128
    assert resample.resized_size(100, 50, 256, 384, True) == (256, 128)
    # 3 x 1000 on 128 x 128: s = 0.128 -> round(0.384) = 0 -> max(1, .) = 1
    assert resample.resized_size(3, 1000, 128, 128, True) == (1, 128)
    e = resample.extent_of(1080, 1920, 360, 640, 640, 640)
    assert e.dtype == np.float32 and e.tolist() == [np.float32(640 / 360), 1.0, 1080.0, 1920.0]
    assert resample.extent_of(97, 131, 256, 384, 256, 384).tolist() == [1.0, 1.0, 97.0, 131.0]


def test_plan_packs_sources_tables_and_descriptors():
    shapes = [(97, 131), (256, 384), (300, 500), (97, 131)]
    plan = resample.Plan(shapes, 256, 384)
    d = plan.meta[:4 * resample.DESC_WORDS].reshape(4, resample.DESC_WORDS)
    offs = d.view(np.int64)[:, :2]
    assert offs[:, 0].tolist() == [0, 97 * 131 * 3, 97 * 131 * 3 + 256 * 384 * 3, 97 * 131 * 3 + 256 * 384 * 3 + 300 * 500 * 3]
    assert plan.src_offsets == offs[:, 0].tolist() and plan.stage_bytes == offs[3, 0] + 97 * 131 * 3 + 4
    assert (offs[:, 1] % 16 == 0).all() and (d[:, 14] == 384 * 3).all()
    assert d[:, 4:8].tolist() == [[97, 131, 256, 384], [256, 384, 256, 384], [300, 500, 256, 384], [97, 131, 256, 384]]
    assert d[0, 8:14].tolist() == d[3, 8:14].tolist()                             # equal sizes share their tables
    tables = plan.meta[4 * (resample.DESC_WORDS + 4):]
    assert len(tables) == plan.table_words
    bx, cx = resample.resample_tables(500, 384)
    np.testing.assert_array_equal(tables[d[2, 8]:d[2, 8] + bx.size].reshape(bx.shape), bx)
    np.testing.assert_array_equal(tables[d[2, 9]:d[2, 9] + cx.size].reshape(cx.shape), cx)
    assert d[2, 12] == cx.shape[1]
    np.testing.assert_array_equal(plan.meta[4 * resample.DESC_WORDS:4 * (resample.DESC_WORDS + 4)].view(np.float32).reshape(4, 4),
                                  plan.extents)
    keep = resample.Plan([(1080, 1920)], 640, 640, keep_aspect_ratio=True)
    assert keep.new_sizes == [(360, 640)] and keep.work_bytes == 1080 * 1920
    assert resample.capacity_for(5) == 8 and resample.capacity_for(8) == 8 and resample.capacity_for(0) == 1


def test_canvas_places_the_image_top_left():
    src = np.random.RandomState(3).randint(0, 256, (50, 120, 3)).astype(np.uint8)
    c = P.canvas(src, 128, 256, keep_aspect_ratio=True)                           # s = min(2.56, 2.133) -> 107 x 256
    assert resample.resized_size(50, 120, 128, 256, True) == (107, 256)
    np.testing.assert_array_equal(c[:107], P.resize(src, 107, 256))
    assert not c[107:].any()


def test_predict_images_argument_errors_need_no_device():
    from multiposenet_amd.inference.detector import Detector
    det = object.__new__(Detector)                     # the checks run before anything of the instance is touched
    good = np.zeros((10, 12, 3), np.uint8)
    for bad, match in (([], "empty"), ([[[1, 2, 3]]], "numpy arrays"), ([good.astype(np.float32)], "uint8"),
                       ([np.zeros((10, 12), np.uint8)], "height, width, 3"), ([np.zeros((10, 12, 4), np.uint8)], "height, width, 3"),
                       ([np.zeros((0, 12, 3), np.uint8)], "height, width, 3"), (good, "list")):
        with pytest.raises(ValueError, match=match):
            det.predict_images(bad)
    for size in ((640, 600), (0, 128), (100, 100), 640):
        with pytest.raises(ValueError, match="size"):
            det.predict_images([good], size=size)
    # a reduction beyond the kernel's tap loop: 4400 -> 128 is 34.4x, ksize 139 > 65
    with pytest.raises(ValueError, match="taps"):
        det.predict_images([np.zeros((4, 4400, 3), np.uint8)], size=(128, 128))
    assert resample.MAX_KSIZE >= 33                    # at least an 8x reduction


def test_resize_entry_points_validate_before_any_hip_call():
    import ctypes
    from multiposenet_amd import _lib
    P16 = ctypes.c_void_p(4096)
    call = _lib.call
    assert _lib.lib().mpn_image_resize_desc_bytes() == resample.DESC_WORDS * 4 == 64
    assert _lib.lib().mpn_image_resize_workspace_bytes(2, 256, 384, 600) == 600 * 384 * 3
    assert _lib.lib().mpn_image_resize_workspace_bytes(0, 256, 384, 600) == 0
    with pytest.raises(ValueError, match="null"):
        call("mpn_image_resize", None, P16, P16, 1, 128, 128, P16, P16, 1024, None)
    with pytest.raises(ValueError, match="B must"):
        call("mpn_image_resize", P16, P16, P16, 0, 128, 128, P16, P16, 1024, None)
    with pytest.raises(ValueError, match="multiple of 16"):
        call("mpn_image_resize", P16, P16, P16, 1, 128, 100, P16, P16, 1024, None)
    with pytest.raises(ValueError, match="aligned"):
        call("mpn_image_resize", P16, P16, P16, 1, 128, 128, ctypes.c_void_p(4100), P16, 1024, None)
    with pytest.raises(_lib.MpnError, match="workspace"):
        call("mpn_image_resize", P16, P16, P16, 1, 128, 128, P16, P16, 0, None)
    with pytest.raises(ValueError, match="null"):
        call("mpn_pose_gather_sized", P16, P16, P16, None, None, None, 1, 25, 0.0, None, P16, 1 << 20, None)
    with pytest.raises(ValueError, match="rows"):
        call("mpn_pose_gather_sized", P16, P16, P16, None, None, None, 200, 25, 0.0, P16, P16, 1 << 20, None)
    with pytest.raises(_lib.MpnError, match="record of"):
        call("mpn_pose_gather_sized", P16, P16, P16, None, None, None, 2, 25, 0.0, P16, P16, 16, None)


def test_gather_restatement_maps_boxes_and_keypoints():
    import image_gather_ref as G
    import pose_gather_ref as ref
    rng = np.random.RandomState(0)
    B, M = 2, 3
    boxes = rng.rand(B, M, 4).astype(np.float32)
    scores = np.array([[0.9, 0.2, 0.7], [0.6, 0.5, 0.1]], np.float32)
    num = np.array([3, 2], np.int32)
    ks, kp = rng.rand(B * M, 17).astype(np.float32), rng.rand(B * M, 17, 2).astype(np.float32)
    # extents (1, 1, H, W): the record of mpn_pose_gather
    same = G.pose_gather_sized(boxes, scores, num, ks, kp, 0, 0.3, [[1, 1, 256, 384]] * 2)
    assert same.tobytes() == ref.pose_gather(boxes, scores, num, ks, kp, 0, 0.3, 256, 384).tobytes()
    ext = np.array([[640 / 360, 1.0, 1080, 1920], [1.0, 2.5, 97, 131]], np.float32)
    rec = G.pose_gather_sized(boxes, scores, num, ks, kp, 0, 0.3, ext)
    rows = rec[ref.header_words(B) * 4:].view(ref.ROW)
    assert rec[:4].view(np.int32)[0] == 4 and rows["image_index"][:4].tolist() == [0, 0, 1, 1]
    want = (boxes[1, 0] * np.array([1.0, 2.5, 1.0, 2.5], np.float32)).astype(np.float32)
    np.testing.assert_array_equal(rows["box"][2], want)
    x = np.float32(want[1] * np.float32(131)) + np.float32(kp[3, 5, 1] * np.float32(np.float32(want[3] * np.float32(131)) - np.float32(want[1] * np.float32(131))))
    assert rows["keypoints"][2][5, 0] == x and rows["keypoints"][2][5, 2] == ks[3, 5]
