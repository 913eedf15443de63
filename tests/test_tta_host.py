"""CPU: the numpy definition of the test-time augmentation merge (tests/tta_ref.py), the argument checks of flip= / scales=,
and the declaration and binding of the two entry points."""
import os
import re

import numpy as np
import pytest

import tta_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps(seed, b, h, w):
    r = np.random.RandomState(seed)
    return r.randn(b, h, w, 17).astype(np.float32), r.randn(b, h, w).astype(np.float32)


def test_one_unmirrored_source_is_the_identity():
    heat, seg = _maps(0, 2, 5, 7)
    got = tta_ref.merge([(heat, seg, False)])
    assert got[0].tobytes() == heat.tobytes() and got[1].tobytes() == seg.tobytes()


def test_mirror_and_swap_of_the_base_merges_to_the_base():
    from multiposenet_amd.detector.input_pipeline.keypoint_augment import FLIP_ORDER
    heat, seg = _maps(1, 2, 5, 7)
    assert list(FLIP_ORDER[FLIP_ORDER]) == list(range(17))            # an involution: swapping twice is the identity
    mheat, mseg = np.ascontiguousarray(heat[:, :, ::-1][..., FLIP_ORDER]), np.ascontiguousarray(seg[:, :, ::-1])
    assert not np.array_equal(mheat, heat)
    got = tta_ref.merge([(heat, seg, False), (mheat, mseg, True)])    # (a + a) / 2 is exact
    assert got[0].tobytes() == heat.tobytes() and got[1].tobytes() == seg.tobytes()
    alone = tta_ref.merge([(mheat, mseg, True)])
    assert alone[0].tobytes() == heat.tobytes() and alone[1].tobytes() == seg.tobytes()


def test_a_constant_map_stays_constant_over_resized_sources():
    c = np.float32(0.3125)                                             # 5 / 16: sums of up to 8 copies and the division are exact
    sources = [(np.full((1, h, w, 17), c, np.float32), np.full((1, h, w), c, np.float32), m)
               for (h, w), m in (((4, 6), False), ((2, 3), True), ((8, 12), False), ((6, 9), True), ((3, 5), False))]
    heat, seg = tta_ref.merge(sources)
    assert heat.shape == (1, 4, 6, 17) and seg.shape == (1, 4, 6)
    assert np.all(heat == c) and np.all(seg == c)


def test_resize_is_half_pixel_bilinear_with_clamped_edges():
    a = np.arange(4, dtype=np.float32).reshape(1, 1, 4)
    up = tta_ref.resize(a, 1, 8)[0, 0]
    np.testing.assert_array_equal(up, np.float32([0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3]))
    down = tta_ref.resize(a, 1, 2)[0, 0]
    np.testing.assert_array_equal(down, np.float32([0.5, 2.5]))
    assert tta_ref.resize(a, 1, 4) is a


@pytest.mark.parametrize("scales, match", [
    ([(200, 200)], "multiples of 128"),
    ([(128, 0)], "multiples of 128"),
    ([(128, 384)], "aspect"),
    ([(128, 128), (128, 128)], "twice"),
    ([(256, 256)], "base size"),
    ([(128, 128), (384, 384), (512, 512), (640, 640)], "at most 3"),
    ([128], "width, height"),
])
def test_check_tta_refuses(scales, match):
    from multiposenet_amd.inference.detector import check_tta
    with pytest.raises(ValueError, match=match):
        check_tta(False, scales, 256, 256)


def test_check_tta_accepts():
    from multiposenet_amd.inference.detector import check_tta
    assert check_tta(False, None, 256, 256) == () == check_tta(False, [], 256, 256)
    assert check_tta(True, None, 256, 256) == ('tta', True, ())
    assert check_tta(False, [(128, 128)], 256, 256) == ('tta', False, ((128, 128),))
    # (width, height): a 384 x 256 base (height 256, width 384) takes 192 x 128 ... which is no multiple of 128; 768 x 512 is
    assert check_tta(True, [(768, 512)], 256, 384) == ('tta', True, ((768, 512),))
    with pytest.raises(ValueError, match="aspect"):
        check_tta(True, [(512, 768)], 256, 384)
    with pytest.raises(ValueError, match="flip"):
        check_tta(1, None, 256, 256)


def test_entry_points_are_declared_and_bound():
    from multiposenet_amd import _lib
    from multiposenet_amd.inference import tta
    hdr = open(os.path.join(ROOT, "include", "mpn.h")).read()
    for name in ("mpn_mirror_images", "mpn_tta_merge"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert int(re.search(r"#define\s+MPN_TTA_MAX_SOURCES\s+(\d+)", hdr).group(1)) == tta.MAX_SOURCES == 8
    assert 2 * (1 + tta.MAX_SCALES) == tta.MAX_SOURCES
    import ctypes
    assert ctypes.sizeof(tta.Source) == 32
    # argument checks run before any HIP call
    with pytest.raises(ValueError, match="null"):
        _lib.call("mpn_mirror_images", None, 1, 1, 1, None, None)
    with pytest.raises(ValueError, match="sources"):
        _lib.call("mpn_tta_merge", ctypes.c_void_p(4096), 9, 1, 1, 1, ctypes.c_void_p(4096), ctypes.c_void_p(4096), None)
