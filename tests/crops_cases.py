"""Handmade cases for `mpn_person_crops`: frames of 37 x 53, 64 x 48 and 208 x 16 pixels (height x width) and crops of
(16, 8), (24, 16) and (8, 8). A case is one record: `images`, per image its `boxes` (float32 [n, 4], normalised (ymin, xmin,
ymax, xmax)), the crop `size`, `pad` and `max_boxes`; every case runs with both fits and the fill below.

A box is given in pixels and divided by the frame's size in float32, so a bound is exact only where pixel / size is: on the 64
rows of the second frame, on the 16 columns of the third, and at multiples of 3 on the 48 columns of the second. No box is
exact on both axes of one of these frames at the crops' sizes, so each axis has its own unscaled case."""
import numpy as np

F = np.float32
FILL = (7, 130, 255)
SIZES = {'small': (37, 53), 'square': (64, 48), 'tall': (208, 16)}


def frame(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def box(h, w, y0, x0, y1, x1):
    """Pixel bounds -> the float32 normalised box."""
    return np.array([F(y0) / F(h), F(x0) / F(w), F(y1) / F(h), F(x1) / F(w)], F)


def _boxes(name, rows):
    h, w = SIZES[name]
    return np.stack([box(h, w, *r) for r in rows]).astype(F) if rows else np.zeros((0, 4), F)


def _case(name, frames, size, pad=0.0, max_boxes=4):
    """frames: [(which frame, [pixel boxes])]"""
    images = [frame(11 + i, *SIZES[which]) for i, (which, _) in enumerate(frames)]
    return dict(name=name, images=images, boxes=[_boxes(which, rows) for which, rows in frames], size=size, pad=pad,
                max_boxes=max_boxes, fill=FILL)


def cases():
    nan_box = box(37, 53, 5, 6, 20, 30)
    nan_box[2] = np.nan
    empties = _case("empty", [('small', [(40, 60, 50, 70), (5, 20, 30, 20), (5, 6, 20, 30), (4.5, 7.25, 21.75, 19.5)])], (16, 8))
    empties['boxes'][0][2] = nan_box
    out = [
        _case("inside_fractional", [('small', [(3.3, 10.6, 30.9, 41.2)])], (16, 8)),
        _case("pad_clipped", [('small', [(2, 3, 20, 30), (20, 35, 36, 52)])], (24, 16), pad=0.25),
        empties,
        _case("enlarged", [('small', [(10.2, 20.1, 13.7, 24.7)])], (24, 16)),
        # 16 rows at the integer offset 10 and at 10.5: the vertical taps are the identity; 12 columns -> 8
        _case("unscaled_rows", [('square', [(10, 12, 26, 24), (10.5, 12, 26.5, 24)])], (16, 8)),
        # 8 columns at the integer offset 4 and at 4.5: the horizontal taps are the identity
        _case("unscaled_columns", [('tall', [(30, 4, 52, 12), (30, 4.5, 52, 12.5)])], (8, 8)),
        # 200 rows -> 8: 25x, refused; 120 rows -> 8: 15x, and 128 rows -> 8: 16x, the last ratio the tap rows hold
        _case("reduced", [('tall', [(4, 2, 204, 14), (40, 0, 160, 16), (40, 1, 168, 15)])], (8, 8)),
        # fit='pad': a tall box of 32 x 9 -> 16 x 4.5 -> 4 columns (half to even), 32 x 15 -> 7.5 -> 8; a wide one of 10 x 36
        _case("tall_and_wide", [('square', [(8, 12, 40, 21), (8, 12, 40, 27), (20, 6, 30, 42)])], (16, 8)),
        _case("nobody_in_the_first", [('small', []), ('square', [(5, 5, 50, 40)])], (8, 8)),
        _case("every_slot", [('small', [(1, 1, 30, 20), (5, 25, 36, 50), (0, 0, 37, 53)]),
                             ('small', [(10, 10, 20, 20), (2, 30, 35, 45), (15, 5, 33, 48)])], (8, 8), max_boxes=3),
        _case("three_sizes", [('small', [(3, 4, 33, 40), (10, 30, 30, 52)]), ('square', [(1.5, 2.5, 60, 44)]),
                              ('tall', [(20, 1, 100, 15), (100, 0, 208, 16)])], (8, 8), pad=0.1),
    ]
    return out


def check_cases(R):
    """What the cases are meant to hit, asserted on the reference `R` (tests/crops_ref.py): a case that no longer does fails
    here, not silently."""
    by_name = {c['name']: c for c in cases()}

    def infos(name, fit):
        c = by_name[name]
        return R.person_crops(c['images'], c['boxes'], len(c['images']) * c['max_boxes'], c['size'], c['pad'], fit, c['fill'])[1]
    i = infos("pad_clipped", 'stretch')
    assert i['clipped'].tolist()[:2] == [True, True] and not i['empty'][:2].any()
    assert i['rect'][0, 0] == 0.0 and i['rect'][0, 1] == 0.0 and i['rect'][1, 2] == 53.0 and i['rect'][1, 3] == 37.0
    i = infos("empty", 'stretch')
    assert i['empty'].tolist() == [True, True, True, False] and i['clipped'].tolist() == [True, False, False, False]
    i = infos("unscaled_rows", 'stretch')
    assert (i['rect'][:2, 3] - i['rect'][:2, 1]).tolist() == [16.0, 16.0] and i['rect'][:2, 1].tolist() == [10.0, 10.5]
    i = infos("unscaled_columns", 'stretch')
    assert (i['rect'][:2, 2] - i['rect'][:2, 0]).tolist() == [8.0, 8.0] and i['rect'][:2, 0].tolist() == [4.0, 4.5]
    for fit in R.FITS:
        i = infos("reduced", fit)
        assert i['too_large'].tolist()[:3] == [True, False, False]
    c = by_name["reduced"]
    rect = i['rect'][1]
    assert R.ksize_of(rect[1], rect[3], 8) in (61, 63) and R.ksize_of(i['rect'][2, 1], i['rect'][2, 3], 8) == 65
    i = infos("tall_and_wide", 'pad')
    assert i['placed'].tolist()[:3] == [[0, 2, 16, 4], [0, 0, 16, 8], [7, 0, 2, 8]]
    i = infos("every_slot", 'stretch')
    assert i['used'].all()
    i = infos("nobody_in_the_first", 'stretch')
    assert i['used'].tolist() == [True] + [False] * 7
