"""`mpn_person_crops` (include/mpn.h) restated as plain loops: the rectangle of a person, where the resized part lies in the
crop, Pillow's `Image.resize((new_w, new_h), Image.BICUBIC, box=(x0, y0, x1, y1))` of the WHOLE frame as two passes of integer
arithmetic, and the slots of a record. Python floats are IEEE float64 and Python evaluates one operation at a time, in the
order written: every line below is the arithmetic of the header. tests/test_person_crops_host.py holds it against Pillow."""
import math

import numpy as np

PRECISION_BITS = 22
MAX_KSIZE = 65                                                      # MPN_IMAGE_RESIZE_MAX_KSIZE
FITS = ('stretch', 'pad')


def rect_of(box, h, w, pad):
    """box: four float32 (ymin, xmin, ymax, xmax) normalised to the frame -> ((x0, y0, x1, y1), empty, clipped)."""
    h, w, pad = float(h), float(w), float(pad)
    ymin, xmin, ymax, xmax = h * float(box[0]), w * float(box[1]), h * float(box[2]), w * float(box[3])
    bw = xmax - xmin
    bh = ymax - ymin
    px = pad * bw
    py = pad * bh
    x0, x1, y0, y1 = xmin - px, xmax + px, ymin - py, ymax + py
    if not all(math.isfinite(v) for v in (x0, y0, x1, y1)):
        return (0.0, 0.0, 0.0, 0.0), True, False
    clipped = False
    if x0 < 0.0:
        x0, clipped = 0.0, True
    if x1 > w:
        x1, clipped = w, True
    if y0 < 0.0:
        y0, clipped = 0.0, True
    if y1 > h:
        y1, clipped = h, True
    empty = not (x1 - x0 > 0.0) or not (y1 - y0 > 0.0)
    return (x0, y0, x1, y1), empty, clipped


def _rounded(v, most):
    """min(most, max(1, rint(v))) in float64, rint half to even (Python's `round`; an infinite v gives most)."""
    return int(min(float(most), max(1.0, float(np.rint(v)))))


def placement(rh, rw, H, W, fit):
    """(top, left, new_h, new_w) of an rh x rw rectangle in an H x W crop."""
    if fit == 'stretch':
        return 0, 0, H, W
    s = min(H / rh, W / rw)
    new_h, new_w = _rounded(rh * s, H), _rounded(rw * s, W)
    return (H - new_h) // 2, (W - new_w) // 2, new_h, new_w


def _bicubic(x, a=-0.5):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize_of(in0, in1, out):
    scale = (in1 - in0) / out
    support = 2.0 * max(scale, 1.0)
    return int(math.ceil(support)) * 2 + 1


def axis_taps(in0, in1, in_size, out):
    """The taps of one axis: [(first, [coefficients])] per output, Pillow's precompute_coeffs with a box."""
    scale = (in1 - in0) / out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    taps = []
    for xx in range(out):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        weights = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        total = 0.0
        for v in weights:
            total += v
        if total != 0.0:
            weights = [v / total for v in weights]
        taps.append((xmin, [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in weights]))
    return taps


def _clip8(acc):
    return min(max(acc >> PRECISION_BITS, 0), 255)


def resize_box(image, rect, new_h, new_w):
    """The two passes over the whole frame: horizontal first, rounded to uint8, then vertical. uint8 [new_h, new_w, 3]."""
    h, w, _ = image.shape
    x0, y0, x1, y1 = rect
    xt, yt = axis_taps(x0, x1, w, new_w), axis_taps(y0, y1, h, new_h)
    half = 1 << (PRECISION_BITS - 1)
    src = image.astype(np.int64)
    lo = min(first for first, _ in yt)
    hi = max(first + len(k) for first, k in yt)
    tmp = np.zeros((hi - lo, new_w, 3), np.int64)
    for xx, (first, k) in enumerate(xt):
        for r in range(lo, hi):
            for c in range(3):
                acc = half
                for j, v in enumerate(k):
                    acc += int(src[r, first + j, c]) * v
                tmp[r - lo, xx, c] = _clip8(acc)
    out = np.zeros((new_h, new_w, 3), np.uint8)
    for yy, (first, k) in enumerate(yt):
        for xx in range(new_w):
            for c in range(3):
                acc = half
                for j, v in enumerate(k):
                    acc += int(tmp[first + j - lo, xx, c]) * v
                out[yy, xx, c] = _clip8(acc)
    return out


def resize_box_fast(image, rect, new_h, new_w):
    """`resize_box` with the tap sums as integer numpy products (the same int64 values: tests hold the two together)."""
    h, w, _ = image.shape
    x0, y0, x1, y1 = rect
    xt, yt = axis_taps(x0, x1, w, new_w), axis_taps(y0, y1, h, new_h)
    half = 1 << (PRECISION_BITS - 1)
    lo = min(first for first, _ in yt)
    hi = max(first + len(k) for first, k in yt)
    src = image[lo:hi].astype(np.int64)
    tmp = np.zeros((hi - lo, new_w, 3), np.int64)
    for xx, (first, k) in enumerate(xt):
        acc = half + (src[:, first:first + len(k), :] * np.asarray(k, np.int64)[None, :, None]).sum(axis=1)
        tmp[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    out = np.zeros((new_h, new_w, 3), np.uint8)
    for yy, (first, k) in enumerate(yt):
        acc = half + (tmp[first - lo:first - lo + len(k)] * np.asarray(k, np.int64)[:, None, None]).sum(axis=0)
        out[yy] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def crop(image, box, size, pad=0.0, fit='stretch', fill=(0, 0, 0), fast=True):
    """One person of a uint8 [h, w, 3] frame -> (uint8 [H, W, 3], info): info = {'rect': four floats, 'placed': (top, left,
    new_h, new_w), 'empty', 'too_large', 'clipped'}."""
    H, W = size
    h, w, _ = image.shape
    rect, empty, clipped = rect_of(box, h, w, pad)
    out = np.empty((H, W, 3), np.uint8)
    out[...] = np.asarray(fill, np.uint8)
    info = {'rect': rect, 'placed': (0, 0, 0, 0), 'empty': empty, 'too_large': False, 'clipped': clipped}
    if empty:
        return out, info
    x0, y0, x1, y1 = rect
    top, left, new_h, new_w = info['placed'] = placement(y1 - y0, x1 - x0, H, W, fit)
    if ksize_of(x0, x1, new_w) > MAX_KSIZE or ksize_of(y0, y1, new_h) > MAX_KSIZE:
        info['too_large'] = True
        return out, info
    out[top:top + new_h, left:left + new_w] = (resize_box_fast if fast else resize_box)(image, rect, new_h, new_w)
    return out, info


def person_crops(images, boxes, slots, size, pad=0.0, fit='stretch', fill=(0, 0, 0)):
    """images: b frames; boxes: per frame float32 [n_i, 4] -> (crops uint8 [slots, H, W, 3], info): the persons in record order
    in the first sum(n_i) slots, every later slot zeros. info: 'rect' f64 [slots, 4], 'placed' int32 [slots, 4], 'empty',
    'too_large', 'clipped' and 'used' bool [slots]."""
    H, W = size
    out = np.zeros((slots, H, W, 3), np.uint8)
    info = {'rect': np.zeros((slots, 4), np.float64), 'placed': np.zeros((slots, 4), np.int32),
            'empty': np.zeros(slots, bool), 'too_large': np.zeros(slots, bool), 'clipped': np.zeros(slots, bool),
            'used': np.zeros(slots, bool)}
    s = 0
    for image, rows in zip(images, boxes):
        for box in np.asarray(rows, np.float32).reshape(-1, 4):
            out[s], one = crop(image, box, size, pad, fit, fill)
            info['used'][s] = True
            for key in ('rect', 'placed', 'empty', 'too_large', 'clipped'):
                info[key][s] = one[key]
            s += 1
    return out, info
