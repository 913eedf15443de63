"""The definition of `mpn_anonymize` (include/mpn.h) restated with numpy and plain loops: the yardstick of
tests/test_anonymize_gpu.py; tests/test_anonymize_host.py holds it against Pillow where Pillow draws the same thing (filled
rectangles) and checks its properties.

The arithmetic is the project's own, NOT Pillow's `reduce` / `GaussianBlur`: float64 bounds from the record's float32 values,
an integer half-open region, an integer ellipse test, and box means rounded as (2*S + n) // (2*n).

A `spec` is anything with the attributes of `inference.Anonymize` (region, mode, shape, blocks, radius, color, scale,
min_size, fallback, min_keypoint_score)."""
import math

import numpy as np

F64 = np.float64
FACE = 5                                # nose, eyes, ears: joints 0..4
BOUND = 2.0 ** 20
ELLIPSE_MAX = 32768


def region_of(box, keypoints, h, w, spec, with_keypoints=True):
    """box f32 [4] normalised (ymin, xmin, ymax, xmax), keypoints f32 [17, 3] (x, y, score) in image pixels (or None) ->
    (x0, y0, x1, y1), half-open, or None."""
    with np.errstate(all='ignore'):
        by0, bx0, by1, bx1 = F64(box[0]) * F64(h), F64(box[1]) * F64(w), F64(box[2]) * F64(h), F64(box[3]) * F64(w)
        if spec.region == 'box':
            fx0, fy0, fx1, fy1 = bx0, by0, bx1, by1
        else:
            face = []
            if with_keypoints and keypoints is not None:
                face = [j for j in range(FACE) if np.float32(keypoints[j][2]) >= np.float32(spec.min_keypoint_score)]
            if face:
                cx, cy = F64(0.0), F64(0.0)
                for j in face:
                    cx = cx + F64(keypoints[j][0])
                    cy = cy + F64(keypoints[j][1])
                cx, cy = cx / F64(len(face)), cy / F64(len(face))
                e = F64(0.0)
                for j in face:
                    d = abs(F64(keypoints[j][0]) - cx)
                    if d > e:
                        e = d
                    d = abs(F64(keypoints[j][1]) - cy)
                    if d > e:
                        e = d
                s = e * F64(spec.scale)
                t = (by1 - by0) * F64(spec.min_size)
                if t > s:
                    s = t
                fx0, fy0, fx1, fy1 = cx - s, cy - s, cx + s, cy + s
            else:
                fx0, fy0, fx1, fy1 = bx0, by0, bx1, by0 + (by1 - by0) * F64(spec.fallback)
    bounds = [float(v) for v in (fx0, fy0, fx1, fy1)]
    if not all(math.isfinite(v) for v in bounds):
        return None
    fx0, fy0, fx1, fy1 = (min(max(v, -BOUND), BOUND) for v in bounds)
    x0, y0, x1, y1 = math.floor(fx0), math.floor(fy0), math.ceil(fx1), math.ceil(fy1)
    if x1 - x0 <= 0 or y1 - y0 <= 0:
        return None
    return x0, y0, x1, y1


def covered(x, y, region, shape):
    """Is frame pixel (x, y) covered? Python integers: exact."""
    x0, y0, x1, y1 = region
    if not (x0 <= x < x1 and y0 <= y < y1):
        return False
    a, b = x1 - x0, y1 - y0
    if shape == 'rectangle' or a > ELLIPSE_MAX or b > ELLIPSE_MAX:
        return True
    u, v = 2 * x + 1 - (x0 + x1), 2 * y + 1 - (y0 + y1)
    return u * u * b * b + v * v * a * a <= a * a * b * b


def coverage(region, shape, h, w):
    """(ya, xa, mask): `covered` for every pixel of the region's part of an h x w frame, mask bool [yb - ya, xb - xa]
    (int64 arithmetic: at most 62 bits); None when the region misses the frame."""
    x0, y0, x1, y1 = region
    xa, xb, ya, yb = max(x0, 0), min(x1, w), max(y0, 0), min(y1, h)
    if xa >= xb or ya >= yb:
        return None
    mask = np.ones((yb - ya, xb - xa), bool)
    a, b = x1 - x0, y1 - y0
    if shape == 'ellipse' and a <= ELLIPSE_MAX and b <= ELLIPSE_MAX:
        u = (2 * np.arange(xa, xb, dtype=np.int64) + 1 - (x0 + x1))[None, :]
        v = (2 * np.arange(ya, yb, dtype=np.int64) + 1 - (y0 + y1))[:, None]
        mask = u * u * (b * b) + v * v * (a * a) <= a * a * b * b
    return ya, xa, mask


def box_mean_1d(a, radius, axis):
    """One 1-D box mean of an int64 array along `axis`: n = 2*radius + 1 samples, indices clamped to the array."""
    n = 2 * radius + 1
    length = a.shape[axis]
    total = np.zeros_like(a)
    for k in range(-radius, radius + 1):
        total += np.take(a, np.clip(np.arange(length) + k, 0, length - 1), axis=axis)
    return (2 * total + n) // (2 * n)


def blur(image, radius, passes=3):
    """The whole frame after `passes` passes of a horizontal then a vertical box mean, uint8 between them."""
    cur = image.astype(np.int64)
    for _ in range(passes):
        cur = box_mean_1d(cur, radius, 1)
        cur = box_mean_1d(cur, radius, 0)
    return cur.astype(np.uint8)


def blur_window(image, radius, ya, yb, xa, xb, passes=3):
    """`blur(image, radius)[ya:yb, xa:xb]`, computed from the window grown by passes * radius (clipped to the frame): a 1-D
    mean reaches `radius` far, so what the clamp at a cut that is not the frame's edge gets wrong travels `radius` a pass and
    ends outside [ya, yb) x [xa, xb). tests/test_anonymize_host.py holds this against `blur`."""
    h, w, _ = image.shape
    m = passes * radius
    y0, y1, x0, x1 = max(ya - m, 0), min(yb + m, h), max(xa - m, 0), min(xb + m, w)
    return blur(image[y0:y1, x0:x1], radius, passes)[ya - y0:yb - y0, xa - x0:xb - x0]


def anonymize(image, boxes, keypoints, spec, with_keypoints=True):
    """image uint8 [h, w, 3]; boxes f32 [n, 4]; keypoints f32 [n, 17, 3] or None -> the anonymised frame. Persons in order:
    the last one that covers a pixel gives its colour, and every person reads `image`, never `out`."""
    h, w, _ = image.shape
    out = image.copy()
    regions = [region_of(boxes[i], None if keypoints is None else keypoints[i], h, w, spec, with_keypoints) for i in range(len(boxes))]
    parts = [(r, coverage(r, spec.shape, h, w)) for r in regions if r is not None]
    parts = [(r, c) for r, c in parts if c is not None]
    blurred = None
    if spec.mode == 'blur' and parts:                               # one window around all regions
        wy0, wy1 = min(c[0] for _, c in parts), max(c[0] + c[2].shape[0] for _, c in parts)
        wx0, wx1 = min(c[1] for _, c in parts), max(c[1] + c[2].shape[1] for _, c in parts)
        blurred = blur_window(image, spec.radius, wy0, wy1, wx0, wx1)
    for (x0, y0, x1, y1), (ya, xa, mask) in parts:
        yb, xb = ya + mask.shape[0], xa + mask.shape[1]
        target = out[ya:yb, xa:xb]
        if spec.mode == 'fill':
            target[mask] = np.asarray(spec.color, np.uint8)
        elif spec.mode == 'blur':
            target[mask] = blurred[ya - wy0:yb - wy0, xa - wx0:xb - wx0][mask]
        else:
            c = -(-max(x1 - x0, y1 - y0) // spec.blocks)
            for j in range((ya - y0) // c, (yb - 1 - y0) // c + 1):
                for i in range((xa - x0) // c, (xb - 1 - x0) // c + 1):
                    ca, cb = max(x0 + i * c, 0), min(x0 + (i + 1) * c, w)       # the cell, clipped to the frame only
                    ra, rb = max(y0 + j * c, 0), min(y0 + (j + 1) * c, h)
                    cell = image[ra:rb, ca:cb].astype(np.int64).reshape(-1, 3)
                    n = len(cell)
                    mean = ((2 * cell.sum(axis=0) + n) // (2 * n)).astype(np.uint8)
                    # the cell's pixels inside the region's part of the frame
                    pa, pb, qa, qb = max(ca, xa), min(cb, xb), max(ra, ya), min(rb, yb)
                    sub = target[qa - ya:qb - ya, pa - xa:pb - xa]
                    sub[mask[qa - ya:qb - ya, pa - xa:pb - xa]] = mean
    return out


def pixel_keypoints(boxes, keypoint_scores, keypoint_positions, height, width):
    """mpn_pose_gather's float32 arithmetic: x = xmin*width + pos_x * (xmax*width - xmin*width), y likewise."""
    f = np.float32
    boxes = np.asarray(boxes, f).reshape(-1, 4)
    n = len(boxes)
    pos = np.asarray(keypoint_positions, f).reshape(n, 17, 2)
    out = np.zeros((n, 17, 3), f)
    for c, (lo_i, hi_i, size, p_i) in enumerate(((1, 3, f(width), 1), (0, 2, f(height), 0))):
        lo = (boxes[:, lo_i] * size).astype(f)[:, None]
        hi = (boxes[:, hi_i] * size).astype(f)[:, None]
        out[:, :, c] = (lo + (pos[:, :, p_i] * (hi - lo).astype(f)).astype(f)).astype(f)
    out[:, :, 2] = np.asarray(keypoint_scores, f).reshape(n, 17)
    return out


def anonymize_outputs(image, outputs, spec):
    """`anonymize` for a result dict: 'keypoints' if it is there, else the gather's arithmetic from 'keypoint_positions' and
    'keypoint_scores', else boxes only."""
    boxes = np.asarray(outputs['boxes'], np.float32).reshape(-1, 4)
    n = len(boxes)
    h, w, _ = image.shape
    if 'keypoints' in outputs and len(outputs['keypoints']) == n:
        return anonymize(image, boxes, np.asarray(outputs['keypoints'], np.float32), spec)
    if all(k in outputs and len(outputs[k]) == n for k in ('keypoint_positions', 'keypoint_scores')):
        return anonymize(image, boxes, pixel_keypoints(boxes, outputs['keypoint_scores'], outputs['keypoint_positions'], h, w), spec)
    return anonymize(image, boxes, None, spec, with_keypoints=False)
