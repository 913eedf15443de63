"""numpy restatement of `draw_everything` of the reference's inference/predict.ipynb (cells 10 and 12) - the yardstick of
tests/test_draw_gpu.py for `mpn_draw_detections` (include/mpn.h), proven against Pillow itself in tests/test_draw_host.py.
Nothing here imports Pillow.

The notebook copies the image, sets alpha 255 and draws, per person in order: the box outline in red, the 16 skeleton edges
as one-pixel white lines, the 17 keypoints as red dots of "radius" 2. Pillow converts every coordinate to int by truncation
toward zero and rasterises with integers only; a later primitive overwrites an earlier one; every pixel is clipped to the frame.

  rectangle (x0,y0)-(x1,y1), outline: rows y0 and y1 over x0..x1; columns x0 and x1 over y0+1..y1-1 - and, when y1 == y0, the
                two pixels (x0, y0+1), (x1, y0+1) (Pillow's edge loop walks from y0+1 towards y1 and excludes its end point).
  line          Bresenham from the FIRST point, the end point included: with n = max(|dx|, |dy|), step i = 0..n along the
                major axis, the minor axis has moved floor((2*m*i + n) / (2*n)) steps (m = min(|dx|, |dy|)): a tie moves.
  dot           ellipse over corners (x0,y0)-(x1,y1) with x1-x0, y1-y0 in {3, 4}: the bounding box without its four corner
                pixels, wherever it lies (STAMPS: one bit mask per row, bit i = pixel x0+i).
"""
import numpy as np

F = np.float32
K = 17
# the 16 limbs of the notebook's skeleton (cell 10) as (keypoint, keypoint), sorted: all lines of a person are white and follow
# each other, so their order among themselves does not show; the direction of a line does (the tie rule), and is the notebook's
EDGES = ((0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 7), (5, 11), (6, 8), (6, 12), (7, 9), (8, 10), (11, 13), (12, 14),
         (13, 15), (14, 16))
RED, WHITE = (255, 0, 0, 255), (255, 255, 255, 255)
RECT, LINE, DOT = 0, 1, 2

# (x1-x0, y1-y0) -> rows of the dot; established against Pillow 12.2.0 (test_draw_host.py sweeps them where Pillow exists)
STAMPS = {(3, 3): (0b0110, 0b1111, 0b1111, 0b0110),
          (3, 4): (0b0110, 0b1111, 0b1111, 0b1111, 0b0110),
          (4, 3): (0b01110, 0b11111, 0b11111, 0b01110),
          (4, 4): (0b01110, 0b11111, 0b11111, 0b11111, 0b01110)}


def trunc(v):
    """C's (int) of a double: toward zero."""
    return int(float(v))


def line_pixels(x0, y0, x1, y1):
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xs, ys = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    n, m = max(dx, dy), min(dx, dy)
    out = []
    for i in range(n + 1):
        k = (2 * m * i + n) // (2 * n) if n else 0
        out.append((x0 + xs * i, y0 + ys * k) if dx > dy else (x0 + xs * k, y0 + ys * i))
    return out


def rect_pixels(x0, y0, x1, y1):
    out = [(x, y) for y in (y0, y1) for x in range(x0, x1 + 1)]
    rows = range(y0 + 1, y1) if y1 > y0 else (y0 + 1,)
    return out + [(x, y) for y in rows for x in (x0, x1)]


def dot_pixels(x0, y0, x1, y1):
    rows = STAMPS.get((x1 - x0, y1 - y0))
    if rows is None:        # only where float32 no longer resolves x +- 2: beyond any frame
        return []
    return [(x0 + i, y0 + j) for j, bits in enumerate(rows) for i in range(x1 - x0 + 1) if bits >> i & 1]


PIXELS = {RECT: rect_pixels, LINE: line_pixels, DOT: dot_pixels}


def primitives(boxes, keypoint_positions, height, width):
    """The integer primitives of one frame in draw order: [(kind, x0, y0, x1, y1)], coordinates as the notebook's numpy
    arithmetic leaves them and Pillow truncates them. boxes f32 [n,4] normalised (ymin, xmin, ymax, xmax); keypoint_positions
    f32 [n,17,2] = (y, x) normalised to the box, or no rows at all (a detector without the PRN): boxes only."""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    pos = np.asarray(keypoint_positions, F).reshape(-1, K, 2)
    scaled = np.array([height, width, height, width]) * boxes               # int64 * float32 -> float64
    out = []
    for i, (ymin, xmin, ymax, xmax) in enumerate(scaled):
        out.append((RECT, trunc(xmin), trunc(ymin), trunc(xmax), trunc(ymax)))
        if len(pos) != len(boxes):
            continue
        kp = pos[i][:, [1, 0]].copy()
        kp *= np.array([xmax - xmin, ymax - ymin])                          # float64 product, rounded to float32
        kp += np.array([xmin, ymin])                                        # float64 sum, rounded to float32
        for p, q in EDGES:
            out.append((LINE, trunc(kp[p, 0]), trunc(kp[p, 1]), trunc(kp[q, 0]), trunc(kp[q, 1])))
        for x, y in kp:
            out.append((DOT, trunc(F(x) - F(2)), trunc(F(y) - F(2)), trunc(F(x) + F(2)), trunc(F(y) + F(2))))
    return out


def paint(rgba, prims):
    h, w = rgba.shape[:2]
    for kind, x0, y0, x1, y1 in prims:
        ink = WHITE if kind == LINE else RED
        if max(abs(x0), abs(y0), abs(x1), abs(y1)) > 1 << 20:
            raise ValueError("draw_ref: a coordinate beyond 2^20 (not a case of the restatement)")
        for x, y in PIXELS[kind](x0, y0, x1, y1):
            if 0 <= x < w and 0 <= y < h:
                rgba[y, x] = ink
    return rgba


def draw_everything(image, outputs):
    """uint8 [h,w,3], {'boxes', 'keypoint_positions'} -> uint8 [h,w,4]."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    h, w = image.shape[:2]
    rgba = np.concatenate([image, np.full((h, w, 1), 255, np.uint8)], axis=2)
    return paint(rgba, primitives(outputs["boxes"], outputs["keypoint_positions"], h, w))
