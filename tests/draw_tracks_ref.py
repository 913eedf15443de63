"""numpy restatement of the picture of `mpn_draw_tracks` (include/mpn.h) - the yardstick of tests/test_draw_tracks_gpu.py,
held against Pillow itself in tests/test_draw_tracks_host.py. Plain loops over integers; nothing here imports Pillow: the
digit stamps ([(mask uint8 [h, w], (ox, oy))] * 10, what `font.getmask2(d, 'L')` gives) and the cell width come in as
arguments. What is unchanged from `draw_everything` - the coordinate arithmetic, rectangle, line and dot rules, truncation -
is tests/draw_ref.py's.

Per kept person, in order: the box outline and the 17 dots in the identity colour palette[(track_id - 1) % P] (red for an
untracked person, track_id 0, or nothing at all with untracked='hide'), the 16 lines in line_color (white when untracked),
then - for a tracked person whose box is drawn - the label: a filled rectangle in the identity colour above the box (inside
it when it would leave the frame at the top), one cell per decimal digit, each digit's stamp blended in text_color by
BLEND8. A later primitive overwrites an earlier one; every pixel is clipped to the frame."""
import numpy as np

import draw_ref as R

F = np.float32
PAD = 1
FILL = 3                                                          # a label; R.RECT, R.LINE, R.DOT are 0, 1, 2
RED, WHITE = (255, 0, 0), (255, 255, 255)


def blend8(m, under, text):
    t = m * text + (255 - m) * under + 128
    return ((t >> 8) + t) >> 8


def metrics(stamps, cell):
    """(top, bot): the rows the digits cover, relative to the text's position. Every stamp lies at most the padding outside
    its cell, so that the label's rectangle encloses it whichever digit it is."""
    top = min(oy for _, (_, oy) in stamps)
    bot = max(oy + m.shape[0] for m, (_, oy) in stamps)
    assert all(ox >= -PAD and ox + m.shape[1] <= cell + PAD for m, (ox, _) in stamps)
    return top, bot


def label_box(x0, y0, track_id, stamps, cell):
    """The label of a box with the integer corner (x0, y0): (lx0, ly0, lw, lh)."""
    top, bot = metrics(stamps, cell)
    lw, lh = 2 * PAD + len(str(int(track_id))) * cell, 2 * PAD + (bot - top)
    return x0, (y0 - lh if y0 - lh >= 0 else y0), lw, lh


def label_pixels(x0, y0, track_id, stamps, cell, ink, text):
    """[(x, y, (r, g, b), blended)] of a label: every pixel of its rectangle. The colour starts as `ink`; the digits are
    drawn from the left, each blending `text` over what is there under its stamp (a glyph wider than its advance reaches
    into the next cell and is blended over there by the next digit too). blended: some stamp has 0 < m < 255 there."""
    lx0, ly0, lw, lh = label_box(x0, y0, track_id, stamps, cell)
    top, _ = metrics(stamps, cell)
    colour = [[list(ink) for _ in range(lw)] for _ in range(lh)]
    blended = [[False] * lw for _ in range(lh)]
    for k, d in enumerate(str(int(track_id))):
        mask, (ox, oy) = stamps[int(d)]
        ax, ay = PAD + k * cell + ox, PAD - top + oy                # the stamp's corner inside the rectangle
        assert ax >= 0 and ay >= 0 and ay + mask.shape[0] <= lh and ax + mask.shape[1] <= lw     # the rectangle encloses it
        for j in range(mask.shape[0]):
            for i in range(mask.shape[1]):
                m = int(mask[j, i])
                colour[ay + j][ax + i] = [blend8(m, u, t) for u, t in zip(colour[ay + j][ax + i], text)]
                blended[ay + j][ax + i] |= 0 < m < 255
    return [(lx0 + i, ly0 + j, tuple(colour[j][i]), blended[j][i]) for j in range(lh) for i in range(lw)]


def smoothed_primitives(keypoints):
    """Lines and dots of one person from float32 (x, y[, score]) rows: [(kind, x0, y0, x1, y1)]."""
    kp = np.asarray(keypoints, F)
    out = [(R.LINE, R.trunc(kp[p, 0]), R.trunc(kp[p, 1]), R.trunc(kp[q, 0]), R.trunc(kp[q, 1])) for p, q in R.EDGES]
    for x, y in kp[:, :2]:
        out.append((R.DOT, R.trunc(F(x) - F(2)), R.trunc(F(y) - F(2)), R.trunc(F(x) + F(2)), R.trunc(F(y) + F(2))))
    return out


def primitives(outputs, height, width, style, stamps, cell):
    """The frame's primitives in draw order: [(kind, x0, y0, x1, y1, ink, text, track_id)]. style: anything with
    TrackStyle's attributes. outputs: 'boxes', 'keypoint_positions' (no rows: boxes and labels only), 'track_ids' and, for
    keypoints='smoothed', 'keypoints_smoothed'."""
    boxes = np.asarray(outputs["boxes"], F).reshape(-1, 4)
    pos = np.asarray(outputs["keypoint_positions"], F).reshape(-1, R.K, 2)
    ids = np.asarray(outputs["track_ids"]).reshape(-1)
    assert len(ids) == len(boxes)
    smoothed = None
    if style.keypoints == "smoothed":
        smoothed = np.asarray(outputs["keypoints_smoothed"], F).reshape(-1, R.K, 3)
    with_keypoints = len(pos if smoothed is None else smoothed) == len(boxes)
    out = []
    for i, track_id in enumerate(int(t) for t in ids):
        if track_id <= 0 and style.untracked == "hide":
            continue
        ink = tuple(style.palette[(track_id - 1) % len(style.palette)]) if track_id > 0 else RED
        line = tuple(style.line_color) if track_id > 0 else WHITE
        own = R.primitives(boxes[i:i + 1], pos[i:i + 1] if with_keypoints else np.zeros((0, R.K, 2), F), height, width)
        if smoothed is not None and with_keypoints:
            own = own[:1] + smoothed_primitives(smoothed[i])
        _, x0, y0, x1, y1 = own[0]
        box_drawn = x1 >= x0 and y1 >= y0                           # (Pillow refuses an inverted box)
        for kind, *c in own[0 if box_drawn else 1:]:
            out.append((kind, *c, line if kind == R.LINE else ink, None, track_id))
        if track_id > 0 and style.labels and box_drawn:
            out.append((FILL, x0, y0, x0, y0, ink, tuple(style.text_color), track_id))
    return out


def paint(rgba, prims, stamps, cell):
    h, w = rgba.shape[:2]
    for kind, x0, y0, x1, y1, ink, text, track_id in prims:
        if max(abs(x0), abs(y0), abs(x1), abs(y1)) > 1 << 20:
            raise ValueError("draw_tracks_ref: a coordinate beyond 2^20 (not a case of the restatement)")
        if kind == FILL:
            for x, y, colour, _ in label_pixels(x0, y0, track_id, stamps, cell, ink, text):
                if 0 <= x < w and 0 <= y < h:
                    rgba[y, x] = colour + (255,)
            continue
        for x, y in R.PIXELS[kind](x0, y0, x1, y1):
            if 0 <= x < w and 0 <= y < h:
                rgba[y, x] = ink + (255,)
    return rgba


def draw_tracks(image, outputs, style, stamps, cell):
    """uint8 [h,w,3], the outputs of a tracked call, a TrackStyle (or its attributes), the digit stamps -> uint8 [h,w,4]."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    h, w = image.shape[:2]
    rgba = np.concatenate([image, np.full((h, w, 1), 255, np.uint8)], axis=2)
    return paint(rgba, primitives(outputs, h, w, style, stamps, cell), stamps, cell)


def blended_label_pixels(outputs, height, width, style, stamps, cell):
    """How many pixels inside the frame lie under a digit stamp with 0 < m < 255: neither colour, a blend."""
    n = 0
    for kind, x0, y0, _, _, ink, text, track_id in primitives(outputs, height, width, style, stamps, cell):
        if kind == FILL:
            n += sum(0 <= x < width and 0 <= y < height and b for x, y, _, b in label_pixels(x0, y0, track_id, stamps, cell, ink, text))
    return n
