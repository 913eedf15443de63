"""The definition of mpn_density_map and mpn_draw_density (include/mpn.h) as plain Python loops: the anchor is zones_ref's f64
arithmetic, unrounded; the state and the picture are integer arithmetic. Produces the rows, the state bytes and the snapshots
the map kernel must equal byte for byte, and the RGBA frames the drawing must. Written from the header, not from the kernels."""
import numpy as np

import zones_ref

SLOTS = 64
FLAG_TRACKED, FLAG_ANKLES, FLAG_NO_ANCHOR, FLAG_OUTSIDE, FLAG_VISIT = 1, 2, 4, 8, 16
FEET, BOX_BOTTOM, BOX_CENTRE = zones_ref.FEET, zones_ref.BOX_BOTTOM, zones_ref.BOX_CENTRE
ANCHOR, BOX = 0, 1
DWELL, VISITS = 0, 1
SATURATED = 2 ** 32 - 1
f64 = np.float64

SLOT = np.dtype([('id', np.int32), ('last', np.int32), ('cell1', np.int32), ('pad', np.int32)])
ROW = np.dtype([('row', np.int32), ('col', np.int32), ('flags', np.uint32), ('cells', np.uint32)])
IMAGE = np.dtype([('max_dwell', np.uint32), ('max_visits', np.uint32), ('counted', np.uint32), ('visits', np.uint32)])


def grid_of(frame_size, cell):
    return -(-int(frame_size[0]) // cell), -(-int(frame_size[1]) // cell)


def state_dtype(gh, gw):
    d = np.dtype([('frames', np.int32), ('max_dwell', np.uint32), ('max_visits', np.uint32), ('pad', np.int32, (5,)),
                  ('slots', SLOT, (SLOTS,)), ('dwell', np.uint32, (gh, gw)), ('visits', np.uint32, (gh, gw))])
    assert d.itemsize == 32 + 64 * 16 + 8 * gh * gw
    return d


class Params:
    """The by-value parameters of mpn_density_map."""

    def __init__(self, frame_size, cell=16, footprint=ANCHOR, anchor=FEET, min_keypoint_score=0.0, half_life=0, show=DWELL):
        self.height, self.width, self.cell = int(frame_size[0]), int(frame_size[1]), int(cell)
        self.gh, self.gw = grid_of(frame_size, cell)
        self.footprint, self.half_life, self.show = int(footprint), int(half_life), int(show)
        self.geo = zones_ref.Geometry(frame_size, anchor=anchor, min_keypoint_score=min_keypoint_score)


def new_state(streams, params):
    return np.zeros(streams, state_dtype(params.gh, params.gw))


def saturating_increment(plane, r, c):
    plane[r, c] = min(int(plane[r, c]) + 1, SATURATED)
    return int(plane[r, c])


def footprint_of(params, box, inside_cell):
    """The cells (r, c) a row with an anchor adds to."""
    if params.footprint == ANCHOR:
        return [inside_cell] if inside_cell is not None else []
    with np.errstate(all='ignore'):
        y0, x0 = f64(box[0]) * f64(params.height), f64(box[1]) * f64(params.width)
        y1, x1 = f64(box[2]) * f64(params.height), f64(box[3]) * f64(params.width)
    if not all(np.isfinite(v) for v in (x0, x1, y0, y1)):
        return []
    s = params.cell
    columns = [c for c in range(params.gw) if x0 <= f64((2 * c + 1) * s) * f64(0.5) < x1]
    return [(r, c) for r in range(params.gh) if y0 <= f64((2 * r + 1) * s) * f64(0.5) < y1 for c in columns]


def run(params, outputs, state, max_boxes, total=None, tracked=True):
    """outputs: b = streams * F dicts with 'boxes' f32 [n, 4] and, optionally, 'keypoints' f32 [n, 17, 3] and 'track_ids' int [n];
    state: `new_state(streams, params)`, advanced in place. total: the record's total where it is smaller than the sum of the
    counts. tracked=False: the launch without track_rows. -> (rows ROW [b * max_boxes], images IMAGE [b], snapshots uint32
    [b, gh, gw])."""
    b, streams = len(outputs), len(state)
    assert b % streams == 0
    F = b // streams
    rows, images = np.zeros(b * max_boxes, ROW), np.zeros(b, IMAGE)
    snapshots = np.zeros((b, params.gh, params.gw), np.uint32)
    counts = [len(o['boxes']) for o in outputs]
    if total is None:
        total = sum(counts)
    total = max(0, min(total, b * max_boxes))
    for s in range(streams):
        st = state[s]
        slots, dwell, visits = st['slots'], st['dwell'], st['visits']
        for j in range(F):
            i = s * F + j
            now = int(st['frames']) + j + 1
            first = min(sum(counts[:i]), total)
            n = min(counts[i], max_boxes, total - first)
            o = outputs[i]
            if params.half_life > 0 and now % params.half_life == 0:        # 1. halving
                dwell >>= 1
                visits >>= 1
                st['max_dwell'] >>= 1
                st['max_visits'] >>= 1
            anchors = [zones_ref.anchor_of(params.geo, o['boxes'][r], o['keypoints'][r] if 'keypoints' in o else None) for r in range(n)]
            ids = [int(o['track_ids'][r]) if tracked else 0 for r in range(n)]
            taken, slot_of = set(), [None] * n                      # 2. the slots, serially in row order
            for r in range(n):
                if ids[r] <= 0 or anchors[r] is None:
                    continue
                match = [k for k in range(SLOTS) if int(slots[k]['id']) == ids[r]]
                if match:
                    if match[0] in taken:
                        continue                                    # the second row with one id: untracked
                    k = match[0]
                else:
                    k = min((int(slots[k]['last']), k) for k in range(SLOTS) if k not in taken)[1]
                    slots[k] = np.zeros((), SLOT)
                    slots[k]['id'] = ids[r]
                taken.add(k)
                slot_of[r] = k
            counted = visited = 0
            for r in range(n):
                row = rows[first + r]
                row['row'] = row['col'] = -1
                if anchors[r] is None:
                    row['flags'] = FLAG_NO_ANCHOR
                    continue
                cx, cy, from_ankles = anchors[r]
                flags = FLAG_ANKLES if from_ankles else 0
                cell = None
                if 0 <= cx < params.width and 0 <= cy < params.height:
                    cell = (int(cy) // params.cell, int(cx) // params.cell)
                    row['row'], row['col'] = cell
                else:
                    flags |= FLAG_OUTSIDE
                if slot_of[r] is not None:                          # 3.
                    slot = slots[slot_of[r]]
                    flags |= FLAG_TRACKED
                    if cell is not None:
                        k = cell[0] * params.gw + cell[1]
                        if int(slot['cell1']) != k + 1:
                            flags |= FLAG_VISIT
                            visited += 1
                            st['max_visits'] = max(int(st['max_visits']), saturating_increment(visits, *cell))      # 5.
                        slot['cell1'] = k + 1
                    else:
                        slot['cell1'] = 0
                    slot['last'] = now
                cells = footprint_of(params, o['boxes'][r], cell)   # 4.
                for rc in cells:
                    st['max_dwell'] = max(int(st['max_dwell']), saturating_increment(dwell, *rc))                   # 5.
                counted += bool(cells)
                row['flags'], row['cells'] = flags, len(cells)
            images[i] = (st['max_dwell'], st['max_visits'], counted, visited)
            snapshots[i] = visits if params.show == VISITS else dwell         # 6.
        st['frames'] += F
    return rows, images, snapshots


def packed(rows, images):
    """The bytes of mpn_density_map's out."""
    return np.concatenate([rows.view(np.uint8), images.view(np.uint8)])


def unpacked(rows, images, counts):
    """The rows of `run` as the dicts `DensityMap.unpack` gives (for whole records: total = the sum of the counts)."""
    res, s = [], 0
    for i, n in enumerate(counts):
        r = rows[s:s + n]
        res.append({'cell': np.stack([r['row'], r['col']], axis=1).astype(np.int32).reshape(n, 2), 'cells': r['cells'].astype(np.int32),
                    'tracked': (r['flags'] & FLAG_TRACKED) != 0, 'visit': (r['flags'] & FLAG_VISIT) != 0,
                    'outside': (r['flags'] & FLAG_OUTSIDE) != 0, 'anchor_from_keypoints': (r['flags'] & FLAG_ANKLES) != 0,
                    'max_dwell': int(images[i]['max_dwell']), 'max_visits': int(images[i]['max_visits']),
                    'counted': int(images[i]['counted']), 'visits': int(images[i]['visits'])})
        s += n
    return res


# ------------------------------------------------------------------------------------------------------------------ the picture
def blend8(m, under, ink):
    t = m * ink + (255 - m) * under + 128
    return ((t >> 8) + t) >> 8


def alpha_table(opacity):
    return [0] + [(opacity * l + 127) // 255 for l in range(1, 256)]


def cell_levels(grid, scale):
    """uint32 [gh, gw] and M -> the cells' levels as a list of lists of ints; M = 0: None (the image is left alone)."""
    if scale == 0:
        return None
    return [[min(255, (255 * int(v) + scale // 2) // scale) for v in row] for row in grid]


def _between(v, s, n, smooth):
    if not smooth:
        return v // s, v // s, 0
    u = 2 * v + 1 - s
    q = u // (2 * s)                                                # Python's // is the floor
    return min(max(q, 0), n - 1), min(max(q + 1, 0), n - 1), u - q * 2 * s


def pixel_level(levels, y, x, cell, smooth):
    gh, gw = len(levels), len(levels[0])
    r0, r1, fy = _between(y, cell, gh, smooth)
    c0, c1, fx = _between(x, cell, gw, smooth)
    s2 = 2 * cell
    return (levels[r0][c0] * (s2 - fx) * (s2 - fy) + levels[r0][c1] * fx * (s2 - fy) + levels[r1][c0] * (s2 - fx) * fy +
            levels[r1][c1] * fx * fy + 2 * cell * cell) // (4 * cell * cell)


def level_image(grid, scale, height, width, cell, smooth):
    """The pixels' levels, uint8 [height, width], or None where the image is left alone."""
    levels = cell_levels(grid, scale)
    if levels is None:
        return None
    return np.array([[pixel_level(levels, y, x, cell, smooth) for x in range(width)] for y in range(height)], np.uint8)


def draw_arrays(rgba, grid, max_shown, cell, smooth, full_scale, opacity, colormap):
    """`draw` with the same integer arithmetic on whole arrays, for frames too large for the loops; tests/test_density_host.py
    holds it against `draw`. Returns a new array."""
    h, w = rgba.shape[:2]
    scale = full_scale if full_scale else int(max_shown)
    if scale == 0:
        return rgba.copy()
    levels = np.minimum(255, (255 * grid.astype(np.int64) + scale // 2) // scale)
    gh, gw = levels.shape

    def between(v, n):
        if not smooth:
            return v // cell, v // cell, np.zeros_like(v)
        u = 2 * v + 1 - cell
        q = u // (2 * cell)                                         # numpy's // is the floor
        return np.clip(q, 0, n - 1), np.clip(q + 1, 0, n - 1), u - q * 2 * cell
    r0, r1, fy = (a[:, None] for a in between(np.arange(h, dtype=np.int64), gh))
    c0, c1, fx = (a[None, :] for a in between(np.arange(w, dtype=np.int64), gw))
    s2 = 2 * cell
    level = (levels[r0, c0] * (s2 - fx) * (s2 - fy) + levels[r0, c1] * fx * (s2 - fy) + levels[r1, c0] * (s2 - fx) * fy +
             levels[r1, c1] * fx * fy + 2 * cell * cell) // (4 * cell * cell)
    alpha = np.array(alpha_table(opacity), np.int64)[level][..., None]
    ink = np.asarray(colormap, np.int64)[level]
    t = alpha * ink + (255 - alpha) * rgba[..., :3].astype(np.int64) + 128
    out = rgba.copy()
    out[..., :3] = np.where(alpha > 0, ((t >> 8) + t) >> 8, rgba[..., :3])
    out[..., 3] = np.where(alpha[..., 0] > 0, 255, rgba[..., 3])
    return out


def draw(rgba, grid, max_shown, cell, smooth, full_scale, opacity, colormap):
    """rgba: uint8 [h, w, 4], changed in place and returned; grid: the shown plane uint32 [gh, gw]; max_shown: the image row's
    maximum of it. Where the level's alpha is > 0 every channel becomes BLEND8(alpha, pixel, colour) and the alpha byte 255."""
    h, w = rgba.shape[:2]
    levels = level_image(grid, full_scale if full_scale else int(max_shown), h, w, cell, smooth)
    if levels is None:
        return rgba
    alpha = alpha_table(opacity)
    for y in range(h):
        for x in range(w):
            level = int(levels[y, x])
            if alpha[level] > 0:
                for c in range(3):
                    rgba[y, x, c] = blend8(alpha[level], int(rgba[y, x, c]), int(colormap[level][c]))
                rgba[y, x, 3] = 255
    return rgba
