"""The definition of mpn_track_trails and mpn_draw_trails (include/mpn.h) as plain Python loops: the anchor is zones_ref's f64
arithmetic, rounded once to f32; the state is integers and f32 pairs; the picture is integer arithmetic. Produces the rows and
the state bytes the history kernel must equal byte for byte, and the RGBA frames the drawing must. Written from the header,
not from the kernels."""
import numpy as np

import zones_ref

SLOTS = 64
FLAG_TRACKED, FLAG_ANKLES, FLAG_NO_ANCHOR, FLAG_APPENDED, FLAG_RESTARTED = 1, 2, 4, 8, 16
FEET, BOX_BOTTOM, BOX_CENTRE = zones_ref.FEET, zones_ref.BOX_BOTTOM, zones_ref.BOX_CENTRE
COORD_MAX = 1 << 29


def slot_dtype(K):
    return np.dtype([('id', np.int32), ('last', np.int32), ('last_append', np.int32), ('count', np.int32), ('head', np.int32),
                     ('pad', np.int32, (3,)), ('ring', np.float32, (K, 2))])


def state_dtype(K):
    d = np.dtype([('frames', np.int32), ('pad', np.int32, (3,)), ('slots', slot_dtype(K), (SLOTS,))])
    assert d.itemsize == 16 + 64 * (32 + 8 * K)
    return d


def row_dtype(K):
    d = np.dtype([('n', np.int32), ('flags', np.uint32), ('points', np.float32, (K + 1, 2))])
    assert d.itemsize == 8 * (K + 2)
    return d


class Params:
    """The by-value parameters of mpn_track_trails."""

    def __init__(self, frame_size, length=32, every=1, max_gap=30, anchor=FEET, min_keypoint_score=0.0):
        self.length, self.every, self.max_gap = int(length), int(every), int(max_gap)
        self.geo = zones_ref.Geometry(frame_size, anchor=anchor, min_keypoint_score=min_keypoint_score)


def new_state(streams, K):
    return np.zeros(streams, state_dtype(K))


def anchor_of(params, box, keypoints):
    """(x, y as f32, from_ankles) of one person, or None: zones' anchor, each coordinate rounded once to f32; not finite before
    or after the rounding: no anchor."""
    a = zones_ref.anchor_of(params.geo, box, keypoints)
    if a is None:
        return None
    with np.errstate(all='ignore'):
        x, y = np.float32(a[0]), np.float32(a[1])
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    return x, y, a[2]


def run(params, outputs, state, max_boxes, total=None):
    """outputs: b = streams * F dicts with 'boxes' f32 [n, 4], 'track_ids' int [n] and, optionally, 'keypoints' f32 [n, 17, 3];
    state: `new_state(streams, K)`, advanced in place. total: the record's total where it is smaller than the sum of the counts.
    -> rows `row_dtype(K)` [b * max_boxes]."""
    K = params.length
    b, streams = len(outputs), len(state)
    assert b % streams == 0
    F = b // streams
    rows = np.zeros(b * max_boxes, row_dtype(K))
    counts = [len(o['boxes']) for o in outputs]
    if total is None:
        total = sum(counts)
    total = max(0, min(total, b * max_boxes))
    for s in range(streams):
        st = state[s]
        slots = st['slots']
        for j in range(F):
            i = s * F + j
            now = int(st['frames']) + j + 1
            first = min(sum(counts[:i]), total)
            n = min(counts[i], max_boxes, total - first)
            o = outputs[i]
            anchors = [anchor_of(params, o['boxes'][r], o['keypoints'][r] if 'keypoints' in o else None) for r in range(n)]
            ids = [int(o['track_ids'][r]) for r in range(n)]
            # 1. the slots, serially in row order
            taken, slot_of = set(), [None] * n
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
                    slots[k] = np.zeros((), slots.dtype)
                    slots[k]['id'] = ids[r]
                taken.add(k)
                slot_of[r] = k
            for r in range(n):
                row = rows[first + r]
                if anchors[r] is None:
                    row['flags'] = FLAG_NO_ANCHOR
                    continue
                cx, cy, from_ankles = anchors[r]
                flags = FLAG_ANKLES if from_ankles else 0
                if slot_of[r] is None:                              # 6. untracked
                    row['n'], row['flags'] = 1, flags
                    row['points'][0] = (cx, cy)
                    continue
                flags |= FLAG_TRACKED
                slot = slots[slot_of[r]]
                if int(slot['count']) > 0 and params.max_gap > 0 and now - int(slot['last']) > params.max_gap:      # 2. restart
                    keep = int(slot['id'])
                    slots[slot_of[r]] = np.zeros((), slots.dtype)
                    slot = slots[slot_of[r]]
                    slot['id'] = keep
                    flags |= FLAG_RESTARTED
                count, head = int(slot['count']), int(slot['head'])
                points = []
                if count == 0 or now - int(slot['last_append']) >= params.every:        # 3. append
                    head = 0 if count == 0 else (head + 1) % K
                    slot['ring'][head] = (cx, cy)
                    count = min(count + 1, K)
                    slot['last_append'] = now
                    flags |= FLAG_APPENDED
                else:
                    points.append((cx, cy))
                slot['count'], slot['head'], slot['last'] = count, head, now        # 4.
                points += [tuple(slot['ring'][(head - q + K) % K]) for q in range(count)]     # 5. newest first
                row['n'], row['flags'] = len(points), flags
                row['points'][:len(points)] = points
        st['frames'] += F
    return rows


def unpacked(rows, counts):
    """The rows of `run` as the dicts `TrackTrails.unpack` gives (for whole records: total = the sum of the counts)."""
    res, s = [], 0
    for n in counts:
        r = rows[s:s + n]
        res.append({'points': r['points'].copy(), 'count': r['n'].copy(), 'tracked': (r['flags'] & FLAG_TRACKED) != 0,
                    'appended': (r['flags'] & FLAG_APPENDED) != 0, 'restarted': (r['flags'] & FLAG_RESTARTED) != 0,
                    'anchor_from_keypoints': (r['flags'] & FLAG_ANKLES) != 0})
        s += n
    return res


# ------------------------------------------------------------------------------------------------------------------ the picture
def trunc(v):
    """An f32 coordinate -> int: clamped to +-2^29 (a NaN becomes the lower bound), then toward zero."""
    v = float(v)
    if v != v:
        return -COORD_MAX
    return int(min(max(v, -float(COORD_MAX)), float(COORD_MAX)))


def segment_pixels(x0, y0, x1, y1, height, width):
    """The pixels of mpn_draw_detections' `line` from (x0, y0), end point included, that lie inside the frame: at step i of the
    major axis the minor axis has moved floor((2*m*i + n) / (2*n)) steps. Only the steps that can hit the frame are walked."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xs, ys = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    out = []
    if dx > dy:
        for x in range(max(min(x0, x1), 0), min(max(x0, x1), width - 1) + 1):
            i = (x - x0) * xs
            y = y0 + ys * ((2 * dy * i + dx) // (2 * dx))
            if 0 <= y < height:
                out.append((x, y))
    else:
        for y in range(max(min(y0, y1), 0), min(max(y0, y1), height - 1) + 1):
            i = (y - y0) * ys
            x = x0 + xs * ((2 * dx * i + dy) // (2 * dy)) if dy else x0
            if 0 <= x < width:
                out.append((x, y))
    return out


def blend8(m, under, ink):
    t = m * ink + (255 - m) * under + 128
    return ((t >> 8) + t) >> 8


def segment_alpha(s, K, fade, min_alpha):
    return 255 - (s * (255 - min_alpha)) // max(K - 1, 1) if fade else 255


def segments(points, count, tracked, track_ids, K, palette, fade, min_alpha):
    """The segments of one image in draw order: [((x0, y0), (x1, y1), (r, g, b), alpha)], from the older point to the newer."""
    out = []
    for pts, n, is_tracked, tid in zip(points, count, tracked, track_ids):
        n = max(0, min(int(n), K + 1))
        if not is_tracked or n < 2 or int(tid) <= 0:
            continue
        ink = palette[(int(tid) - 1) % len(palette)]
        for s in range(n - 2, -1, -1):                              # the oldest first
            a = (trunc(pts[s + 1][0]), trunc(pts[s + 1][1]))
            b = (trunc(pts[s][0]), trunc(pts[s][1]))
            out.append((a, b, ink, segment_alpha(s, K, fade, min_alpha)))
    return out


def draw(rgba, trails, track_ids, K, palette, fade=True, min_alpha=64, touched=None):
    """rgba: uint8 [h, w, 4], changed in place and returned; trails: a dict of `unpacked`. Every pixel of a segment becomes
    BLEND8(alpha, pixel, ink) per colour channel, its alpha byte 255; segments in order, a pixel under two of them twice.
    touched: a dict that counts the blends per pixel."""
    h, w = rgba.shape[:2]
    for a, b, ink, alpha in segments(trails['points'], trails['count'], trails['tracked'], track_ids, K, palette, fade, min_alpha):
        for x, y in segment_pixels(a[0], a[1], b[0], b[1], h, w):
            for c in range(3):
                rgba[y, x, c] = blend8(alpha, int(rgba[y, x, c]), ink[c])
            rgba[y, x, 3] = 255
            if touched is not None:
                touched[(x, y)] = touched.get((x, y), 0) + 1
    return rgba
