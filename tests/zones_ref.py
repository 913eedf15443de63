"""The definition of mpn_zone_events (include/mpn.h) as plain Python loops: f64 arithmetic through numpy scalars, one operation
at a time in the order the header writes them, and integers for the state. Produces the person rows, the image rows and the
state bytes the kernel must equal byte for byte. Written from the header, not from the kernel."""
import numpy as np

MAX_ZONES = MAX_LINES = MAX_VERTICES = 16
SLOTS = 64
LEFT_ANKLE, RIGHT_ANKLE = 15, 16
FLAG_TRACKED, FLAG_ANKLES, FLAG_NO_ANCHOR = 1, 2, 4
FEET, BOX_BOTTOM, BOX_CENTRE = 0, 1, 2

SLOT = np.dtype([('id', np.int32), ('inside', np.uint32), ('last', np.int32), ('pad', np.int32), ('anchor', np.float64, (2,)),
                 ('entered_frame', np.int32, (16,)), ('run', np.uint8, (16,))])
STATE = np.dtype([('frames', np.int32), ('pad', np.int32, (3,)), ('zone_entries', np.uint32, (16,)), ('zone_exits', np.uint32, (16,)),
                  ('line_positive', np.uint32, (16,)), ('line_negative', np.uint32, (16,)), ('slots', SLOT, (SLOTS,))])
PERSON = np.dtype([('inside', np.uint32), ('entered', np.uint32), ('exited', np.uint32), ('crossed_positive', np.uint32),
                   ('crossed_negative', np.uint32), ('flags', np.uint32), ('anchor', np.float64, (2,)), ('dwell', np.int32, (16,))])
IMAGE = np.dtype([(k, np.uint32, (16,)) for k in ('occupancy', 'entries', 'exits', 'positive', 'negative', 'total_entries',
                                                  'total_exits', 'total_positive', 'total_negative')])
assert (SLOT.itemsize, STATE.itemsize, PERSON.itemsize, IMAGE.itemsize) == (112, 7440, 104, 576)

f64 = np.float64


class Geometry:
    """What the table says, as plain Python values: zones as lists of (x, y), lines as ((Px, Py), (Qx, Qy))."""

    def __init__(self, frame_size, zones=(), lines=(), anchor=FEET, min_frames=1, min_keypoint_score=0.0):
        self.height, self.width = f64(frame_size[0]), f64(frame_size[1])
        self.zones = [[(f64(x), f64(y)) for x, y in polygon] for polygon in zones]
        self.lines = [((f64(p[0]), f64(p[1])), (f64(q[0]), f64(q[1]))) for p, q in lines]
        self.anchor, self.min_frames, self.min_keypoint_score = int(anchor), int(min_frames), f64(min_keypoint_score)


def new_state(streams):
    return np.zeros(streams, STATE)


def pack_state(state):
    return state.tobytes()


def anchor_of(geo, box, keypoints):
    """(x, y, from_ankles) of one person, or None when a coordinate is not finite. box: (ymin, xmin, ymax, xmax) f32,
    normalised; keypoints: f32 [17, 3] (x, y, score) in pixels, or None."""
    ymin, xmin, ymax, xmax = (f64(v) for v in box)
    passing = []
    if geo.anchor == FEET and keypoints is not None:
        for k in (LEFT_ANKLE, RIGHT_ANKLE):
            if f64(keypoints[k][2]) >= geo.min_keypoint_score:      # (a NaN never passes)
                passing.append((f64(keypoints[k][0]), f64(keypoints[k][1])))
    with np.errstate(all='ignore'):
        if len(passing) == 2:
            x, y = (passing[0][0] + passing[1][0]) * f64(0.5), (passing[0][1] + passing[1][1]) * f64(0.5)
        elif len(passing) == 1:
            x, y = passing[0]
        else:
            x = (xmin + xmax) * f64(0.5) * geo.width
            y = (ymin + ymax) * f64(0.5) * geo.height if geo.anchor == BOX_CENTRE else ymax * geo.height
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    return x, y, bool(passing)


def inside(polygon, ax, ay):
    """The crossing number of the header, without a division."""
    crossed = 0
    x1, y1 = polygon[-1]
    for x2, y2 in polygon:
        if (y1 > ay) != (y2 > ay):
            with np.errstate(all='ignore'):
                t = (x2 - x1) * (ay - y1) - (ax - x1) * (y2 - y1)
            crossed += bool(t > 0) if y2 > y1 else bool(t < 0)
        x1, y1 = x2, y2
    return crossed % 2 == 1


def crossing(line, a, c):
    """0 = not crossed, +1 = positive, -1 = negative: line (P, Q), movement a -> c."""
    (px, py), (qx, qy) = line
    (ax, ay), (cx, cy) = a, c
    with np.errstate(all='ignore'):
        da = (qx - px) * (ay - py) - (qy - py) * (ax - px)
        dc = (qx - px) * (cy - py) - (qy - py) * (cx - px)
        ep = (cx - ax) * (py - ay) - (cy - ay) * (px - ax)
        eq = (cx - ax) * (qy - ay) - (cy - ay) * (qx - ax)
    if (da > 0) != (dc > 0) and (ep > 0) != (eq > 0):
        return 1 if dc > 0 else -1
    return 0


def run(geo, outputs, state, max_boxes, total=None):
    """outputs: b = streams * F dicts with 'boxes' f32 [n, 4], 'track_ids' int [n] and, optionally, 'keypoints' f32 [n, 17, 3];
    state: `new_state(streams)`, advanced in place. total: the record's total where it is smaller than the sum of the counts
    (rows behind it do not exist). -> (person rows PERSON [b * max_boxes], image rows IMAGE [b])."""
    b, streams = len(outputs), len(state)
    assert b % streams == 0
    F = b // streams
    persons, images = np.zeros(b * max_boxes, PERSON), np.zeros(b, IMAGE)
    counts = [len(o['boxes']) for o in outputs]
    if total is None:
        total = sum(counts)
    total = max(0, min(total, b * max_boxes))
    Z, L = len(geo.zones), len(geo.lines)
    for s in range(streams):
        st = state[s]
        slots = st['slots']
        for j in range(F):
            i = s * F + j
            now = int(st['frames']) + j + 1
            first = min(sum(counts[:i]), total)
            n = min(counts[i], max_boxes, total - first)
            o = outputs[i]
            anchors = [anchor_of(geo, o['boxes'][r], o['keypoints'][r] if 'keypoints' in o else None) for r in range(n)]
            ids = [int(o['track_ids'][r]) for r in range(n)]
            raw = [0] * n
            for r in range(n):
                if anchors[r] is not None:
                    for z in range(Z):
                        raw[r] |= int(inside(geo.zones[z], anchors[r][0], anchors[r][1])) << z
            # 1. the slots, serially in row order
            taken, slot_of, fresh = set(), [None] * n, [False] * n
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
                    fresh[r] = True
                taken.add(k)
                slot_of[r] = k
            for r in range(n):
                row = persons[first + r]
                if anchors[r] is None:
                    row['flags'] = FLAG_NO_ANCHOR
                    continue
                cx, cy, from_ankles = anchors[r]
                row['anchor'] = (cx, cy)
                row['flags'] = FLAG_ANKLES if from_ankles else 0
                if slot_of[r] is None:                              # 5. untracked
                    row['inside'] = raw[r]
                    continue
                row['flags'] |= FLAG_TRACKED
                slot = slots[slot_of[r]]
                confirmed = int(slot['inside'])
                for z in range(Z):                                  # 2. zones
                    bit = 1 << z
                    if (raw[r] & bit) == (confirmed & bit):
                        slot['run'][z] = 0
                    elif int(slot['run'][z]) + 1 >= geo.min_frames:
                        confirmed ^= bit
                        slot['run'][z] = 0
                        if confirmed & bit:
                            row['entered'] |= bit
                            slot['entered_frame'][z] = now
                        else:
                            row['exited'] |= bit
                            slot['entered_frame'][z] = 0
                    else:
                        slot['run'][z] += 1
                    row['dwell'][z] = now - int(slot['entered_frame'][z]) + 1 if confirmed & bit else 0
                if int(slot['last']) != 0:                          # 3. lines
                    a = (f64(slot['anchor'][0]), f64(slot['anchor'][1]))
                    for l in range(L):
                        way = crossing(geo.lines[l], a, (cx, cy))
                        if way > 0:
                            row['crossed_positive'] |= 1 << l
                        elif way < 0:
                            row['crossed_negative'] |= 1 << l
                slot['inside'], slot['last'], slot['anchor'] = confirmed, now, (cx, cy)     # 4.
                row['inside'] = confirmed
            im = images[i]
            for r in range(n):
                row = persons[first + r]
                for q in range(16):
                    im['occupancy'][q] += (int(row['inside']) >> q) & 1
                    im['entries'][q] += (int(row['entered']) >> q) & 1
                    im['exits'][q] += (int(row['exited']) >> q) & 1
                    im['positive'][q] += (int(row['crossed_positive']) >> q) & 1
                    im['negative'][q] += (int(row['crossed_negative']) >> q) & 1
            st['zone_entries'] += im['entries']
            st['zone_exits'] += im['exits']
            st['line_positive'] += im['positive']
            st['line_negative'] += im['negative']
            im['total_entries'], im['total_exits'] = st['zone_entries'], st['zone_exits']
            im['total_positive'], im['total_negative'] = st['line_positive'], st['line_negative']
        st['frames'] += F
    return persons, images


def unpacked(geo, persons, images, counts, max_boxes):
    """The rows of `run` as the dicts `ZoneCounter.unpack` gives (for whole records: total = the sum of the counts)."""
    Z, L = len(geo.zones), len(geo.lines)
    res, s = [], 0
    for i, n in enumerate(counts):
        r, im = persons[s:s + n], images[i]
        bits = lambda field, m: np.array([[(int(v) >> q) & 1 for q in range(m)] for v in r[field]], bool).reshape(n, m)
        res.append({'inside': bits('inside', Z), 'entered': bits('entered', Z), 'exited': bits('exited', Z),
                    'crossed_positive': bits('crossed_positive', L), 'crossed_negative': bits('crossed_negative', L),
                    'anchor': r['anchor'].copy(), 'anchor_from_keypoints': (r['flags'] & FLAG_ANKLES) != 0,
                    'dwell_frames': r['dwell'][:, :Z].copy(),
                    'occupancy': im['occupancy'][:Z].copy(), 'entries': im['entries'][:Z].copy(), 'exits': im['exits'][:Z].copy(),
                    'total_entries': im['total_entries'][:Z].copy(), 'total_exits': im['total_exits'][:Z].copy(),
                    'line_positive': im['positive'][:L].copy(), 'line_negative': im['negative'][:L].copy(),
                    'total_line_positive': im['total_positive'][:L].copy(),
                    'total_line_negative': im['total_negative'][:L].copy()})
        s += n
    return res
