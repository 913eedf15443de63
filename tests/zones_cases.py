"""Handmade cases for mpn_zone_events: a few frames of a few persons with ids written by hand. A case is a dict: 'name', 'geo'
(the keyword arguments of `ZoneCounter` / `zones_ref.Geometry`), 'frames' (per frame a list of persons), 'max_boxes' (as small as
the case allows) and, for one case, 'total' (the record's total, smaller than the sum of its counts). Every coordinate is a small
integer or a half, exact in f32 and in f64; where a case says what must come out, the arithmetic is in its comment."""
import numpy as np

import zones_ref as ref

H, W = 480, 640
SQUARE = [(10, 10), (50, 10), (50, 50), (10, 50)]
TRIANGLE = [(100, 100), (140, 100), (100, 140)]                      # its sloped edge: x + y = 240
CONCAVE = [(200, 0), (300, 0), (300, 100), (260, 100), (260, 40), (240, 40), (240, 100), (200, 100)]     # a U open at the bottom
GATE = ((400, 0), (400, 100))                                       # d(X) = -100 * (Xx - 400): positive to the LEFT of x = 400
STANDARD = dict(frame_size=(H, W), zones={'square': SQUARE, 'triangle': TRIANGLE, 'concave': CONCAVE}, lines={'gate': GATE})


def person(track_id, x, y, score=0.9, left=None, right=None):
    """A person whose ankles are both at (x, y) unless given as (x, y, score), and whose box ends 8 pixels below them, 20 pixels
    wide around x + 4: the box's bottom centre is (x + 4, y + 8), so that the fallback shows."""
    kp = np.zeros((17, 3), np.float32)
    kp[:, 0], kp[:, 1], kp[:, 2] = x, y - 20, 0.9
    kp[15] = left if left is not None else (x, y, score)
    kp[16] = right if right is not None else (x, y, score)
    box = np.array([(y - 40) / H, (x - 6) / W, (y + 8) / H, (x + 14) / W], np.float32)
    return {'track_id': track_id, 'box': box, 'keypoints': kp, 'score': np.float32(0.8)}


def outputs_of(frames, keypoints=True):
    """Frames of persons -> the dicts a tracker's host side returns."""
    out = []
    for persons in frames:
        n = len(persons)
        d = {'boxes': np.array([p['box'] for p in persons], np.float32).reshape(n, 4),
             'scores': np.array([p['score'] for p in persons], np.float32).reshape(n),
             'track_ids': np.array([p['track_id'] for p in persons], np.int32).reshape(n)}
        if keypoints:
            d['keypoints'] = np.array([p['keypoints'] for p in persons], np.float32).reshape(n, 17, 3)
        out.append(d)
    return out


def geometry(geo):
    """The keyword arguments of a ZoneCounter -> the reference's Geometry."""
    zones, lines = geo.get('zones') or {}, geo.get('lines') or {}
    zones = list(zones.values()) if isinstance(zones, dict) else list(zones)
    lines = list(lines.values()) if isinstance(lines, dict) else list(lines)
    anchor = {'feet': ref.FEET, 'box_bottom': ref.BOX_BOTTOM, 'box_centre': ref.BOX_CENTRE}[geo.get('anchor', 'feet')]
    return ref.Geometry(geo['frame_size'], zones, lines, anchor, geo.get('min_frames', 1), geo.get('min_keypoint_score', 0.0))


def case(name, geo, frames, max_boxes=None, total=None):
    most = max([len(f) for f in frames] + [1])
    return {'name': name, 'geo': geo, 'frames': frames, 'max_boxes': max_boxes or most, 'total': total}


def _circle(cx, cy, radius, n=16):
    """n vertices on a circle, rounded to quarters of a pixel: exact in f64 whatever libm says."""
    a = 2 * np.pi * np.arange(n) / n
    return [(float(np.round((cx + radius * np.cos(t)) * 4) / 4), float(np.round((cy + radius * np.sin(t)) * 4) / 4)) for t in a]


def _full():
    rng = np.random.RandomState(7)
    zones = {f'z{i}': _circle(80 + 150 * (i % 4), 60 + 110 * (i // 4), 40 + 5 * i) for i in range(16)}
    lines = {f'l{i}': ((20 + 38 * i, 0), (60 + 30 * i, 479)) if i % 2 == 0 else ((0, 20 + 28 * i), (639, 50 + 22 * i)) for i in range(16)}
    frames = []
    for _ in range(4):
        frames.append([person(i + 1, int(rng.randint(0, W)), int(rng.randint(0, H))) for i in range(12)] +
                      [person(0, int(rng.randint(0, W)), int(rng.randint(0, H)))])
    return case('full', dict(frame_size=(H, W), zones=zones, lines=lines, min_frames=2), frames)


FLICKER = [[person(1, *p)] for p in [(30, 30), (30, 30), (30, 30), (60, 30), (30, 30), (60, 30), (60, 30), (60, 30)]]

CASES = [
    # (250, 70) lies in the notch of the U: outside; the others are inside. In frame 2 the persons change places.
    case('concave', STANDARD, [[person(1, 250, 70), person(2, 220, 70), person(3, 280, 70), person(4, 250, 20)],
                               [person(1, 220, 70), person(2, 250, 70), person(3, 250, 20), person(4, 280, 70)]]),
    # the crossing rule decides: of the square the sides x = 10 and y = 10 belong to it, x = 50 and y = 50 do not
    case('boundary', STANDARD, [[person(1, 10, 10), person(2, 50, 50), person(3, 30, 10), person(4, 30, 50), person(5, 120, 120),
                                 person(6, 0, 10), person(7, 60, 50), person(8, 10, 30), person(9, 50, 30), person(10, 100, 120),
                                 person(11, 100, 100), person(12, 140, 100), person(13, 100, 140), person(14, 119.5, 120)],
                                [person(1, 10, 10)]]),
    # ends on the line: d(C) = 0 is not > 0, d(A) > 0: crossed, negative. The next step starts on it: d(A) = 0 and d(C) < 0: not
    # crossed. Once, not twice.
    case('line_end_on', STANDARD, [[person(1, 390, 50)], [person(1, 400, 50)], [person(1, 410, 50)]]),
    # through Q = (400, 100): e(Q) = 0 and e(P) < 0: not crossed; through P = (400, 0): e(P) = 0 and e(Q) > 0: crossed
    case('line_endpoint', STANDARD, [[person(1, 390, 100), person(2, 390, 0)], [person(1, 410, 100), person(2, 410, 0)]]),
    case('line_parallel', STANDARD, [[person(1, 400, 20), person(2, 390, 20)], [person(1, 400, 80), person(2, 390, 80)]]),
    # frames 2 and 3 do not see person 1: the crossing is found in frame 4, against the anchor of frame 1
    case('line_gap', STANDARD, [[person(1, 410, 50), person(2, 30, 30)], [person(2, 30, 30)], [], [person(1, 390, 50)]]),
    case('flicker_1', dict(STANDARD, min_frames=1), FLICKER),
    case('flicker_2', dict(STANDARD, min_frames=2), FLICKER),
    case('flicker_3', dict(STANDARD, min_frames=3), FLICKER),
    # person 1: the left ankle fails, the right one at (30, 30) is the anchor; person 2: both fail, the box's bottom centre
    # (64, 58) is; person 3: both pass, their mean (30, 40)
    case('ankles', dict(STANDARD, min_keypoint_score=0.5),
         [[person(1, 0, 0, left=(300, 300, 0.2), right=(30, 30, 0.6)), person(2, 60, 50, score=0.4),
           person(3, 0, 0, left=(20, 30, 0.5), right=(40, 50, 0.9))]] * 2),
    # a NaN keypoint with a passing score: no anchor, and no state is touched: frame 3 finds the crossing against frame 1
    case('nan_keypoint', STANDARD, [[person(1, 390, 50), person(2, 30, 30)],
                                    [person(1, 0, 0, left=(np.nan, 50, 0.9), right=(410, 50, 0.9)), person(2, 30, 30)],
                                    [person(1, 410, 50), person(2, 30, 30)], [person(1, 390, 50)]]),
    # the tracker gives the person a new id: a second entry, no exit of the first
    case('id_change', STANDARD, [[person(1, 30, 30)], [person(1, 30, 30)], [person(2, 30, 30)], [person(2, 30, 30)]]),
    case('untracked', STANDARD, [[person(0, 30, 30), person(-1, 120, 110), person(5, 30, 30)]] * 2),
    case('empty_frame', STANDARD, [[person(1, 30, 30)], [], [person(1, 60, 30)], []]),
    # two rows with one id in a frame: the second is handled as untracked
    case('duplicate_id', STANDARD, [[person(1, 30, 30), person(1, 120, 110)], [person(1, 120, 110), person(1, 30, 30)]]),
    # every slot is evicted: 64 ids, 64 other ids, then some of the first again (new identities), then nothing
    case('evict_all', STANDARD, [[person(1 + i, 30 + (i % 2) * 30, 30) for i in range(64)],
                                 [person(101 + i, 30, 30) for i in range(64)],
                                 [person(1 + i, 30, 30) for i in range(0, 64, 7)], []], max_boxes=64),
    # ids 1..20 in frame 1; 21..40 and 1..5 again in frame 2; 30 new ids in frame 3 take the 24 unused slots and then the
    # stalest, the slots of ids 6..11; frame 4: 12 is known (it leaves the square), 6 is new again and takes the stalest slot
    # left, that of 13, so that 13, which comes behind it in the frame, is new as well; 1 is known and enters again
    case('evict_stale', STANDARD, [[person(1 + i, 30, 30) for i in range(20)],
                                   [person(21 + i, 30, 30) for i in range(20)] + [person(1 + i, 60, 30) for i in range(5)],
                                   [person(201 + i, 30, 30) for i in range(30)],
                                   [person(12, 60, 30), person(6, 60, 30), person(13, 60, 30), person(1, 30, 30),
                                    person(231, 30, 30)]], max_boxes=64),
    # the record's total says 4 rows, its counts 3 + 3: the second frame has one row
    case('total_clamped', STANDARD, [[person(1, 30, 30), person(2, 120, 110), person(3, 60, 30)],
                                     [person(1, 60, 30), person(2, 30, 30), person(3, 30, 30)]], total=4),
    case('box_centre', dict(STANDARD, anchor='box_centre'), [[person(1, 30, 40), person(2, 30, 80)]] * 2),
    case('box_bottom', dict(STANDARD, anchor='box_bottom'), [[person(1, 30, 40), person(2, 30, 80)]] * 2),
    _full(),
]
BY_NAME = {c['name']: c for c in CASES}

# two cases with one geometry side by side as the two streams of one call (the shorter one padded with empty frames)
PAIRS = [('evict_all', 'evict_stale'), ('concave', 'boundary'), ('line_gap', 'id_change'), ('nan_keypoint', 'untracked')]


def pair(first, second):
    a, b = BY_NAME[first], BY_NAME[second]
    assert a['geo'] == b['geo'] and a['total'] is None and b['total'] is None
    F = max(len(a['frames']), len(b['frames']))
    frames = a['frames'] + [[]] * (F - len(a['frames'])) + b['frames'] + [[]] * (F - len(b['frames']))
    return case(f'{first}+{second}', a['geo'], frames, max(a['max_boxes'], b['max_boxes']))
