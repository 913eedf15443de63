"""Handmade cases for mpn_track_trails: a few frames of a few persons with ids written by hand. A case is a dict: 'name',
'params' (the keyword arguments of `TrackTrails` that the history reads), 'frames' (per frame a list of `zones_cases.person`s),
'max_boxes' (as small as the case allows) and, for one case, 'total' (the record's total, smaller than the sum of its counts).
Every coordinate is a small integer or a half, exact in f32 and in f64. The persons are zones_cases': both ankles at (x, y), the
box's bottom centre at (x + 4, y + 8)."""
import numpy as np

import trails_ref as ref
import zones_cases
from zones_cases import person

H, W = zones_cases.H, zones_cases.W
ZONES = zones_cases.BY_NAME


def params(**kw):
    return dict(dict(frame_size=(H, W), length=5, every=1, max_gap=30), **kw)


def reference_params(p):
    """The keyword arguments of a TrackTrails -> the reference's Params."""
    anchor = {'feet': ref.FEET, 'box_bottom': ref.BOX_BOTTOM, 'box_centre': ref.BOX_CENTRE}[p.get('anchor', 'feet')]
    return ref.Params(p['frame_size'], p.get('length', 32), p.get('every', 1), p.get('max_gap', 30), anchor,
                      p.get('min_keypoint_score', 0.0))


def case(name, p, frames, max_boxes=None, total=None):
    most = max([len(f) for f in frames] + [1])
    return {'name': name, 'params': p, 'frames': frames, 'max_boxes': max_boxes or most, 'total': total}


def walk(track_id, n, x0=20, y0=30, step=7):
    """n frames of one person walking to the right."""
    return [[person(track_id, x0 + step * i, y0 + (i % 3))] for i in range(n)]


# person 1 is seen in frames 1-3 and 6-10, person 2 in every frame: over the gap person 1 keeps its points
GAP = [[person(1, 20 + 5 * i, 40), person(2, 300 - 5 * i, 90)] if i not in (3, 4) else [person(2, 300 - 5 * i, 90)] for i in range(10)]
# max_gap = 2: person 1 comes back after exactly 2 frames (frame 1 -> 3: no restart), person 2 after 3 (frame 1 -> 4: restart);
# person 3 is seen throughout
GAPS = [[person(1, 20, 40), person(2, 60, 40), person(3, 100, 40)], [person(3, 104, 40)], [person(1, 24, 40), person(3, 108, 40)],
        [person(2, 64, 40), person(1, 28, 40)], [person(2, 68, 40), person(1, 32, 40), person(3, 112, 40)]]
HUGE = np.float32(3e38)


def _overflow():
    """A box whose bottom centre is finite in f64 and not in f32: ((0 + 3e38) * 0.5 * 640): no anchor; then the person again."""
    p = person(1, 30, 30, score=0.1)
    p['box'] = np.array([0, 0, 0.5, HUGE], np.float32)
    return [[person(1, 20, 30, score=0.1)], [p, person(2, 50, 50)], [person(1, 40, 30, score=0.1)]]


CASES = [
    case('length_1', params(length=1), walk(3, 4)),
    case('length_2', params(length=2), walk(3, 6)),                 # wraps its ring of 2 three times
    case('wrap_twice', params(length=5), walk(7, 12) ),             # 12 points through a ring of 5
    case('length_64', params(length=64), walk(1, 6) + [[person(1, 70, 35), person(2, 10, 10)]]),
    case('every_1', params(every=1), GAP),
    case('every_2', params(every=2), GAP),                          # n = count + 1 on the frames between two kept points
    case('every_5', params(every=5, length=2), GAP),
    case('max_gap_2', params(max_gap=2), GAPS),
    case('max_gap_0', params(max_gap=0), GAPS),
    case('max_gap_2_every_2', params(max_gap=2, every=2), GAPS),
    case('duplicate_id', params(), ZONES['duplicate_id']['frames']),
    case('evict_all', params(length=2), ZONES['evict_all']['frames'], max_boxes=64),
    case('evict_stale', params(length=2), ZONES['evict_stale']['frames'], max_boxes=64),
    case('nan_keypoint', params(), ZONES['nan_keypoint']['frames']),
    case('ankles', params(min_keypoint_score=0.5), ZONES['ankles']['frames']),
    case('box_centre', params(anchor='box_centre'), ZONES['box_centre']['frames']),
    case('box_bottom', params(anchor='box_bottom'), ZONES['box_bottom']['frames']),
    case('empty_frame', params(), ZONES['empty_frame']['frames']),
    case('total_clamped', params(), ZONES['total_clamped']['frames'], total=4),
    case('untracked', params(), ZONES['untracked']['frames']),
    case('f32_overflow', params(min_keypoint_score=0.5), _overflow()),
]
BY_NAME = {c['name']: c for c in CASES}

# two cases with the same parameters side by side as the two streams of one call (the shorter one padded with empty frames)
PAIRS = [('evict_all', 'evict_stale'), ('wrap_twice', 'every_1'), ('nan_keypoint', 'untracked'), ('duplicate_id', 'empty_frame')]


def pair(first, second):
    a, b = BY_NAME[first], BY_NAME[second]
    assert a['params'] == b['params'] and a['total'] is None and b['total'] is None
    F = max(len(a['frames']), len(b['frames']))
    frames = a['frames'] + [[]] * (F - len(a['frames'])) + b['frames'] + [[]] * (F - len(b['frames']))
    return case(f'{first}+{second}', a['params'], frames, max(a['max_boxes'], b['max_boxes']))


outputs_of = zones_cases.outputs_of


# ------------------------------------------------------------------------------------------------------------------ the picture
# A setting is what one TrackTrails draws with; under each, images of the three frame sizes: a ragged batch for the kernel.
SIZES = [(1, 1), (5, 7), (33, 67)]
RED_GREEN = ((255, 0, 0), (0, 255, 0), (10, 20, 30))
SETTINGS = [dict(length=5, fade=True, min_alpha=64, palette=None), dict(length=5, fade=False, min_alpha=64, palette=RED_GREEN),
            dict(length=5, fade=True, min_alpha=0, palette=RED_GREEN), dict(length=5, fade=True, min_alpha=255, palette=None),
            dict(length=1, fade=True, min_alpha=64, palette=None), dict(length=2, fade=True, min_alpha=17, palette=RED_GREEN),
            dict(length=64, fade=True, min_alpha=0, palette=None)]


def trails_of(K, persons):
    """[(track_id, tracked, [(x, y), ...] newest first)] -> (track ids, the 'trails' dict of `TrackTrails.unpack`)."""
    n = len(persons)
    points, count = np.zeros((n, K + 1, 2), np.float32), np.zeros(n, np.int32)
    for i, (_, _, pts) in enumerate(persons):
        assert len(pts) <= K + 1
        count[i] = len(pts)
        points[i, :len(pts)] = np.asarray(pts, np.float32).reshape(-1, 2)
    tracked = np.array([bool(t) for _, t, _ in persons], bool).reshape(n)
    ids = np.array([i for i, _, _ in persons], np.int32).reshape(n)
    flags = np.zeros(n, bool)
    return ids, {'points': points, 'count': count, 'tracked': tracked, 'appended': flags, 'restarted': flags,
                 'anchor_from_keypoints': flags}


def _handmade(K, h, w):
    """Trails that cross themselves and each other, negative and fractional coordinates, points far outside the frame,
    zero-length segments, and the rows that are not drawn, cut to K + 1 points."""
    cut = lambda pts: pts[:K + 1]                                   # noqa: E731
    return [(1, True, cut([(w - 2, h - 3), (1.5, 1.25), (w - 2.5, 1.75), (2, h - 2.5), (w / 2, -3.5), (-4.5, h / 2)])),   # an X and more
            (2, True, cut([(w / 2, -0.5), (w / 2, h + 0.5)])),                              # across the first; both ends outside
            (0, False, [(3, 3)]),                                                           # untracked: one point
            (5, True, [(2, 2)]),                                                            # a first observation: no segment
            (3, True, cut([(3, 2), (3, 2), (3.9, 2.9), (-0.9, -0.9), (-0.9, -0.9)])),       # zero-length segments
            (6, False, cut([(0, 0), (w, h)])),                                              # not tracked: not drawn
            (0, True, cut([(0, h), (w, 0)])),                                               # no identity: not drawn
            (14, True, cut([(-5000, -4000), (5000, 4321.5), (w / 3, 1 - h), (2 * w, h / 2)]))]  # far outside


def _seeded(K, h, w, seed):
    rng = np.random.RandomState(seed)
    persons = []
    for i in range(6):
        n = int(rng.randint(0, K + 2))
        pts = np.round(rng.uniform(-0.5, 1.5, (n, 2)) * (w, h) * 4) / 4      # quarters of a pixel, a third of them off the frame
        if n > 2 and i % 2:
            pts[1] = pts[0]                                                  # a zero-length segment
        persons.append((int(rng.randint(1, 40)), bool(rng.rand() < 0.8), [tuple(p) for p in pts]))
    return persons


def draw_images(setting):
    """The images of one setting: per frame size the handmade trails and two seeded sets."""
    K = setting['length']
    out = []
    for k, (h, w) in enumerate(SIZES):
        for which, persons in enumerate([_handmade(K, h, w), _seeded(K, h, w, 10 * k + 1), _seeded(K, h, w, 10 * k + 2)]):
            ids, trails = trails_of(K, persons)
            out.append({'name': f'{h}x{w}#{which}', 'h': h, 'w': w, 'track_ids': ids, 'trails': trails})
    return out


def background(h, w, seed=0):
    """A seeded RGBA frame with alpha 255, as mpn_draw_detections leaves it."""
    rgba = np.random.RandomState(seed).randint(0, 256, (h, w, 4)).astype(np.uint8)
    rgba[..., 3] = 255
    return rgba


def palette_of(setting):
    from multiposenet_amd.inference.draw import DEFAULT_PALETTE
    return setting['palette'] if setting['palette'] is not None else DEFAULT_PALETTE
