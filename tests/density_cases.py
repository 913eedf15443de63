"""Handmade cases for mpn_density_map and mpn_draw_density: a few frames of a few persons with ids written by hand, on frames of
48 x 80 pixels. A case is a dict: 'name', 'params' (the keyword arguments of `DensityMap` that the map reads), 'frames' (per frame
a list of `person`s), 'max_boxes' (as small as the case allows), 'tracked' (False: the launch without track rows), 'preload'
({(plane, row, col): count} written into the empty state first) and, for one case, 'total' (the record's total, smaller than the
sum of its counts). Every coordinate is a small integer, exact in f32 and in f64. cell = 8 gives a grid of 6 x 10, cell = 7 one of
7 x 12 whose last row and column are ragged."""
import numpy as np

import density_ref as ref

H, W = 48, 80
FULL = ref.SATURATED


def person(track_id, x, y, score=0.9, left=None, right=None, box=None):
    """A person whose ankles are both at (x, y) unless given as (x, y, score). box: (x0, y0, x1, y1) in pixels; else 8 wide and
    14 high, ending 2 pixels below the ankles around x + 1: its bottom centre is (x + 1, y + 2), its centre (x + 1, y - 5). The
    box is stored normalised in f32: its edges in pixels are what the f64 products give, never on a cell's centre here."""
    kp = np.zeros((17, 3), np.float32)
    kp[:, 0], kp[:, 1], kp[:, 2] = x, y - 6, 0.9
    kp[15] = left if left is not None else (x, y, score)
    kp[16] = right if right is not None else (x, y, score)
    x0, y0, x1, y1 = box if box is not None else (x - 3, y - 12, x + 5, y + 2)
    return {'track_id': track_id, 'box': np.array([y0 / H, x0 / W, y1 / H, x1 / W], np.float32), 'keypoints': kp,
            'score': np.float32(0.8)}


def outputs_of(frames, keypoints=True, track_ids=True):
    """Frames of persons -> the dicts a Detector returns."""
    out = []
    for persons in frames:
        n = len(persons)
        d = {'boxes': np.array([p['box'] for p in persons], np.float32).reshape(n, 4),
             'scores': np.array([p['score'] for p in persons], np.float32).reshape(n)}
        if track_ids:
            d['track_ids'] = np.array([p['track_id'] for p in persons], np.int32).reshape(n)
        if keypoints:
            d['keypoints'] = np.array([p['keypoints'] for p in persons], np.float32).reshape(n, 17, 3)
        out.append(d)
    return out


def params(**kw):
    return dict(dict(frame_size=(H, W), cell=8), **kw)


def reference_params(p):
    """The keyword arguments of a DensityMap -> the reference's Params."""
    anchor = {'feet': ref.FEET, 'box_bottom': ref.BOX_BOTTOM, 'box_centre': ref.BOX_CENTRE}[p.get('anchor', 'feet')]
    return ref.Params(p['frame_size'], p.get('cell', 16), {'anchor': ref.ANCHOR, 'box': ref.BOX}[p.get('footprint', 'anchor')], anchor,
                      p.get('min_keypoint_score', 0.0), p.get('half_life', 0), {'dwell': ref.DWELL, 'visits': ref.VISITS}[p.get('show', 'dwell')])


def case(name, p, frames, max_boxes=None, total=None, tracked=True, preload=None):
    most = max([len(f) for f in frames] + [1])
    return {'name': name, 'params': p, 'frames': frames, 'max_boxes': max_boxes or most, 'total': total, 'tracked': tracked,
            'preload': preload or {}}


def preloaded(c, streams=1):
    """The case's start state: empty but for its preload, in every stream."""
    p = reference_params(c['params'])
    state = ref.new_state(streams, p)
    for (plane, r, col), value in c['preload'].items():
        state[plane][:, r, col] = value
    return state


STAY = [[person(1, 20, 20)]] * 4                                    # cell (2, 2) in every frame
# frame 2 stays in cell (2, 2): no visit; frame 3 is cell (2, 3): a visit; frame 4 is back: a visit
WANDER = [[person(1, 20, 20)], [person(1, 23, 23)], [person(1, 30, 20)], [person(1, 20, 20)]]
# frame 2 stands left of the frame: OUTSIDE, the slot forgets its cell; frame 3 is the old cell: a visit; frame 4 is not
LEAVE = [[person(1, 20, 20)], [person(1, -5, 20)], [person(1, 20, 20)], [person(1, 20, 20)]]
NAN = float('nan')

CASES = [
    # dwell of (2, 2): 1; halved to 0, + 1 = 1; 2; halved to 1, + 1 = 2. visits: 1; halved to 0 and no visit; 0; 0
    case('halving', params(half_life=2), STAY),
    case('halving_visits_shown', params(half_life=3, show='visits'), WANDER),
    # (2, 2) is full in both planes: the add saturates. With half_life = 3, frame 3 halves to 2^31 - 1 and adds: 2^31
    case('saturate', params(), STAY[:3], preload={('dwell', 2, 2): FULL, ('visits', 2, 2): FULL, ('dwell', 0, 0): 7}),
    case('saturate_then_halve', params(half_life=3), STAY[:3], preload={('dwell', 2, 2): FULL, ('visits', 2, 2): FULL}),
    case('wander', params(), WANDER),
    case('leave_and_reenter', params(), LEAVE),
    # two rows with id 1: the second is untracked - it dwells, it does not visit
    case('duplicate_id', params(), [[person(1, 20, 20), person(1, 50, 30)], [person(1, 50, 30), person(1, 20, 20)], [person(1, 20, 20)]]),
    # 64 ids fill the slots; the 65th takes slot 0 (every `last` is 1: the lowest index), which was id 1's; id 1 is new in frame 3
    # and visits the cell it never left, taking the stalest slot, id 2's
    case('evict', params(), [[person(1 + i, 4 + 8 * (i % 10), 4 + 8 * (i // 10 % 6)) for i in range(64)], [person(65, 20, 20)],
                             [person(1, 4, 4), person(2, 12, 4)]], max_boxes=64),
    # a NaN ankle with a passing score: no anchor; ids 0 and -1: untracked
    case('no_anchor', params(), [[person(1, 20, 20), person(2, 60, 40)], [person(1, 0, 0, left=(NAN, 20, 0.9), right=(20, 20, 0.9)),
                                                                            person(2, 60, 40)],
                                 [person(0, 20, 20), person(-1, 60, 40), person(1, 20, 20)]]),
    case('ankles', params(min_keypoint_score=0.5),
         [[person(1, 0, 0, left=(70, 40, 0.2), right=(30, 30, 0.6)), person(2, 60, 30, score=0.4),
           person(3, 0, 0, left=(20, 30, 0.5), right=(40, 34, 0.9))]] * 3),
    case('box_centre', params(anchor='box_centre'), [[person(1, 30, 20), person(2, 30, 40)]] * 3),
    case('box_bottom', params(anchor='box_bottom'), [[person(1, 30, 20), person(2, 30, 46)]] * 3),     # (31, 48): OUTSIDE, below the frame
    case('empty_frame', params(), [[person(1, 20, 20)], [], [person(1, 30, 20)], []]),
    case('total_clamped', params(), [[person(1, 20, 20), person(2, 60, 40), person(3, 30, 20)],
                                     [person(1, 30, 20), person(2, 20, 20), person(3, 20, 20)], []], total=4),
    case('untracked_launch', params(), WANDER, tracked=False),
    # the box of (78, 46) spans x 75..83, y 34..48: the centres x = 76, y = 36 and 44: two cells, the rest of it past the frame.
    # The box x 5..11, y 5..11 covers no centre (4, 12). A box over everything: 60 cells. A box with x1 = inf: nothing.
    case('box_footprint', params(footprint='box'),
         [[person(1, 78, 46), person(2, 8, 8, box=(5, 5, 11, 11)), person(3, 40, 24, box=(-10, -10, 200, 100))],
          [person(1, 20, 20), person(4, 40, 24, box=(10, 10, float('inf'), 30))], [person(1, 20, 20, box=(16, 2, 30, 21))]]),
    case('box_footprint_halving', params(footprint='box', half_life=2, anchor='box_centre'),
         [[person(1, 20, 20), person(2, 24, 22)], [person(1, 28, 20)], [], [person(2, 24, 30)]]),
    # cell = 7: 7 x 12 cells, the last row holds y = 42..47, the last column x = 77..79
    case('ragged', params(cell=7), [[person(1, 79, 47), person(2, 76, 41)], [person(1, 77, 42)], [person(2, 0, 0), person(1, 6, 7)]]),
    case('ragged_box', params(cell=7, footprint='box'), [[person(1, 79, 47), person(2, 40, 20, box=(60, 30, 90, 60))], [person(1, 77, 42)],
                                                         [person(2, 3, 3, box=(0, 0, 4, 4))]]),
]
BY_NAME = {c['name']: c for c in CASES}

# two cases with the same parameters side by side as the two streams of one call (the shorter one padded with empty frames)
PAIRS = [('wander', 'leave_and_reenter'), ('evict', 'no_anchor'), ('duplicate_id', 'empty_frame'), ('saturate', 'wander')]


def pair(first, second):
    a, b = BY_NAME[first], BY_NAME[second]
    assert a['params'] == b['params'] and a['total'] is None and b['total'] is None and a['tracked'] and b['tracked']
    F = max(len(a['frames']), len(b['frames']))
    frames = a['frames'] + [[]] * (F - len(a['frames'])) + b['frames'] + [[]] * (F - len(b['frames']))
    return case(f'{first}+{second}', a['params'], frames, max(a['max_boxes'], b['max_boxes']), preload=a['preload'])


def pair_state(first, second):
    """The start state of `pair`: stream 0 has the first case's preload, stream 1 the second's."""
    state = preloaded(BY_NAME[first], 2)
    state[1] = preloaded(BY_NAME[second], 1)[0]
    return state


# ------------------------------------------------------------------------------------------------------------------ the picture
# A setting is what one DensityMap draws with. Under each, three grids for frames of the setting's size: a ragged batch is not
# possible here (every frame of a call has one size), so the three images differ in their counts alone.
RAINBOW = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], axis=1).astype(np.uint8)
SETTINGS = [dict(size=(48, 80), cell=4, smooth=True, full_scale=0, opacity=160, colormap=None),
            dict(size=(48, 80), cell=4, smooth=False, full_scale=0, opacity=255, colormap=RAINBOW),
            dict(size=(48, 80), cell=7, smooth=True, full_scale=40, opacity=200, colormap=RAINBOW),
            dict(size=(48, 80), cell=7, smooth=False, full_scale=1000, opacity=160, colormap=None),
            dict(size=(33, 67), cell=7, smooth=True, full_scale=0, opacity=97, colormap=None),
            dict(size=(48, 300), cell=256, smooth=True, full_scale=0, opacity=160, colormap=None),     # two cells side by side
            dict(size=(48, 300), cell=256, smooth=False, full_scale=90, opacity=31, colormap=RAINBOW),
            dict(size=(9, 300), cell=256, smooth=True, full_scale=0, opacity=255, colormap=RAINBOW)]
# one cell over the whole frame: every pixel has the cell's level, so an image is blended everywhere or nowhere - the one shape
# that cannot do both in one image, kept out of SETTINGS for that reason
ONE_CELL = [dict(size=(48, 80), cell=256, smooth=True, full_scale=0, opacity=160, colormap=None),
            dict(size=(48, 80), cell=256, smooth=False, full_scale=90, opacity=31, colormap=RAINBOW)]


def colormap_of(setting):
    from multiposenet_amd.inference.maps import colour_table
    return setting['colormap'] if setting['colormap'] is not None else colour_table()[:, :3]


def draw_grids(setting):
    """[(name, grid uint32 [gh, gw], max)] of one setting: a handmade grid (a blob, a full cell next to empty ones, a count
    beyond every full_scale), a seeded sparse one, and an empty one, which must leave its frame alone."""
    gh, gw = ref.grid_of(setting['size'], setting['cell'])
    hand = np.zeros((gh, gw), np.uint32)
    hand[0, 0] = 5000
    hand[gh // 2, gw // 2] = 60
    hand[gh // 2, max(gw // 2 - 1, 0)] = max(int(hand[gh // 2, max(gw // 2 - 1, 0)]), 30)
    hand[gh - 1, gw - 1] = max(int(hand[gh - 1, gw - 1]), 1)
    rng = np.random.RandomState(gh * 100 + gw)
    seeded = (rng.randint(0, 50, (gh, gw)) * (rng.rand(gh, gw) < 0.3)).astype(np.uint32)
    seeded[rng.randint(gh), rng.randint(gw)] = 49
    if gh * gw == 2:                                                # two cells: the left one empty, so that the pixels left of its
        hand[0, 0], hand[0, 1] = 0, 60                              # centre keep their bytes with and without smooth
        seeded[0, 0], seeded[0, 1] = 0, 37
    return [('hand', hand, int(hand.max())), ('seeded', seeded, int(seeded.max())), ('empty', np.zeros((gh, gw), np.uint32), 0)]


def background(h, w, seed=0):
    """A seeded RGBA frame with alpha 255, as mpn_draw_detections leaves it."""
    rgba = np.random.RandomState(seed).randint(0, 256, (h, w, 4)).astype(np.uint8)
    rgba[..., 3] = 255
    return rgba
