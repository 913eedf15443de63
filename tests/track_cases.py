"""Hand-built sequences for mpn_pose_track: 12 frames each, max_boxes 8, max_tracks 8 or 4. A person is a fixed 17-point
skeleton of a given height around a centre that moves at constant velocity; every frame adds a seeded jitter of at most half a
pixel to each keypoint, so that no OKS is exactly 1. Boxes are normalised (ymin, xmin, ymax, xmax) on a 640 x 480 image,
keypoints are (x, y, score) in its pixels - what `Detector.predict_batch` returns.

The scenarios: persons drifting; two persons crossing; a person absent for exactly max_misses frames (keeps the id) and for
one frame more (a new id); a late entrant, an empty frame and a detection below new_track_score; more persons than slots, one
of whom leaves so that a slot is freed and reused in the same frame; two byte-identical detections in one frame."""
import numpy as np

import track_ref as ref

WIDTH, HEIGHT = 640, 480
FRAMES = 12
MAX_BOXES = 8
MAX_MISSES = 2
MATCH_THRESHOLD = 0.3
NEW_TRACK_SCORE = 0.3
SEED = 20

# the skeleton, relative to the person's centre: x in units of the width (half the height), y in units of the height
_X = np.array([0, .1, -.1, .2, -.2, .3, -.3, .4, -.4, .35, -.35, .2, -.2, .25, -.25, .2, -.2])
_Y = np.array([-.45, -.48, -.48, -.45, -.45, -.3, -.3, -.1, -.1, .05, .05, 0, 0, .25, .25, .48, .48])


def person(cx, cy, height, score, rng):
    """(box f32 [4], score f32, keypoints f32 [17,3]) of one detection."""
    w = 0.5 * height
    kp = np.zeros((17, 3), np.float32)
    kp[:, 0] = cx + _X * w + rng.uniform(-0.5, 0.5, 17)
    kp[:, 1] = cy + _Y * height + rng.uniform(-0.5, 0.5, 17)
    kp[:, 2] = 0.5 + 0.02 * np.arange(17)
    box = np.array([(cy - height / 2) / HEIGHT, (cx - w / 2) / WIDTH, (cy + height / 2) / HEIGHT, (cx + w / 2) / WIDTH], np.float32)
    return box, np.float32(score), kp


def _frame(dets):
    n = len(dets)
    return {'boxes': np.array([d[0] for d in dets], np.float32).reshape(n, 4),
            'scores': np.array([d[1] for d in dets], np.float32).reshape(n),
            'keypoints': np.array([d[2] for d in dets], np.float32).reshape(n, 17, 3)}


def _sequence(script, rng):
    """script(f) -> a list of (cx, cy, height, score) or ('copy', i): detection i of the frame once more, byte for byte."""
    frames = []
    for f in range(FRAMES):
        dets = []
        for item in script(f):
            dets.append(dets[item[1]] if item[0] == 'copy' else person(*item, rng))
        assert len(dets) <= MAX_BOXES
        frames.append(_frame(dets))
    return frames


def _drift(f):
    return [(100 + 6 * f, 150 + 2 * f, 160, .9), (320 - 4 * f, 300, 200, .8), (540, 200 + 5 * f, 180, .7)]


def _crossing(f):
    return [(250 + 10 * f, 200, 200, .9), (360 - 10 * f, 260, 200, .8)]


def _absent(frames_away):
    def script(f):
        dets = [(150, 200, 180, .9)] if not 4 <= f < 4 + frames_away else []
        return dets + [(450, 250, 180, .8)]
    return script


def _late_empty_weak(f):
    if f == 8:
        return []
    dets = [(120 + 3 * f, 240, 200, .9)]
    if 2 <= f <= 4:
        dets.append((320, 120, 120, .2))                            # below new_track_score, away from everybody: untracked
    if f >= 5:
        dets.append((500, 240 - 2 * f, 180, .6))
    return dets


def _crowd_of_six(f):
    """Six persons and four slots: two overflow in every frame; person 1 leaves after frame 3, its slot is freed in frame 6
    (misses 3 > 2) and taken by an overflowing person in that same frame."""
    xs = (60, 160, 260, 360, 460, 560)
    return [(x + 2 * f, 240, 180, .9 - .05 * i) for i, x in enumerate(xs) if not (i == 1 and f >= 4)]


def _identical(f):
    dets = [(200 + 4 * f, 240, 200, .9), (480, 240, 180, .8)]
    if f in (3, 4, 7):
        dets.append(('copy', 0))                                    # the first person twice, byte for byte
    return dets


def _entrants(f):
    """Three persons, two more from frame 5 on, four slots: the fifth overflows until a leaver's slot is freed."""
    dets = [(80, 200, 160, .9), (240, 200, 160, .8)]
    if f < 7:
        dets.append((400, 200, 160, .7))
    if f >= 5:
        dets += [(560, 200, 160, .6), (320, 400, 120, .5)]
    return dets


# name -> (max_tracks, script); the expected ids of three of them are written out in tests/test_pose_track_host.py
SCRIPTS = [('drift', 8, _drift), ('crossing', 8, _crossing), ('absent_max_misses', 8, _absent(MAX_MISSES)),
           ('absent_one_more', 8, _absent(MAX_MISSES + 1)), ('late_empty_weak', 8, _late_empty_weak), ('identical', 8, _identical),
           ('crowd_of_six', 4, _crowd_of_six), ('entrants', 4, _entrants)]

_cache = {}


def cases():
    """[(name, max_tracks, frames)]: frames is the list of 12 result dicts. Built once."""
    if 'cases' not in _cache:
        rng = np.random.RandomState(SEED)
        _cache['cases'] = [(name, max_tracks, _sequence(script, rng)) for name, max_tracks, script in SCRIPTS]
    return _cache['cases']


def params(max_tracks, similarity):
    return ref.Params(max_tracks, similarity, MATCH_THRESHOLD, MAX_MISSES, NEW_TRACK_SCORE)


def pairs():
    """The table as two-stream cases: neighbours with the same max_tracks, stream 0 and stream 1 with different content."""
    table = cases()
    out = []
    for i in range(0, len(table), 2):
        a, b = table[i], table[i + 1]
        assert a[1] == b[1]
        out.append((a[0] + '+' + b[0], a[1], [a[2], b[2]]))
    return out


def reference(frames_per_stream, max_tracks, similarity, log=None):
    """The reference over a list of streams' sequences, frame by frame -> (rows[stream][frame], packed state after each frame).
    Computed once per (case, similarity) and shared: the reference does not depend on how a sequence is cut into calls."""
    key = (tuple(id(s) for s in frames_per_stream), max_tracks, similarity)
    if key not in _cache or log is not None:
        p = params(max_tracks, similarity)
        state = ref.new_state(len(frames_per_stream), max_tracks)
        rows = [[] for _ in frames_per_stream]
        packed = []
        for f in range(FRAMES):
            got = ref.run([seq[f] for seq in frames_per_stream], state, p, log)
            for s, g in enumerate(got):
                rows[s].append(g)
            packed.append(ref.pack_state(state))
        _cache[key] = (rows, packed)
    return _cache[key]
