"""Inputs for mpn_pose_track_motion, shared by tests/test_pose_motion_host.py (which asserts what the GPU comparison relies on)
and tests/test_pose_motion_gpu.py. Box-only sequences under IoU - float32 arithmetic that is the same on both sides, all
values dyadic where a test states ids - their twins with keypoints (a rigid 17-joint person on a quarter-pixel grid whose
centroid is exact in float32, so that a steady walk is predicted byte for byte), `track_assign_cases`' table, crowd and box
cases run with motion, and a two-person crossing with a drop-out. References are computed once and never changed."""
import collections

import numpy as np

import track_assign_cases as acases
import track_cases as cases
import track_motion_ref as mref
import track_ref as ref

NEW_TRACK_SCORE = 0.3
GAIN, DAMPING = 0.5, 1.0
ASSIGNMENTS = ('greedy', 'optimal')

# frames: the result dicts of ONE stream; streams > 1 cases carry a list of such lists in `seqs`
Case = collections.namedtuple('Case', 'name similarities max_tracks max_boxes match_threshold max_misses gain damping seqs')
_cache = {}


def _case(name, similarities, max_tracks, max_boxes, thr, max_misses, frames, gain=GAIN, damping=DAMPING, seqs=None):
    return Case(name, similarities, max_tracks, max_boxes, thr, max_misses, gain, damping, seqs if seqs is not None else [frames])


# ---- box sequences (IoU) ----

def occlusion_xs():
    """x = 0.5 i for frames 0..7, absent in 8..10, back at 0.5 i for 11..14."""
    return [[0.5 * i] if not 8 <= i <= 10 else [] for i in range(15)]


def acceleration_xs():
    """The step grows by 0.25 per frame: x = the running sum of 0, 0.25, 0.5, .. 2.0."""
    return [[float(x)] for x in np.cumsum(0.25 * np.arange(9))]


def boxes_of(xs_per_frame):
    return [acases.frame(xs) for xs in xs_per_frame]


def reuse_slot_xs():
    """Two slots, max_misses 1. A walks on; B leaves after frame 1 and its slot is freed in frame 3 (misses 2 > 1); C enters in
    that same frame into the slot just freed and walks the other way: its velocities start from nothing."""
    out = []
    for f in range(8):
        xs = [0.25 * f]
        if f <= 1:
            xs.append(4.0 + 0.5 * f)
        if f >= 3:
            xs.append(9.0 - 0.375 * f)
        out.append(xs)
    return out


def one_slot_xs():
    """One slot and two persons: the first is tracked and predicted, the second overflows in every frame."""
    return [[0.5 * f, 5.0] for f in range(5)]


# ---- persons with keypoints (OKS and IoU) ----

WIDTH, HEIGHT = 640, 480
PERSON = 128.0                          # a person's height in pixels; the width is half of it


def _skeleton():
    """Joint offsets from the centre on a quarter-pixel grid whose sums over the 17 joints are 0: the centroid of a person at
    (cx, cy) on that grid is (cx, cy) exactly, every partial sum being a multiple of 1/4 below 2^14."""
    x = np.round(cases._X * (PERSON / 2) * 4) / 4
    y = np.round(cases._Y * PERSON * 4) / 4
    x[0] -= x.sum()
    y[0] -= y.sum()
    assert x.sum() == 0 and y.sum() == 0
    return x, y


def person(cx, cy, score=0.9):
    """(box f32 [4], score f32, keypoints f32 [17,3]); cx, cy multiples of 1/4."""
    x, y = _skeleton()
    kp = np.zeros((17, 3), np.float32)
    kp[:, 0], kp[:, 1], kp[:, 2] = cx + x, cy + y, 0.5 + 0.02 * np.arange(17)
    w = PERSON / 2
    box = np.array([(cy - PERSON / 2) / HEIGHT, (cx - w / 2) / WIDTH, (cy + PERSON / 2) / HEIGHT, (cx + w / 2) / WIDTH], np.float32)
    return box, np.float32(score), kp


def persons_of(centres_per_frame):
    return [cases._frame([person(*c) for c in centres]) for centres in centres_per_frame]


def occlusion_kp_centres():
    """The occlusion case in pixels: 8 px a frame (one step still matches under OKS, four do not)."""
    return [[(100.0 + 8.0 * i, 240.0)] if not 8 <= i <= 10 else [] for i in range(15)]


def acceleration_kp_centres():
    """The step grows by 4 px a frame, up to 32 px."""
    return [[(100.0 + float(x), 240.0)] for x in np.cumsum(4.0 * np.arange(9))]


def crossing_centres():
    """Two persons walk through each other at 8 and 7.5 px a frame, 24 px apart in height; the first is hidden in frames 5 and
    6, while they pass, and is back on the far side."""
    out = []
    for f in range(12):
        c = [(280.0 - 7.5 * f, 252.0, 0.8)]
        if f not in (5, 6):
            c.insert(0, (200.0 + 8.0 * f, 228.0, 0.9))
        out.append(c)
    return out


def all_cases():
    if 'cases' not in _cache:
        iou, both = ('iou',), ('iou', 'oks')
        out = [
            _case('occlusion', iou, 4, 2, 0.3, 4, boxes_of(occlusion_xs())),
            _case('occlusion_damped', iou, 4, 2, 0.3, 4, boxes_of(occlusion_xs()), damping=0.5),
            _case('acceleration', iou, 8, 2, 0.3, 4, boxes_of(acceleration_xs())),
            _case('reuse_slot', iou, 2, 4, 0.3, 1, boxes_of(reuse_slot_xs())),
            _case('one_slot', iou, 1, 2, 0.3, 2, boxes_of(one_slot_xs())),
            _case('occlusion_kp', both, 4, 2, 0.3, 4, persons_of(occlusion_kp_centres())),
            _case('acceleration_kp', both, 8, 2, 0.3, 4, persons_of(acceleration_kp_centres())),
            _case('crossing_dropout', both, 4, 4, 0.3, 4, persons_of(crossing_centres())),
        ]
        # track_assign_cases' box sequences: an empty frame, a NaN box, more and fewer detections than tracks, ties, and 64
        # detections on 64 slots
        for name, max_tracks, max_boxes, thr, frames in acases.iou_cases():
            if name in ('empty_frame', 'nan_box', 'more_and_fewer', 'equal_boxes', 'crossing_2x2', 'random64'):
                out.append(_case(name, iou, max_tracks, max_boxes, thr, acases.MAX_MISSES, frames))
            if name == 'random64':                                  # the same 64 detections on a single slot: 63 overflow
                out.append(_case('random64_one_slot', iou, 1, max_boxes, thr, acases.MAX_MISSES, frames))
        for streams in (1, 2):
            for name, max_tracks, seqs in acases.table(streams):
                out.append(_case('table_' + name, both, max_tracks, cases.MAX_BOXES, cases.MATCH_THRESHOLD, cases.MAX_MISSES, None, seqs=seqs))
        for max_tracks in (64, 40):
            out.append(_case(f'crowd{max_tracks}', both, max_tracks, 64, cases.MATCH_THRESHOLD, cases.MAX_MISSES, acases.crowd()))
        _cache['cases'] = out
    return _cache['cases']


def case(name):
    return next(c for c in all_cases() if c.name == name)


def combos():
    """[(case name, similarity, assignment)]: what both test files walk."""
    return [(c.name, similarity, assignment) for c in all_cases() for similarity in c.similarities for assignment in ASSIGNMENTS]


def params(c, similarity, assignment, gain=None, damping=None):
    return mref.Params(c.max_tracks, similarity, c.match_threshold, c.max_misses, NEW_TRACK_SCORE, assignment,
                       c.gain if gain is None else gain, c.damping if damping is None else damping)


Reference = collections.namedtuple('Reference', 'rows packed motion log')


def reference(name, similarity, assignment, gain=None, damping=None):
    """The reference frame by frame: rows[stream][frame], and the packed track and motion states after each frame; the log of
    its decisions. Computed once per key and shared."""
    key = (name, similarity, assignment, gain, damping)
    if key not in _cache:
        c = case(name)
        p = params(c, similarity, assignment, gain, damping)
        state = mref.new_state(len(c.seqs), c.max_tracks)
        rows, packed, motion, log = [[] for _ in c.seqs], [], [], []
        with np.errstate(invalid='ignore'):                         # (the NaN box)
            for f in range(len(c.seqs[0])):
                for s, g in enumerate(mref.run([seq[f] for seq in c.seqs], state, p, log)):
                    rows[s].append(g)
                packed.append(mref.pack_state(state))
                motion.append(mref.pack_motion(state))
        _cache[key] = Reference(rows, packed, motion, log)
    return _cache[key]


def plain_reference(name, similarity, assignment):
    """The same case under the reference without motion (`track_ref` or `track_assign_ref`): (rows[stream][frame], packed)."""
    key = ('plain', name, similarity, assignment)
    if key not in _cache:
        c = case(name)
        module = ref if assignment == 'greedy' else acases.opt
        p = ref.Params(c.max_tracks, similarity, c.match_threshold, c.max_misses, NEW_TRACK_SCORE)
        state = module.new_state(len(c.seqs), c.max_tracks)
        rows, packed = [[] for _ in c.seqs], []
        with np.errstate(invalid='ignore'):
            for f in range(len(c.seqs[0])):
                for s, g in enumerate(module.run([seq[f] for seq in c.seqs], state, p)):
                    rows[s].append(g)
                packed.append(module.pack_state(state))
        _cache[key] = (rows, packed)
    return _cache[key]


def ids_of(rows):
    """The first person's id per frame of stream 0, None where the frame has no person."""
    return [int(r['track_ids'][0]) if len(r['track_ids']) else None for r in rows[0]]
