"""Inputs for mpn_pose_track_optimal, shared by tests/test_pose_assign_host.py (which asserts what the GPU comparison relies
on) and tests/test_pose_assign_gpu.py: box-only sequences under IoU - float32 arithmetic that is the same on both sides, so
ties and near-ties are welcome there - and `track_cases`' table and a crowd of 48 under OKS. References are computed once."""
import numpy as np

import track_assign_ref as opt
import track_cases as cases
import track_ref as ref

MAX_MISSES = 2
NEW_TRACK_SCORE = 0.3
_cache = {}


def frame(xs, y0=0.0, y1=1.0, width=1.0, scores=None):
    """Boxes (ymin, xmin, ymax, xmax) of one width in a row at the given xmin values."""
    xs = np.asarray(xs, np.float32).reshape(-1)
    n = len(xs)
    boxes = np.stack([np.full(n, y0, np.float32), xs, np.full(n, y1, np.float32), xs + np.float32(width)], axis=1).reshape(n, 4)
    return {'boxes': boxes.astype(np.float32), 'scores': np.full(n, 0.9, np.float32) if scores is None else np.asarray(scores, np.float32)}


def chain(n):
    """n unit boxes in a row, then the same persons half a box and 1/256 further right (exact in float32): every detection
    overlaps its own track (IoU 0.3299) a little less than its right-hand neighbour's (0.3368)."""
    return [frame(np.arange(n)), frame(np.arange(n) + (0.5 + 1.0 / 256))]


def crossing():
    """Tracks at x = 0 and 0.1337; detection 0 at 0.0526 (IoU 0.90 with track 0, 0.85 with track 1), detection 1 at -0.1111
    (0.80 with track 0, 0.61 with track 1: below the threshold 0.7). Greedy takes 0.90 and leaves detection 1 alone; the
    optimum is 0.85 + 0.80."""
    return [frame([0.0, 0.1337]), frame([0.0526, -0.1111]), frame([0.06, -0.1])]


def random64(frames=3, seed=11):
    """64 boxes of 1 x 1 with corners in a 4 x 4 square: each overlaps about eight others above the threshold. The later
    frames are the same persons moved by up to 0.3, in a shuffled row order."""
    rng = np.random.RandomState(seed)
    at = rng.uniform(0, 4, (64, 2))
    seq = []
    for f in range(frames):
        order = rng.permutation(64) if f else np.arange(64)
        yx = (at + (rng.uniform(-0.3, 0.3, (64, 2)) if f else 0))[order].astype(np.float32)
        boxes = np.concatenate([yx, yx + np.float32(1)], axis=1).astype(np.float32)
        seq.append({'boxes': boxes, 'scores': np.full(64, 0.9, np.float32)})
    return seq


def nan_box():
    second = frame([0.0, 2.0, 4.1])
    second['boxes'][1, 1] = np.nan                                  # its xmin: the IoU with every track is not >= anything
    return [frame([0.0, 2.0, 4.0]), second, frame([0.1, 2.0, 4.0]), frame([0.1, 2.0, 4.0])]


def iou_cases():
    """[(name, max_tracks, max_boxes, match_threshold, frames)]."""
    if 'iou' not in _cache:
        _cache['iou'] = [
            ('one_by_one', 1, 1, 0.3, [frame([0.0]), frame([0.1]), frame([0.15])]),
            ('crossing_2x2', 4, 4, 0.7, crossing()),
            # two tracks and five detections, then five tracks and two detections (which go to the fourth and the first)
            ('more_and_fewer', 8, 8, 0.3, [frame([0.0, 3.0]), frame([0.2, 0.4, 2.9, 3.3, 6.0]), frame([3.2, 0.25])]),
            ('all_below', 8, 8, 0.5, [frame([0.0, 1.0, 2.0]), frame([0.5, 1.5, 2.5]), frame([0.5, 1.5, 2.5])]),
            ('empty_frame', 8, 8, 0.3, [frame([0.0, 0.5]), frame([]), frame([0.6, 0.1])]),
            ('nan_box', 8, 8, 0.3, nan_box()),
            ('chain16', 24, 16, 0.3, chain(16)),
            ('chain64', 64, 64, 0.3, chain(64)),
            ('random64', 64, 64, 0.3, random64()),
            # every box the same: every weight ties and only the stated order decides
            ('equal_boxes', 8, 8, 0.3, [frame([1.0] * 6), frame([1.0] * 6), frame([1.0] * 4), frame([1.0] * 7)]),
        ]
    return _cache['iou']


def iou_params(max_tracks, match_threshold):
    return ref.Params(max_tracks, 'iou', match_threshold, MAX_MISSES, NEW_TRACK_SCORE)


def iou_reference(name, module=opt, log=None):
    """(rows per frame, packed state after each frame) of one IoU case under `module` (the optimal or the greedy reference)."""
    key = ('iou', name, module.__name__)
    if key not in _cache or log is not None:
        _, max_tracks, _, thr, frames = next(c for c in iou_cases() if c[0] == name)
        state = module.new_state(1, max_tracks)
        rows, packed = [], []
        with np.errstate(invalid='ignore'):                         # (the NaN box)
            for o in frames:
                rows += module.run([o], state, iou_params(max_tracks, thr), log)
                packed.append(module.pack_state(state))
        _cache[key] = (rows, packed)
    return _cache[key]


def table(streams):
    """`track_cases`' table as one-stream or two-stream cases: [(name, max_tracks, [frames per stream])]."""
    return [(name, mt, [frames]) for name, mt, frames in cases.cases()] if streams == 1 else cases.pairs()


def table_reference(seqs, max_tracks, similarity, module=opt, log=None):
    """`track_cases.reference` under `module`: (rows[stream][frame], packed state after each frame)."""
    key = ('table', tuple(id(s) for s in seqs), max_tracks, similarity, module.__name__)
    if key not in _cache or log is not None:
        p = cases.params(max_tracks, similarity)
        state = module.new_state(len(seqs), max_tracks)
        rows, packed = [[] for _ in seqs], []
        for f in range(cases.FRAMES):
            for s, g in enumerate(module.run([seq[f] for seq in seqs], state, p, log)):
                rows[s].append(g)
            packed.append(module.pack_state(state))
        _cache[key] = (rows, packed)
    return _cache[key]


def crowd(frames=3, columns=8, lines=6):
    """48 persons on a grid of a 1000 x 1000 image, drifting; the last person of every line is missing in frame 1. With 40
    slots eight persons overflow."""
    if 'crowd' not in _cache:
        rng = np.random.RandomState(7)
        _cache['crowd'] = [cases._frame([cases.person(80 + 120 * c + 3 * f, 90 + 150 * l + 2 * f, 100, 0.9 - 0.01 * (c + columns * l), rng)
                                         for l in range(lines) for c in range(columns) if not (f == 1 and c == columns - 1)])
                           for f in range(frames)]
    return _cache['crowd']


def crowd_reference(max_tracks, similarity, log=None):
    key = ('crowd', max_tracks, similarity)
    if key not in _cache or log is not None:
        state = opt.new_state(1, max_tracks)
        rows = opt.run(crowd(), state, ref.Params(max_tracks, similarity, cases.MATCH_THRESHOLD, cases.MAX_MISSES, cases.NEW_TRACK_SCORE), log)
        _cache[key] = (rows, opt.pack_state(state), state[0].dropped)
    return _cache[key]
