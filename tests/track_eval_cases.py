"""Handmade cases for mpn_track_eval and `track_metrics.TrackEvaluator`: a few frames each, with the numbers they must give
written out by hand in `expect`. Test infrastructure only.

A case: {'name', 'streams', 'threshold', 'outputs' (b dicts: 'keypoints' f32 [n,17,3], 'scores', 'boxes', 'track_ids'),
'groundtruth' (b dicts with 'track_ids': the file's ids), 'identities' (b arrays of dense indices, the order of first
appearance per stream - or what the case gives instead), 'raw_identities' (True: the dense indices are the case's own and go
to the kernel as they are), 'expect' (a subset of the metrics)}. b = streams * F, stream-major."""
import numpy as np

import track_eval_ref as ref

K = 17
# a person: 17 keypoints on a 5 x 4 grid of 10 x 20 pixel steps around its centre; the extent is 40 x 60
_DX = np.array([(k % 5 - 2) * 10.0 for k in range(K)])
_DY = np.array([(k // 5 - 1.5) * 20.0 for k in range(K)])
AREA = 40.0 * 60.0


def pose(cx, cy):
    kp = np.zeros((K, 3), np.float32)
    kp[:, 0], kp[:, 1], kp[:, 2] = cx + _DX, cy + _DY, 1.0
    return kp


def oks_at(shift):
    """The similarity of a person moved by `shift` pixels in x against its ground truth (in the arithmetic of the reference)."""
    kp = pose(500.0, 500.0)
    g = kp.astype(np.float64)
    g[:, 2] = 2
    moved = kp.copy()
    moved[:, 0] += np.float32(shift)
    return float(ref.oks(moved, g, (480.0, 470.0, 40.0, 60.0), AREA)[0])


def shift_for(target):
    """The whole number of quarter pixels (exact in float32 at these coordinates) whose similarity is nearest below `target`."""
    lo, hi = 0.0, 400.0
    for _ in range(60):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if oks_at(mid) > target else (lo, mid)
    return np.ceil(hi * 4) / 4


def person(track_id, cx, cy):
    return (track_id, pose(cx, cy))


def truth(file_id, cx, cy, crowd=False, visible=True):
    kp = pose(cx, cy).astype(np.float64)
    kp[:, 2] = 2 if visible else 0
    if not visible:
        kp[:, :2] = 0
    return (file_id, kp, (cx - 20.0, cy - 30.0, 40.0, 60.0), crowd)


def _output(persons):
    n = len(persons)
    kp = np.stack([p[1] for p in persons]).astype(np.float32) if n else np.zeros((0, K, 3), np.float32)
    boxes = np.zeros((n, 4), np.float32)
    for i in range(n):
        boxes[i] = (kp[i, :, 1].min() / 1000, kp[i, :, 0].min() / 1000, kp[i, :, 1].max() / 1000, kp[i, :, 0].max() / 1000)
    return {'keypoints': kp, 'scores': np.full(n, 0.9, np.float32), 'boxes': boxes,
            'keypoint_scores': np.ones((n, K), np.float32), 'keypoint_positions': np.zeros((n, K, 2), np.float32),
            'track_ids': np.array([p[0] for p in persons], np.int32).reshape(n)}


def _groundtruth(truths):
    g = len(truths)
    return {'keypoints': np.stack([t[1] for t in truths]) if g else np.zeros((0, K, 3)),
            'boxes': np.array([t[2] for t in truths], np.float64).reshape(g, 4),
            'area': np.full(g, AREA), 'iscrowd': np.array([int(t[3]) for t in truths], np.int32).reshape(g),
            'track_ids': np.array([t[0] for t in truths], np.int64).reshape(g)}


def dense_identities(groundtruth, streams):
    """The dense index of every ground truth: the order of first appearance of the file's ids within the stream, ignored rows
    (-1: no memory) left out - what `TrackEvaluator` does."""
    F = len(groundtruth) // streams
    seen = [{} for _ in range(streams)]
    out = []
    for i, gt in enumerate(groundtruth):
        _, _, _, ignore = ref.gt_arrays(gt)
        row = []
        for j, fid in enumerate(gt['track_ids']):
            row.append(-1 if ignore[j] else seen[i // F].setdefault(int(fid), len(seen[i // F])))
        out.append(np.array(row, np.int32).reshape(len(row)))
    return out


def case(name, frames, expect=None, streams=1, threshold=0.5, identities=None):
    outputs = [_output(p) for p, _ in frames]
    groundtruth = [_groundtruth(t) for _, t in frames]
    raw = identities is not None
    if not raw:
        identities = dense_identities(groundtruth, streams)
    return {'name': name, 'streams': streams, 'threshold': threshold, 'outputs': outputs, 'groundtruth': groundtruth,
            'identities': [np.asarray(i, np.int32) for i in identities], 'raw_identities': raw, 'expect': expect or {}}


A, B, C = (200.0, 200.0), (500.0, 200.0), (800.0, 200.0)
D95, D60, D35 = shift_for(0.95), shift_for(0.60), shift_for(0.35)


def _one_one():
    frames = [([person(1, *A)], [truth(7, *A)])] * 3
    return case('one_one', frames, {'num_frames': 3, 'num_objects': 3, 'num_predictions': 3, 'num_matches': 3, 'num_switches': 0,
                                    'num_misses': 0, 'num_false_positives': 0, 'mota': 1.0, 'motp': 1.0, 'recall': 1.0,
                                    'precision': 1.0, 'idtp': 3, 'idf1': 1.0, 'mostly_tracked': 1, 'num_fragmentations': 0})


def _empty_frames():
    frames = [([person(1, *A)], []), ([], [truth(7, *A)]), ([], [])]
    # one false positive, one miss: mota = 1 - 2 / 1; no pair ever overlaps: idtp = 0, idf1 = 0 / (0 + 1 + 1)
    return case('empty_frames', frames, {'num_frames': 3, 'num_objects': 1, 'num_predictions': 1, 'num_matches': 0,
                                         'num_misses': 1, 'num_false_positives': 1, 'mota': -1.0, 'recall': 0.0,
                                         'precision': 0.0, 'idtp': 0, 'idfp': 1, 'idfn': 1, 'idf1': 0.0, 'mostly_lost': 1})


def _swap():
    gts = [truth(10, *A), truth(20, *B)]
    frames = [([person(1, *A), person(2, *B)], gts), ([person(2, *A), person(1, *B)], gts), ([person(2, *A), person(1, *B)], gts)]
    # a switch each in the second frame, none in the third: mota = 1 - 2 / 6. Each identity is with one track for two of
    # its three frames: idtp = 4, idf1 = 8 / (8 + 2 + 2)
    return case('swap', frames, {'num_objects': 6, 'num_matches': 6, 'num_switches': 2, 'num_misses': 0, 'num_false_positives': 0,
                                 'mota': 1 - 2 / 6, 'recall': 1.0, 'idtp': 4, 'idfp': 2, 'idfn': 2, 'idf1': 2 / 3})


def _kept():
    # the old track is still eligible (about 0.6) and a nearer one (1.0) appears: the correspondence is kept, no switch
    frames = [([person(1, *A)], [truth(7, *A)]),
              ([person(2, *A), person(1, A[0] + D60, A[1])], [truth(7, *A)])]
    return case('kept', frames, {'num_objects': 2, 'num_predictions': 3, 'num_matches': 2, 'num_switches': 0,
                                 'num_false_positives': 1, 'mota': 0.5, 'idtp': 2, 'idf1': 2 * 2 / (2 * 2 + 1 + 0)})


def _two_by_two():
    # ground truths g0 at x and g1 at x + D95 + D35; persons h0 at x + D95 (0.95 with g0, 0.35 with g1) and h1 at x - D35
    # (0.35 with g0, far below 0.3 with g1). The larger sum, 0.95, has one pair; the rule takes the two pairs of 0.35.
    x, y = 500.0, 500.0
    frames = [([person(1, x + D95, y), person(2, x - D35, y)], [truth(1, x, y), truth(2, x + D95 + D35, y)])]
    return case('two_by_two', frames, {'num_objects': 2, 'num_matches': 2, 'num_misses': 0, 'num_false_positives': 0, 'mota': 1.0,
                                       'idtp': 2, 'idf1': 1.0}, threshold=0.3)


def _ignored():
    # a crowd region without keypoints (its doubled box takes the person in: similarity 1) absorbs track 2; track 3, far from
    # everything, is a false positive
    frames = [([person(1, *A), person(2, *B), person(3, *C)], [truth(7, *A), truth(8, *B, crowd=True, visible=False)])]
    return case('ignored', frames, {'num_objects': 1, 'num_predictions': 2, 'num_matches': 1, 'num_false_positives': 1,
                                    'num_misses': 0, 'mota': 0.0, 'precision': 0.5, 'idtp': 1, 'idfp': 1, 'idfn': 0})


def _untracked():
    frames = [([person(1, *A), person(0, *B)], [truth(7, *A), truth(8, *B)])]
    return case('untracked', frames, {'num_objects': 2, 'num_predictions': 1, 'num_matches': 1, 'num_misses': 1,
                                      'num_false_positives': 0, 'mota': 0.5, 'recall': 0.5, 'precision': 1.0})


def _no_memory():
    # an identity index outside the state: matched in every frame, never kept, never a switch, nothing stored
    frames = [([person(1, *A)], [truth(7, *A)]), ([person(2, *A)], [truth(7, *A)]), ([person(2, *A)], [truth(7, *A)])]
    return case('no_memory', frames, {'num_objects': 3, 'num_matches': 3, 'num_switches': 0, 'mota': 1.0},
                identities=[[9999], [-1], [256]])


def _trajectories():
    # ten frames. Identity 1: matched in frames 0-3 and 6-9 (8 of 10: mostly tracked, one fragmentation); identity 2: in frame
    # 0 alone (1 of 10: mostly lost); identity 3: in frames 0-4 (5 of 10: partially tracked). 14 matches of 30 objects.
    gts = [truth(1, *A), truth(2, *B), truth(3, *C)]
    frames = []
    for f in range(10):
        persons = []
        if f < 4 or f >= 6:
            persons.append(person(1, *A))
        if f == 0:
            persons.append(person(2, *B))
        if f < 5:
            persons.append(person(3, *C))
        frames.append((persons, gts))
    return case('trajectories', frames, {'num_frames': 10, 'num_objects': 30, 'num_predictions': 14, 'num_matches': 14,
                                         'num_misses': 16, 'num_switches': 0, 'num_false_positives': 0, 'mota': 1 - 16 / 30,
                                         'num_unique_objects': 3, 'mostly_tracked': 1, 'mostly_lost': 1, 'partially_tracked': 1,
                                         'num_fragmentations': 1, 'idtp': 14, 'idf1': 28 / (28 + 0 + 16)})


def _two_tracks_in_turn():
    # always matched (recall 1, one switch: mota 0.75), but the better of its two tracks covers half of it: idf1 0.5
    frames = [([person(1 if f < 2 else 2, *A)], [truth(7, *A)]) for f in range(4)]
    return case('two_tracks_in_turn', frames, {'num_objects': 4, 'num_matches': 4, 'num_switches': 1, 'recall': 1.0, 'mota': 0.75,
                                               'idtp': 2, 'idfp': 2, 'idfn': 2, 'idp': 0.5, 'idr': 0.5, 'idf1': 0.5})


def _full():
    # 64 x 64 in one frame: person p stands on ground truth (37 p) % 64, 100 pixels apart on a grid (bit 63, every lane)
    spots = [(100.0 + 100.0 * (i % 8), 100.0 + 100.0 * (i // 8)) for i in range(64)]
    frames = [([person(p + 1, *spots[(37 * p) % 64]) for p in range(64)], [truth(1000 + g, *spots[g]) for g in range(64)])]
    return case('full', frames, {'num_objects': 64, 'num_predictions': 64, 'num_matches': 64, 'num_misses': 0,
                                 'num_false_positives': 0, 'mota': 1.0, 'recall': 1.0, 'precision': 1.0})


def _video(streams):
    """16 frames (one stream), or the same 16 images as 4 streams of 4: three persons who drift, tracks that jitter around
    them by whole pixels, a track that changes hands, a person who is missed and a stray track."""
    rng = np.random.RandomState(5)
    frames = []
    for f in range(16):
        centres = [(200.0 + 6 * f, 300.0), (420.0 - 4 * f, 300.0 + 3 * f), (700.0, 320.0 + 5 * f)]
        gts = [truth(11, *centres[0]), truth(12, *centres[1]), truth(13, *centres[2], crowd=(f % 5 == 4))]
        ids = [1, 2, 3] if f < 7 else [1, 4, 3] if f < 11 else [4, 1, 3]
        persons = []
        for j, (cx, cy) in enumerate(centres):
            if j == 1 and f in (3, 4):
                continue
            jitter = rng.randint(-6, 7, 2).astype(np.float64)
            persons.append(person(ids[j] if not (j == 0 and f == 9) else 0, cx + jitter[0], cy + jitter[1]))
        if f % 3 == 0:
            persons.append(person(9, 900.0, 100.0 + f))
        order = rng.permutation(len(persons))
        frames.append(([persons[i] for i in order], gts))
    return case(f'video_{streams}', frames, streams=streams)


def all_cases():
    return [_one_one(), _empty_frames(), _swap(), _kept(), _two_by_two(), _ignored(), _untracked(), _no_memory(),
            _trajectories(), _two_tracks_in_turn(), _full(), _video(1), _video(4)]


CASES = all_cases()
