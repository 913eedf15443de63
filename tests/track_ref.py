"""The definition of mpn_pose_track (include/mpn.h) as plain loops in numpy: float32 for IoU, float64 for OKS, one operation
per line in the documented order. Test infrastructure only; the kernel and `tracking.PoseTracker` are compared with it.

    state = new_state(streams, max_tracks)
    rows = run(outputs, state, params)              # b = streams * F result dicts in, b dicts of per-person arrays out
    pack_state(state)                               # the bytes mpn_pose_track leaves in `next`

`run(..., log=[])` appends every comparison whose outcome a last-bit difference in a similarity could change: each
similarity against the threshold, and each round's winner against every other pair that was still open, with a flag for a
tie that cannot break: the two pairs have byte-identical inputs (the same arithmetic on the same bits), or - OKS - each
detection repeats its own track's keypoints byte for byte (a video that stands still): every dx and dy is 0, e is 0 / ... = 0,
exp(-0.0) is exactly 1 in any exp that is within 1 ulp and monotonic, and the OKS is 17 / 17 = 1 on both sides."""
import collections

import numpy as np

K = 17
# cocoeval.py, Params.setKpParams; computeOks: vars = (sigmas * 2)**2
SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
VARS = (SIGMAS * 2) ** 2
EPS = np.spacing(1)
FLAG_NEW, FLAG_OVERFLOW = 1, 2
DATA = 5 + 3 * K                        # box[4], score, keypoints[17][3]

Params = collections.namedtuple('Params', 'max_tracks similarity match_threshold max_misses new_track_score')


class Stream:
    def __init__(self, max_tracks):
        self.next_id, self.dropped = 1, 0
        self.id = np.zeros(max_tracks, np.int32)
        self.hits, self.age, self.misses = np.zeros(max_tracks, np.int32), np.zeros(max_tracks, np.int32), np.zeros(max_tracks, np.int32)
        self.data = np.zeros((max_tracks, DATA), np.float32)


def new_state(streams, max_tracks):
    return [Stream(max_tracks) for _ in range(streams)]


def pack_state(state):
    out = []
    for st in state:
        out.append(np.array([st.next_id, st.dropped, 0, 0], np.int32).tobytes())
        for t in range(len(st.id)):
            out.append(np.array([st.id[t], st.hits[t], st.age[t], st.misses[t]], np.int32).tobytes())
            out.append(st.data[t].tobytes())
    return b''.join(out)


def iou(a, b):
    """Two record boxes (ymin, xmin, ymax, xmax), float32 scalars throughout."""
    zero = np.float32(0)
    x0 = a[1] if a[1] > b[1] else b[1]
    x1 = a[3] if a[3] < b[3] else b[3]
    y0 = a[0] if a[0] > b[0] else b[0]
    y1 = a[2] if a[2] < b[2] else b[2]
    iw = x1 - x0
    ih = y1 - y0
    iw = iw if iw > zero else zero
    ih = ih if ih > zero else zero
    inter = iw * ih
    area_a = (a[3] - a[1]) * (a[2] - a[0])
    area_b = (b[3] - b[1]) * (b[2] - b[0])
    union = area_a + area_b - inter
    assert inter.dtype == np.float32 and union.dtype == np.float32
    return inter / union if union > zero else zero


def extent_area(kp):
    """keypoints float32 [17,3]: min / max in float32, differences and product in float64."""
    xl, xh, yl, yh = kp[:, 0].min(), kp[:, 0].max(), kp[:, 1].min(), kp[:, 1].max()
    return (np.float64(xh) - np.float64(xl)) * (np.float64(yh) - np.float64(yl))


def oks(track_kp, det_kp):
    """The track's keypoints in the ground-truth role, all 17 visible (cocoeval.py computeOks)."""
    denom = extent_area(track_kp) + EPS
    total = np.float64(0.0)
    for k in range(K):
        dx = np.float64(det_kp[k, 0]) - np.float64(track_kp[k, 0])
        dy = np.float64(det_kp[k, 1]) - np.float64(track_kp[k, 1])
        e = (dx * dx + dy * dy) / VARS[k] / denom / 2
        total += np.exp(-e)
    return total / np.float64(K)


def _arrays(o):
    """A result dict -> boxes f32 [n,4], scores f32 [n], keypoints f32 [n,17,3] (zeros where the dict has none)."""
    scores = np.asarray(o['scores'], np.float32).reshape(-1)
    n = len(scores)
    boxes = np.asarray(o['boxes'], np.float32).reshape(-1, 4) if 'boxes' in o and len(o['boxes']) == n else np.zeros((n, 4), np.float32)
    kp = o.get('keypoints')
    kp = np.asarray(kp, np.float32).reshape(-1, K, 3) if kp is not None and len(kp) == n else np.zeros((n, K, 3), np.float32)
    return boxes, scores, kp


def step(st, o, p, log=None):
    """One frame of one stream: the state `st` is advanced in place; returns the frame's output rows."""
    boxes, scores, kps = _arrays(o)
    n, T = len(scores), len(st.id)
    det = np.concatenate([boxes, scores[:, None], kps.reshape(n, 3 * K)], axis=1).astype(np.float32) if n else np.zeros((0, DATA), np.float32)
    live = [t for t in range(T) if st.id[t] != 0]
    thr = np.float64(np.float32(p.match_threshold))
    sim = {}
    for t in live:
        for d in range(n):
            if p.similarity == 'iou':
                sim[t, d] = np.float64(iou(st.data[t, :4], det[d, :4]))
            else:
                sim[t, d] = oks(st.data[t, 5:].reshape(K, 3), det[d, 5:].reshape(K, 3))
            if log is not None:
                log.append(('threshold', float(sim[t, d]), float(thr), False))
    track_of, det_of = {}, {}
    # 1. greedy matching: the largest similarity first, ties to the smaller slot, then the smaller detection
    while True:
        best = None
        open_pairs = []
        for t in live:
            if t in det_of:
                continue
            for d in range(n):
                if d in track_of:
                    continue
                v = sim[t, d]
                if not v >= thr:
                    continue
                open_pairs.append((t, d))
                if best is None or v > best[0]:
                    best = (v, t, d)
        if best is None:
            break
        v, t, d = best
        if log is not None:
            for t2, d2 in open_pairs:
                if (t2, d2) != (t, d):
                    same = st.data[t2].tobytes() == st.data[t].tobytes() and det[d2].tobytes() == det[d].tobytes()
                    if p.similarity == 'oks' and not same:          # both detections repeat their own track's keypoints
                        same = all(st.data[a, 5:].tobytes() == det[b, 5:].tobytes() for a, b in ((t, d), (t2, d2)))
                    log.append(('winner', float(v), float(sim[t2, d2]), same))
        det_of[t], track_of[d] = d, t
    row_slot, row_flags, row_sim = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    for t in live:
        if t in det_of:                                             # 2. a matched track takes the detection
            d = det_of[t]
            st.data[t] = det[d]
            st.misses[t] = 0
            st.hits[t] += 1
            st.age[t] += 1
            row_slot[d], row_sim[d] = t, sim[t, d]
        else:                                                       # 3. an unmatched one ages, and is freed past max_misses
            st.misses[t] += 1
            st.age[t] += 1
            if st.misses[t] > p.max_misses:
                st.id[t] = st.hits[t] = st.age[t] = st.misses[t] = 0
                st.data[t] = 0
    for d in range(n):                                              # 4. births, in row order, into the lowest free slot
        if d in track_of or not scores[d] >= np.float32(p.new_track_score):
            continue
        free = [t for t in range(T) if st.id[t] == 0]
        if not free:
            row_flags[d] = FLAG_OVERFLOW
            st.dropped += 1
            continue
        t = free[0]
        st.id[t], st.hits[t], st.age[t], st.misses[t] = st.next_id, 1, 1, 0
        st.next_id += 1
        st.data[t] = det[d]
        row_slot[d], row_flags[d] = t, FLAG_NEW
    ids = np.array([st.id[t] if t >= 0 else 0 for t in row_slot], np.int32).reshape(n)
    hits = np.array([st.hits[t] if t >= 0 else 0 for t in row_slot], np.int32).reshape(n)
    return {'track_ids': ids, 'slots': row_slot, 'track_hits': hits, 'flags': row_flags, 'track_new': (row_flags & FLAG_NEW) != 0,
            'track_similarity': row_sim}


def run(outputs, state, p, log=None):
    """b = streams * F result dicts: stream s owns images s*F .. s*F+F-1 in time order. The state is advanced in place."""
    streams = len(state)
    assert len(outputs) % streams == 0
    F = len(outputs) // streams
    return [step(state[i // F], o, p, log) for i, o in enumerate(outputs)]


def undecided(log, margin=1e-9):
    """The logged comparisons a last-bit difference could flip: neither an exact tie of bit-identical inputs nor apart by a
    relative margin above `margin`."""
    bad = []
    for kind, a, b, same in log:
        if kind == 'winner' and a == b and same:
            continue
        if not abs(a - b) > margin * max(abs(a), abs(b)):
            bad.append((kind, a, b, same))
    return bad
