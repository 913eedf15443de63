"""The definition of mpn_pose_track_motion (include/mpn.h) as plain loops in numpy: `track_ref`'s IoU, OKS and state with the
track's PREDICTED pose in the track's role, step 1 either `track_ref`'s greedy rounds or `track_assign_ref`'s optimal assignment,
the velocity update and the coasting rows; float32 scalars, one operation per line in the documented order. Test
infrastructure only; the kernel and `tracking.PoseTracker(motion=...)` are compared with it.

    state = new_state(streams, max_tracks)
    rows = run(outputs, state, params)              # b = streams * F result dicts in, b dicts of per-person arrays out
    pack_state(state), pack_motion(state)           # the bytes the launch leaves in `next` and `motion_next`
    pack_coast(rows, max_tracks)                    # the bytes it leaves in `coast_out`

`run(..., log=[])` appends what the reference of the chosen assignment appends ('threshold' and 'winner', or 'threshold',
'quantum' and 'path'); `undecided(log, assignment)` is that reference's. An exact tie ("same") is one of byte-identical
predicted poses and detections, or - OKS - of detections that repeat their own track's predicted keypoints byte for byte."""
import collections

import numpy as np

import track_assign_ref as opt
import track_ref as ref
from track_ref import FLAG_NEW, FLAG_OVERFLOW, DATA, K, pack_state  # noqa: F401

V = 6                                   # vel[0..3]: the box, vel[4..5]: the keypoint centroid (x, y)
COAST = np.dtype([('id', np.int32), ('misses', np.int32), ('box', np.float32, (4,)), ('keypoints', np.float32, (K, 2))])

Params = collections.namedtuple('Params', 'max_tracks similarity match_threshold max_misses new_track_score assignment '
                                          'velocity_gain damping')


def new_state(streams, max_tracks):
    state = ref.new_state(streams, max_tracks)
    for st in state:
        st.mid, st.seen = np.zeros(max_tracks, np.int32), np.zeros(max_tracks, np.int32)
        st.vel = np.zeros((max_tracks, V), np.float32)
    return state


def pack_motion(state):
    out = []
    for st in state:
        out.append(np.zeros(4, np.int32).tobytes())
        for t in range(len(st.id)):
            out.append(np.array([st.mid[t], st.seen[t]], np.int32).tobytes())
            out.append(st.vel[t].tobytes())
    return b''.join(out)


def pack_coast(rows, max_tracks):
    """The coasting rows of a launch over these images: max_tracks rows of 160 bytes each, packed at the front, the rest zero."""
    out = np.zeros((len(rows), max_tracks), COAST)
    for i, r in enumerate(rows):
        m = len(r['coasting_ids'])
        out['id'][i, :m], out['misses'][i, :m] = r['coasting_ids'], r['coasting_misses']
        out['box'][i, :m], out['keypoints'][i, :m] = r['coasting_boxes'], r['coasting_keypoints']
    return out.tobytes()


def centroid(kp):
    """keypoints float32 [17, >= 2] -> (cx, cy): the sums in keypoint order from the first keypoint on, then / 17."""
    sx, sy = kp[0, 0], kp[0, 1]
    for k in range(1, K):
        sx = sx + kp[k, 0]
        sy = sy + kp[k, 1]
    assert sx.dtype == np.float32
    return sx / np.float32(17), sy / np.float32(17)


def predict(data, vel, misses):
    """Step 0 of one slot: (pbox f32 [4], pkp f32 [17,2])."""
    gap = np.float32(int(misses) + 1)
    pbox = np.zeros(4, np.float32)
    for c in range(4):
        pbox[c] = data[c] + vel[c] * gap
    kp = data[5:].reshape(K, 3)
    pkp = np.zeros((K, 2), np.float32)
    for k in range(K):
        pkp[k, 0] = kp[k, 0] + vel[4] * gap
        pkp[k, 1] = kp[k, 1] + vel[5] * gap
    return pbox, pkp


def _greedy(live, n, sim, thr, same_pair, log):
    """Step 1 of mpn_pose_track: track_ref's rounds."""
    track_of, det_of = {}, {}
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
                    log.append(('winner', float(v), float(sim[t2, d2]), same_pair((t, d), (t2, d2))))
        det_of[t], track_of[d] = d, t
    return det_of


def _optimal(live, n, T, sim, thr, exact_pair, log):
    """Step 1 of mpn_pose_track_optimal: track_assign_ref's problem and algorithm."""
    cost = {}
    for t in live:
        for d in range(n):
            if not sim[t, d] >= thr:
                continue
            cost[d + 1, t + 1] = -(opt.quantum(sim[t, d]) + 1)
            if log is not None:
                scaled = float(sim[t, d]) * opt.QUANTA
                log.append(('quantum', scaled, abs(scaled - round(scaled)), sim[t, d] == 1.0 and exact_pair(t, d)))
    for d in range(n):
        cost[d + 1, T + d + 1] = 0
    on = opt.assign(cost, n, T, log)
    return {j - 1: on[j] - 1 for j in range(1, T + 1) if on[j] != 0}


def step(st, o, p, log=None):
    """One frame of one stream: the state `st` is advanced in place; returns the frame's output rows and coasting rows."""
    boxes, scores, kps = ref._arrays(o)
    n, T = len(scores), len(st.id)
    det = np.concatenate([boxes, scores[:, None], kps.reshape(n, 3 * K)], axis=1).astype(np.float32) if n else np.zeros((0, DATA), np.float32)
    gain, damping = np.float32(p.velocity_gain), np.float32(p.damping)
    for t in range(T):                                              # velocities another track left, or none, read as zero
        if st.id[t] == 0 or st.mid[t] != st.id[t]:
            st.mid[t], st.seen[t] = st.id[t], 0
            st.vel[t] = 0
    live = [t for t in range(T) if st.id[t] != 0]
    thr = np.float64(np.float32(p.match_threshold))
    pred = {t: predict(st.data[t], st.vel[t], st.misses[t]) for t in live}      # 0. the prediction
    sim = {}
    for t in live:
        pbox, pkp = pred[t]
        for d in range(n):
            if p.similarity == 'iou':
                sim[t, d] = np.float64(ref.iou(pbox, det[d, :4]))
            else:
                sim[t, d] = ref.oks(pkp, det[d, 5:].reshape(K, 3))
            if log is not None:
                log.append(('threshold', float(sim[t, d]), float(thr), False))

    def repeats(t, d):                                              # the detection's keypoints are the predicted ones, byte for byte
        return pred[t][1].tobytes() == np.ascontiguousarray(det[d, 5:].reshape(K, 3)[:, :2]).tobytes()

    def same_pair(a, b):
        same = all(x.tobytes() == y.tobytes() for x, y in zip(pred[a[0]], pred[b[0]])) and det[a[1]].tobytes() == det[b[1]].tobytes()
        return same or (p.similarity == 'oks' and repeats(*a) and repeats(*b))
    if p.assignment == 'greedy':
        det_of = _greedy(live, n, sim, thr, same_pair, log)
    else:
        det_of = _optimal(live, n, T, sim, thr, repeats, log)
    track_of = {d: t for t, d in det_of.items()}
    row_slot, row_flags, row_sim = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    coasting = []
    for t in live:
        if t in det_of:                                             # 2. a matched track takes the detection
            d = det_of[t]
            gap = np.float32(int(st.misses[t]) + 1)
            last = list(st.data[t, :4]) + list(centroid(st.data[t, 5:].reshape(K, 3)))
            z = list(det[d, :4]) + list(centroid(det[d, 5:].reshape(K, 3)))
            g = np.float32(1) if st.seen[t] == 0 and gain > 0 else gain
            for c in range(V):
                vobs = (z[c] - last[c]) / gap
                st.vel[t, c] = st.vel[t, c] + g * (vobs - st.vel[t, c])
            st.seen[t] += 1
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
                st.mid[t] = st.seen[t] = 0
                st.vel[t] = 0
            else:
                for c in range(V):
                    st.vel[t, c] = st.vel[t, c] * damping
                coasting.append(t)
    coast = np.zeros(len(coasting), COAST)
    for r, t in enumerate(coasting):                                # the live slots nothing matched, at step 0's pose
        coast[r] = (st.id[t], st.misses[t], pred[t][0], pred[t][1])
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
        st.mid[t], st.seen[t] = st.next_id, 0
        st.vel[t] = 0
        st.next_id += 1
        st.data[t] = det[d]
        row_slot[d], row_flags[d] = t, FLAG_NEW
    ids = np.array([st.id[t] if t >= 0 else 0 for t in row_slot], np.int32).reshape(n)
    hits = np.array([st.hits[t] if t >= 0 else 0 for t in row_slot], np.int32).reshape(n)
    return {'track_ids': ids, 'slots': row_slot, 'track_hits': hits, 'flags': row_flags, 'track_new': (row_flags & FLAG_NEW) != 0,
            'track_similarity': row_sim, 'coasting_ids': coast['id'].copy(), 'coasting_misses': coast['misses'].copy(),
            'coasting_boxes': coast['box'].copy(), 'coasting_keypoints': coast['keypoints'].copy()}


def run(outputs, state, p, log=None):
    """b = streams * F result dicts: stream s owns images s*F .. s*F+F-1 in time order. The state is advanced in place."""
    streams = len(state)
    assert len(outputs) % streams == 0
    F = len(outputs) // streams
    return [step(state[i // F], o, p, log) for i, o in enumerate(outputs)]


def undecided(log, assignment):
    """The logged decisions a last-bit difference in a similarity could flip, as the reference of `assignment` judges them."""
    return ref.undecided(log) if assignment == 'greedy' else opt.undecided(log)
