"""The definition of mpn_pose_track_optimal (include/mpn.h) as plain loops: `track_ref`'s similarities, state and steps 2 - 4,
with step 1 the maximum-weight matching of the gated pairs under weights quantised to integers, found by the
shortest-augmenting-path Hungarian method in the documented order (rows in row order, columns scanned upwards, ties to the
smaller column). Test infrastructure only; the kernel and `tracking.PoseTracker(assignment='optimal')` are compared with it.

    state = new_state(streams, max_tracks)
    rows = run(outputs, state, params)              # the interface of track_ref.run
    pack_state(state)

`run(..., log=[])` appends ('threshold', similarity, threshold, False) for every pair as `track_ref` does,
('quantum', similarity * 2^20, its distance from the nearest integer, exact) for every eligible pair - exact: the detection
repeats the track's keypoints byte for byte and the similarity is 1.0, `track_ref`'s docstring says why that is the same in
any exp within 1 ulp - and ('path', row, columns on the augmenting path that was flipped, columns the search for it took
into its tree: the trips of the kernel's scan loop) for every inserted row."""
import numpy as np

from track_ref import (FLAG_NEW, FLAG_OVERFLOW, DATA, K, Params, Stream, _arrays, iou, new_state, oks,  # noqa: F401
                       pack_state)

QUANTA = 1 << 20


def quantum(s):
    """floor(s * 2^20) in float64, clamped to 0 .. 2^20 before the conversion to an integer."""
    q = np.floor(np.float64(s) * np.float64(QUANTA))
    q = np.float64(0) if q < 0 else (np.float64(QUANTA) if q > QUANTA else q)
    return int(q)


def assign(cost, n, T, log=None):
    """cost: {(i, j): integer} over rows i = 1..n and columns j = 1..T+n, absent pairs left out; every row has its dummy column
    T + i. Returns p[0..m]: the row on column j, 0 = none."""
    m = T + n
    u, v, p, way = [0] * (n + 1), [0] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = [None] * (m + 1)
        used = [False] * (m + 1)
        steps = 0
        while True:
            steps += 1
            used[j0] = True
            i0 = p[j0]
            delta, j1 = None, None
            for j in range(1, m + 1):
                if used[j]:
                    continue
                if (i0, j) in cost:
                    cur = cost[i0, j] - u[i0] - v[j]
                    if minv[j] is None or cur < minv[j]:
                        minv[j] = cur
                        way[j] = j0
                if minv[j] is not None and (delta is None or minv[j] < delta):
                    delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                elif minv[j] is not None:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        length = 0
        while True:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            length += 1
            if j0 == 0:
                break
        if log is not None:
            log.append(('path', i, length, steps))
    return p


def step(st, o, p, log=None):
    """One frame of one stream: the state `st` is advanced in place; returns the frame's output rows."""
    boxes, scores, kps = _arrays(o)
    n, T = len(scores), len(st.id)
    det = np.concatenate([boxes, scores[:, None], kps.reshape(n, 3 * K)], axis=1).astype(np.float32) if n else np.zeros((0, DATA), np.float32)
    live = [t for t in range(T) if st.id[t] != 0]
    thr = np.float64(np.float32(p.match_threshold))
    sim, cost = {}, {}
    for t in live:
        for d in range(n):
            if p.similarity == 'iou':
                sim[t, d] = np.float64(iou(st.data[t, :4], det[d, :4]))
            else:
                sim[t, d] = oks(st.data[t, 5:].reshape(K, 3), det[d, 5:].reshape(K, 3))
            if log is not None:
                log.append(('threshold', float(sim[t, d]), float(thr), False))
            if not sim[t, d] >= thr:                                    # (a NaN is never eligible)
                continue
            cost[d + 1, t + 1] = -(quantum(sim[t, d]) + 1)
            if log is not None:
                scaled = float(sim[t, d]) * QUANTA
                exact = sim[t, d] == 1.0 and st.data[t, 5:].tobytes() == det[d, 5:].tobytes()
                log.append(('quantum', scaled, abs(scaled - round(scaled)), exact))
    for d in range(n):
        cost[d + 1, T + d + 1] = 0
    # 1. the optimal assignment
    on = assign(cost, n, T, log)
    det_of = {j - 1: on[j] - 1 for j in range(1, T + 1) if on[j] != 0}
    track_of = {d: t for t, d in det_of.items()}
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


def undecided(log, margin=1e-9, quantum_margin=1e-6):
    """The logged decisions a last-bit difference in a similarity could flip: a threshold comparison not apart by a relative
    `margin`, and a quantum closer than `quantum_margin` to an integer (a few ulp of a similarity near 1, scaled by 2^20, are
    about 1e-10) unless the similarity is exactly 1.0 for byte-identical keypoints."""
    bad = []
    for entry in log:
        if entry[0] == 'threshold':
            _, a, b, _ = entry
            if not abs(a - b) > margin * max(abs(a), abs(b)):
                bad.append(entry)
        elif entry[0] == 'quantum':
            _, _, distance, exact = entry
            if not exact and not distance > quantum_margin:
                bad.append(entry)
    return bad


def longest_path(log):
    """The longest augmenting path that was flipped, in columns."""
    return max((e[2] for e in log if e[0] == 'path'), default=0)


def longest_search(log):
    """The most columns a row's search took into its tree before it reached a free one."""
    return max((e[3] for e in log if e[0] == 'path'), default=0)
