"""The definition of mpn_pose_nms (include/mpn.h) as plain loops over a record's bytes: Python floats (IEEE float64) and
math.exp, numpy float32 scalars where the header names f32, one operation per line in the documented order. Test
infrastructure only; it shares no code with multiposenet_amd - the record's layout is restated here.

    record_out, info, sim = run(record, b, max_boxes, threshold, min_keypoint_score, score_mode)
    kept = survivors(kp, scores, kscores, threshold, min_keypoint_score, score_mode)[0]     # one image's arrays

`run(..., log=[])` appends (similarity, threshold) for every comparison the suppression makes; `undecided(log)` lists those a
last-bit difference in exp could flip. A similarity is a mean of at most 17 values in (0, 1], each <= 1 exactly, so it never
exceeds 1: against a threshold of 1 (or more) no comparison can come out true whatever the last bit, and none is listed."""
import math

import numpy as np

K = 17
ROW_WORDS = 108                          # int32 image_index, f32 box[4], score, keypoint_scores[17], positions[17][2], keypoints[17][3]
OFF_SCORE, OFF_KSCORE, OFF_KEYPOINTS = 5, 6, 57
SIGMAS = [.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]
VARS = [(s / 10.0 * 2) * (s / 10.0 * 2) for s in SIGMAS]           # cocoeval.py: vars = (sigmas * 2)**2
EPS = 2.0 ** -52


def header_words(b):
    return (2 * b + 2 + 3) // 4 * 4


def record_bytes(b, max_boxes):
    return (header_words(b) + b * max_boxes * ROW_WORDS) * 4


def info_head_bytes(b):
    return (4 * b + 15) // 16 * 16


def info_bytes(b, max_boxes):
    return info_head_bytes(b) + b * max_boxes * 16


def order_score(score, kscores, score_mode):
    """float32 throughout."""
    if score_mode == 0:
        return np.float32(score)
    m = np.float32(0)
    for k in range(K):
        m = np.float32(m + np.float32(kscores[k]))
    m = np.float32(m / np.float32(17))
    return np.float32(np.float32(score) * m)


def visited_before(sj, j, si, i):
    """Descending order score, equal scores in record order, NaN behind every number (in record order)."""
    if math.isnan(sj):
        return math.isnan(si) and j < i
    if math.isnan(si):
        return True
    return sj > si or (sj == si and j < i)


def extent_area(kp):
    """keypoints float32 [17,3]: min / max in float32, the differences and the product in float64."""
    xl = xh = np.float32(kp[0, 0])
    yl = yh = np.float32(kp[0, 1])
    for k in range(1, K):
        x, y = np.float32(kp[k, 0]), np.float32(kp[k, 1])
        xl, xh = (x if x < xl else xl), (x if x > xh else xh)
        yl, yh = (y if y < yl else yl), (y if y > yh else yh)
    return (float(xh) - float(xl)) * (float(yh) - float(yl))


def similarity(kp_p, kp_q, area_p, area_q, min_keypoint_score):
    mks = np.float32(min_keypoint_score)
    counting = [k for k in range(K) if np.float32(kp_p[k, 2]) >= mks and np.float32(kp_q[k, 2]) >= mks]
    m = len(counting)
    if m == 0:
        return 0.0
    denom = (area_p + area_q) / 2 + EPS
    total = 0.0
    for k in counting:
        dx = float(kp_q[k, 0]) - float(kp_p[k, 0])
        dy = float(kp_q[k, 1]) - float(kp_p[k, 1])
        e = (dx * dx + dy * dy) / VARS[k] / denom / 2
        total += math.exp(-e)
    return total / m


def survivors(kp, scores, kscores, threshold, min_keypoint_score, score_mode, log=None):
    """One image: keypoints f32 [n,17,3], box scores f32 [n], keypoint_scores f32 [n,17] -> (kept indices in record order,
    absorbed per person [n], similarity [n][n])."""
    n = len(scores)
    thr = float(np.float32(threshold))
    s = [float(order_score(scores[p], kscores[p], score_mode)) for p in range(n)]
    area = [extent_area(kp[p]) for p in range(n)]
    sim = [[0.0] * n for _ in range(n)]
    for p in range(n):
        for q in range(p + 1, n):
            sim[p][q] = sim[q][p] = similarity(kp[p], kp[q], area[p], area[q], min_keypoint_score)
    order = [None] * n
    for i in range(n):
        order[sum(1 for j in range(n) if j != i and visited_before(s[j], j, s[i], i))] = i
    suppressed, kept, absorbed = set(), [], [0] * n
    for r, p in enumerate(order):
        if p in suppressed:
            continue
        kept.append(p)
        for q in order[r + 1:]:
            if q in suppressed:
                continue
            if log is not None:
                log.append((sim[p][q], thr))
            if sim[p][q] > thr:
                suppressed.add(q)
                absorbed[p] += 1
    return sorted(kept), absorbed, sim


def run(record, b, max_boxes, threshold, min_keypoint_score, score_mode, log=None):
    """record: uint8 array of record_bytes(b, max_boxes) -> (record_out uint8, info uint8, sim f64 [b, max_boxes, max_boxes])."""
    record = np.frombuffer(np.ascontiguousarray(record).tobytes(), np.uint8)
    hw = header_words(b)
    header = record[:hw * 4].view(np.int32)
    rows = record[hw * 4:].view(np.uint32).reshape(b * max_boxes, ROW_WORDS)
    out = np.zeros(record_bytes(b, max_boxes), np.uint8)
    out_header = out[:hw * 4].view(np.int32)
    out_rows = out[hw * 4:].view(np.uint32).reshape(b * max_boxes, ROW_WORDS)
    info = np.zeros(info_bytes(b, max_boxes), np.uint8)
    head = info_head_bytes(b)
    info_suppressed = info[:4 * b].view(np.int32)
    info_rows = info[head:head + 8 * b * max_boxes].view(np.int32).reshape(b * max_boxes, 2)
    work = info[head + 8 * b * max_boxes:].view(np.int32).reshape(b, max_boxes, 2)
    sim_out = np.zeros((b, max_boxes, max_boxes), np.float64)
    first = at = 0
    for i in range(b):
        n = min(max(int(header[1 + i]), 0), max_boxes)
        mine = rows[first:first + n]
        f = mine.view(np.float32)
        kept, absorbed, sim = survivors(f[:, OFF_KEYPOINTS:].reshape(n, K, 3), f[:, OFF_SCORE], f[:, OFF_KSCORE:OFF_KSCORE + K],
                                        threshold, min_keypoint_score, score_mode, log)
        for p in kept:
            out_rows[at] = mine[p]
            info_rows[at] = (p, absorbed[p])
            work[i, p] = (1, absorbed[p])
            at += 1
        out_header[1 + i] = len(kept)
        info_suppressed[i] = n - len(kept)
        if n:
            sim_out[i, :n, :n] = np.array(sim, np.float64).reshape(n, n)
        first += n
    out_header[0] = at
    out_header[1 + b:2 + 2 * b] = header[1 + b:2 + 2 * b]          # num_boxes[b] and the overflow word
    return out, info, sim_out


def undecided(log, margin=1e-9):
    """The logged comparisons closer than `margin` to their threshold (below a threshold of 1: see the module's docstring)."""
    return [(s, thr) for s, thr in log if thr < 1.0 and not abs(s - thr) >= margin]
