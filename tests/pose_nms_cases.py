"""The case table of mpn_pose_nms: one record of B = 8 images x max_boxes = 64 slots, one image per thing the kernel can get
wrong (the table in `images`' docstring), built from fixed seeds. tests/test_pose_nms_host.py asserts on the CPU, with the
reference alone, that every image shows what it is there for and that no decision is within 1e-9 of flipping;
tests/test_pose_nms_gpu.py holds the kernel to the reference on it."""
import numpy as np

import pose_nms_ref as ref

B, MAX_BOXES = 8, 64
THRESHOLD = 0.7
MIN_KEYPOINT_SCORES = (0.0, 0.5)         # below every keypoint score of the table / between image 5's low and high scores
K = 17

# a standing person about 90 x 200 pixels: (x, y) of COCO's 17 joints
_POSE = np.array([[45, 10], [50, 5], [40, 5], [58, 8], [32, 8], [70, 40], [20, 40], [82, 80], [8, 80], [88, 118], [2, 118],
                  [62, 110], [28, 110], [64, 155], [26, 155], [66, 200], [24, 200]], np.float32)


def _person(x, y, score, kscore=0.9, scale=1.0, jitter=None):
    """(keypoints [17,3], box score): the pose at (x, y), every joint scored kscore (a number or 17 of them)."""
    kp = np.zeros((K, 3), np.float32)
    kp[:, :2] = _POSE * np.float32(scale) + np.array([x, y], np.float32)
    if jitter is not None:
        kp[:, :2] += jitter.astype(np.float32)
    kp[:, 2] = kscore
    return kp, np.float32(score)


def images():
    """Image -> list of (keypoints, score) in record order.

    0  no persons
    1  one person
    2  64 copies of one pose, jittered by at most half a pixel (a sigma is 7 pixels and more): one is kept and absorbed 63
    3  a chain A, B, C along x: A suppresses B; B's similarity with C is above the threshold, A's is below: C is kept
    4  64 persons on a grid of 20 pixels, each too far from the next to suppress it and none so far that a similarity
       underflows to 0: nothing is suppressed, all 2016 pairs are computed and every one shows in the matrix
    5  three near-duplicate pairs whose second person scores every joint / all but one / no joint below 0.5: with
       min_keypoint_score 0.5 the pairs have m = 0, 1 and 17 counting joints (with 0.0 all have 17)
    6  a near-duplicate pair whose box scores and keypoint scores order it the other way round: score mode 0 keeps the
       first, mode 1 the second; a third person apart
    7  three byte-identical rows with equal scores (record order decides) and one person apart"""
    rs = np.random.RandomState(7)
    out = [[], [_person(100, 50, 0.8)]]
    out.append([_person(200, 100, 0.95 - 0.01 * i, 0.9 - 0.005 * ((i * 7) % 64), jitter=rs.uniform(-0.5, 0.5, (K, 2))) for i in range(64)])
    out[2][0], out[2][40] = out[2][40], out[2][0]                   # the best score is not the first row
    out.append([_person(100 + 8 * i, 100, 0.9 - 0.1 * i, 0.8 + 0.01 * i) for i in range(3)])
    out.append([_person(10 + 20 * (i % 8), 10 + 20 * (i // 8), 0.3 + 0.01 * ((i * 37) % 64), 0.6 + 0.004 * i) for i in range(64)])
    low, high = np.float32(0.1), np.float32(0.9)
    one = np.full(K, low, np.float32)
    one[3] = high
    out.append([_person(50, 50, 0.90), _person(51, 50.5, 0.85, low),
                _person(250, 50, 0.80), _person(251, 50.5, 0.75, one),
                _person(450, 50, 0.70), _person(451, 50.5, 0.65, high)])
    out.append([_person(100, 100, 0.9, 0.55), _person(101, 100.5, 0.6, 0.95), _person(400, 100, 0.5, 0.6)])
    same = _person(300, 200, 0.5, 0.7)
    out.append([same, _person(50, 20, 0.45, 0.6), same, same])
    assert len(out) == B
    return out


def pack(imgs, b=B, max_boxes=MAX_BOXES, overflow=0):
    """The images -> a record of mpn_pose_gather's layout (uint8). num_boxes[i] = counts[i] + 1 + i: it differs from the
    counts and must be copied through; image_index, box and keypoint_positions are filled with distinct values, the box of a
    person from its keypoints (so that byte-identical persons have byte-identical rows)."""
    assert len(imgs) == b
    record = np.zeros(ref.record_bytes(b, max_boxes), np.uint8)
    hw = ref.header_words(b)
    header = record[:hw * 4].view(np.int32)
    rows = record[hw * 4:].view(np.float32).reshape(b * max_boxes, ref.ROW_WORDS)
    at = 0
    for i, persons in enumerate(imgs):
        assert len(persons) <= max_boxes
        for kp, score in persons:
            row = rows[at]
            row[:1].view(np.int32)[0] = i
            row[1:5] = (kp[:, 1].min() / 640, kp[:, 0].min() / 640, kp[:, 1].max() / 640, kp[:, 0].max() / 640)
            row[ref.OFF_SCORE] = score
            row[ref.OFF_KSCORE:ref.OFF_KSCORE + K] = kp[:, 2]
            row[ref.OFF_KSCORE + K:ref.OFF_KEYPOINTS] = ((kp[:, 1::-1] - kp[:, 1::-1].min(0)) / np.ptp(kp[:, 1::-1], axis=0)).reshape(-1)
            row[ref.OFF_KEYPOINTS:] = kp.reshape(-1)
            at += 1
        header[1 + i] = len(persons)
        header[1 + b + i] = len(persons) + 1 + i
    header[0] = at
    header[1 + 2 * b] = overflow
    return record


def table(overflow=0):
    return pack(images(), overflow=overflow)


def large():
    """The one-block limit: B = 64 images (the table's, eight times over) x 64 slots = 4096 rows, 1160 of them filled."""
    return pack(images() * 8, b=64)


def nan_scores():
    """Beyond the table, at B = 2, max_boxes = 4: persons apart from each other whose box scores are NaN, 0.5, NaN, 0.7 (a
    NaN sorts behind every number, in record order), and a near-duplicate pair where the NaN-scored one comes first in the
    record and must be the one suppressed."""
    nan = np.float32(np.nan)
    return [[_person(10, 10, nan, scale=0.25), _person(110, 10, 0.5, scale=0.25), _person(210, 10, nan, scale=0.25),
             _person(310, 10, 0.7, scale=0.25)],
            [_person(100, 100, nan), _person(101, 100.5, 0.2)]]
