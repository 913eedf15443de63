"""Seeded detections and ground truth for the keypoint-AP tests (shared by the host and the GPU tests, built once).

Persons live in clusters on a coarse grid of a large pixel plane: inside a cluster the OKS values are generic, between
clusters every term exp(-e) underflows to exactly 0 on any IEEE implementation (e > 745), so such OKS are bit-equal zeros.
`make_cases` redraws an image until, in the reference, every OKS is at least MARGIN away from every threshold and from
every other OKS of the same detection that is not bit-equal to it - so that a 1e-16 relative difference in exp cannot
change a single matching decision, and equality of every match is a fair demand."""
import numpy as np

import pose_eval_ref as ref

MARGIN = 1e-9
B, MAX_BOXES, MAX_GT = 5, 25, 64
PITCH = 8000.0                                        # cluster spacing: e > (PITCH/2)^2 / (2 * 40000 * 0.0458) = 4366 > 745


def _person(rng, cx, cy, side):
    """A pose in a side x side box at (cx, cy): keypoints (x, y, v) float64 [17,3] with all v = 2, bbox (x, y, w, h)."""
    x = cx + rng.uniform(0, side, 17)
    y = cy + rng.uniform(0, side, 17)
    return np.stack([x, y, np.full(17, 2.0)], 1), np.array([cx, cy, side, side])


def _detection(rng, kp, area, e_target):
    """Keypoints f32 [17,3] around a ground-truth pose, the per-keypoint error term about e_target."""
    d = np.sqrt(area * e_target) * 2 * ref.SIGMAS[:, None] * rng.normal(0, 1, (17, 2))
    out = np.zeros((17, 3), np.float32)
    out[:, :2] = (kp[:, :2] + d).astype(np.float32)
    out[:, 2] = rng.uniform(0.1, 1.0, 17)
    return out


def _det_dict(rng, kps, scores=None):
    n = len(kps)
    kps = np.array(kps, np.float32).reshape(n, 17, 3)
    scores = rng.uniform(0.06, 1.0, n).astype(np.float32) if scores is None else np.asarray(scores, np.float32)
    return {'boxes': rng.uniform(0, 1, (n, 4)).astype(np.float32), 'scores': scores, 'num_boxes': np.int32(n),
            'keypoint_scores': np.ascontiguousarray(kps[:, :, 2]), 'keypoint_positions': rng.uniform(0, 1, (n, 17, 2)).astype(np.float32),
            'keypoints': kps}


def _gt_dict(kps, boxes, areas, crowd):
    g = len(kps)
    return {'keypoints': np.array(kps, np.float64).reshape(g, 17, 3), 'boxes': np.array(boxes, np.float64).reshape(g, 4),
            'area': np.array(areas, np.float64).reshape(g), 'iscrowd': np.array(crowd, np.int32).reshape(g)}


def _image(kind, rng):
    if kind == 0:                                     # no detections, 2 ground-truth persons
        ps = [_person(rng, 100.0 + 300 * i, 50.0, 120.0) for i in range(2)]
        return _det_dict(rng, []), _gt_dict([p[0] for p in ps], [p[1] for p in ps], [9000.0, 1500.0], [0, 0])
    if kind == 1:                                     # 25 detections on 1 person: 5 of them past max_dets
        kp, box = _person(rng, 200.0, 100.0, 150.0)
        dets = [_detection(rng, kp, 12000.0, rng.uniform(0.01, 1.5)) for _ in range(25)]
        return _det_dict(rng, dets), _gt_dict([kp], [box], [12000.0], [0])
    if kind == 2:                                     # detections, no ground truth (areas on both sides of 32^2 and 96^2)
        dets = [_detection(rng, _person(rng, 50.0, 50.0, s)[0], s * s, 0.1) for s in (10.0, 20.0, 60.0, 80.0, 150.0, 200.0, 400.0)]
        return _det_dict(rng, dets), _gt_dict([], [], [], [])
    if kind == 3:                                     # 64 persons in 16 clusters of 4: plain, partly visible, crowd, k1 == 0
        kps, boxes, areas, crowd, dets = [], [], [], [], []
        for c in range(16):
            cx, cy = PITCH * (c % 4) + 500.0, PITCH * (c // 4) + 500.0
            side = float(rng.choice([25.0, 60.0, 110.0, 190.0]))
            base, box = _person(rng, cx, cy, side)
            area = side * side * rng.uniform(0.5, 1.0)
            for j in range(4):
                kp = base.copy()
                kp[:, :2] += rng.normal(0, 0.03 * side, (17, 2))
                if j == 1:
                    kp[:, 2] = rng.integers(0, 3, 17)
                    kp[0, 2] = 1.0
                if j == 3:
                    kp[:, 2] = 0.0
                kps.append(kp); boxes.append(box + rng.normal(0, 1.0, 4)); crowd.append(1 if j == 2 else 0)
                areas.append(area * rng.uniform(0.8, 1.2))
            if len(dets) < 25:
                for _ in range(2 if c < 9 else 1):
                    dets.append(_detection(rng, base, area, rng.uniform(0.01, 1.0)))
        order = rng.permutation(64)                   # ignored and crowd rows anywhere in the image's own order
        gt = _gt_dict([kps[i] for i in order], [boxes[i] for i in order], [areas[i] for i in order], [crowd[i] for i in order])
        return _det_dict(rng, dets[:25]), gt
    # kind 4: two bit-identical ground-truth rows (+ a third person), detections with equal scores
    kp, box = _person(rng, 300.0, 200.0, 100.0)
    kp2, box2 = _person(rng, 320.0, 210.0, 100.0)
    dets = [_detection(rng, kp, 5000.0, e) for e in (0.02, 0.05, 0.2, 0.4)] + [_detection(rng, kp2, 5000.0, 0.1)]
    det = _det_dict(rng, dets, scores=[0.5, 0.5, 0.5, 0.25, 0.5])
    det['keypoint_scores'][1] = det['keypoint_scores'][0]          # equal in both score modes
    det['keypoint_scores'][2] = det['keypoint_scores'][0]
    det['keypoints'][1:3, :, 2] = det['keypoints'][0, :, 2]
    return det, _gt_dict([kp, kp, kp2], [box, box, box2], [5000.0, 5000.0, 5000.0], [0, 0, 0])


def margins_hold(table):
    """The generator's acceptance rule on one image's reference result."""
    for row, rank in zip(table['oks'], table['rank']):
        if rank >= ref.MAX_DETS:
            continue
        if len(row) and np.min(np.abs(row[:, None] - ref.IOU_THRS[None, :])) < MARGIN:
            return False
        gap = np.abs(row[:, None] - row[None, :])
        if np.any((gap < MARGIN) & (row[:, None] != row[None, :])):
            return False
    return True


def make_cases(seed=2024, tries=50):
    """(detections, ground truth, {score_mode: [reference result per image]}) of the five images; asserts the margins."""
    dets, gts = [], []
    for kind in range(B):
        for attempt in range(tries):
            det, gt = _image(kind, np.random.default_rng([seed, kind, attempt]))
            if all(margins_hold(ref.evaluate_image(det, gt, mode)) for mode in (0, 1)):
                break
        else:
            raise AssertionError(f"image {kind}: no draw in {tries} keeps every OKS {MARGIN} from the thresholds and its neighbours")
        dets.append(det); gts.append(gt)
    want = {mode: [ref.evaluate_image(d, g, mode) for d, g in zip(dets, gts)] for mode in (0, 1)}
    for tables in want.values():
        assert all(margins_hold(t) for t in tables)
    return dets, gts, want


_cache = {}


def cases():
    """make_cases(), computed once per process and shared (read-only by convention)."""
    if 'c' not in _cache:
        _cache['c'] = make_cases()
    return _cache['c']
