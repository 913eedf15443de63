"""Deterministic INPUTS of the detector-metric golden cases (seeded numpy Generator).

Shared by `make_metrics_goldens.py` (which runs the reference's `Evaluator` on them and stores only the seven numbers it
returns in `metrics_goldens.npz`) and by tests/test_metrics_oracle.py. A case is
(name, images, iou_threshold): images is a list, in the order they are added, of
(groundtruth boxes f32 [n,4], detected boxes f32 [m,4], scores f32 [m]) with boxes as (ymin, xmin, ymax, xmax).
"""
import numpy as np

F = np.float32


def _boxes(rng, n, lo=0.05, hi=0.4):
    size = rng.uniform(lo, hi, (n, 2))
    start = rng.uniform(0, 1, (n, 2)) * (1 - size)
    return np.concatenate([start, start + size], 1).astype(F)


def _none(k=0):
    return np.zeros((k, 4), F)


def _random_image(rng, max_gt=6, max_extra=5):
    """Ground truth, and detections that are noisy copies of some of it plus unrelated boxes."""
    gt = _boxes(rng, int(rng.integers(0, max_gt + 1)))
    hit = gt[rng.random(len(gt)) < 0.8]
    hit = hit[rng.integers(0, len(hit), int(rng.integers(0, len(hit) + 3)))] if len(hit) else hit    # repeats allowed
    det = np.concatenate([(hit + rng.normal(0, 0.02, hit.shape)).astype(F), _boxes(rng, int(rng.integers(0, max_extra + 1)))])
    det = det[rng.permutation(len(det))][:25]
    scores = np.round(rng.uniform(0.3, 1.0, len(det)), 2).astype(F)            # two decimals: ties in confidence happen
    return gt, det, scores


def cases():
    """Yield (name, images, iou_threshold)."""
    rng = np.random.default_rng(11)
    gts = [_boxes(rng, n) for n in (3, 1, 5)]
    yield "perfect", [(g, g.copy(), rng.uniform(0.3, 1, len(g)).astype(F)) for g in gts], 0.5
    yield "no_detections", [(g, _none(), np.zeros(0, F)) for g in gts], 0.5
    yield "nothing_at_all", [], 0.5
    g = _boxes(rng, 2)
    dup = np.concatenate([g[:1]] * 4 + [g[1:]])
    dup = (dup + rng.normal(0, 0.01, dup.shape)).astype(F)
    yield "duplicates_on_one_groundtruth", [(g, dup, np.array([0.9, 0.8, 0.95, 0.6, 0.7], F))], 0.5
    g = _boxes(rng, 4)
    det = np.concatenate([g, _boxes(rng, 4)])[[4, 0, 5, 1, 6, 2, 7, 3]]
    yield "ties_in_confidence", [(g, det, np.array([0.5, 0.5, 0.5, 0.5, 0.75, 0.75, 0.5, 0.75], F)),
                                 (g[:2], det[:3], np.array([0.5, 0.75, 0.5], F))], 0.5
    yield "detections_without_groundtruth", [(_none(), _boxes(rng, 3), np.array([0.9, 0.4, 0.6], F)),
                                             (gts[0], gts[0][:2].copy(), np.array([0.8, 0.5], F))], 0.5
    # IoU exactly at the threshold: [0,0,1,1] against [0,0,1,0.5] is 0.5, against [0,0,0.5,0.5] is 0.25 (exact in binary)
    unit = np.array([[0, 0, 1, 1]], F)
    yield "iou_equal_to_threshold", [(unit, np.array([[0, 0, 1, 0.5]], F), np.array([0.9], F))], 0.5
    yield "iou_just_below_threshold", [(unit, np.array([[0, 0, 0.5, 0.5]], F), np.array([0.9], F))], 0.5
    yield "iou_equal_to_quarter_threshold", [(unit, np.array([[0, 0, 0.5, 0.5]], F), np.array([0.9], F))], 0.25
    yield "degenerate_boxes", [(np.array([[0.2, 0.2, 0.2, 0.6], [0.1, 0.1, 0.5, 0.5]], F),
                                np.array([[0.2, 0.2, 0.2, 0.6], [0.5, 0.5, 0.9, 0.9], [0.1, 0.1, 0.5, 0.5]], F),
                                np.array([0.9, 0.8, 0.7], F))], 0.5
    rng = np.random.default_rng(12)
    images = [_random_image(rng) for _ in range(200)]
    yield "random_200_images", images, 0.5
    yield "random_200_images_iou75", images, 0.75
    yield "random_40_images_float64", [(g.astype(np.float64), d.astype(np.float64), s.astype(np.float64))
                                      for g, d, s in images[:40]], 0.5
