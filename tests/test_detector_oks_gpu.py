"""GPU: `groundtruth=` of Detector.predict_batch / predict_images - mpn_oks_match inside the captured graph - against
OksMatcher on the returned dicts and against the COCOeval transcription (tests/pose_eval_ref.py). Image size, variables and
score threshold are those of tests/test_detector_batch_gpu.py."""
import numpy as np
import pytest

import pose_eval_ref as ref
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, models  # noqa: F401 (models: a fixture)

pytestmark = pytest.mark.gpu

TABLE_KEYS = ('rank', 'score', 'area', 'matches', 'ignore')


def _groundtruth(outs, sizes, frac, without=2):
    """Ground truth made from a call's own output: the first persons of every image, each keypoint moved by its own small
    multiple of frac * sqrt(box area) (the error term of OKS is then about frac^2 / (2 (2 sigma)^2) whatever the person's
    size), visibility mixed 0 / 1 / 2, the box in pixels; one crowd row (a copy of person 0); image `without` has no
    ground truth."""
    gts = []
    for i, (o, (h, w)) in enumerate(zip(outs, sizes)):
        n = 0 if i == without else min(len(o['keypoints']), 6)
        b = o['boxes'][:n].astype(np.float64)
        boxes = np.stack([b[:, 1] * w, b[:, 0] * h, (b[:, 3] - b[:, 1]) * w, (b[:, 2] - b[:, 0]) * h], 1)
        step = frac * np.sqrt(np.abs(boxes[:, 2] * boxes[:, 3]))[:, None]
        kp = o['keypoints'][:n].astype(np.float64)
        k = np.arange(17)
        kp[:, :, 0] += step * (1 + (k % 3)) * 0.5
        kp[:, :, 1] -= step * (1 + (k % 4)) * 0.25
        kp[:, :, 2] = (k + np.arange(n)[:, None]) % 3
        crowd = np.zeros(n, np.int32)
        if n:
            kp, boxes, crowd = np.concatenate([kp, kp[:1]]), np.concatenate([boxes, boxes[:1]]), np.append(crowd, 1)
        gts.append({'keypoints': kp, 'boxes': boxes, 'iscrowd': crowd})
    return gts


def _check_tables(outs, gts, matcher_tables, msg):
    for i, (o, g, m) in enumerate(zip(outs, gts, matcher_tables)):
        want = ref.evaluate_image(o, g)
        for k in TABLE_KEYS:
            assert np.asarray(o['oks'][k]).dtype == np.asarray(m[k]).dtype
            np.testing.assert_array_equal(o['oks'][k], m[k], err_msg=f"{msg} image {i} {k}: graph vs OksMatcher")
            np.testing.assert_array_equal(o['oks'][k], want[k], err_msg=f"{msg} image {i} {k}: graph vs reference")


def _stats(outs, gts):
    from multiposenet_amd.pose_metrics import PoseEvaluator
    ev = PoseEvaluator()
    ev.update(outs, gts)
    return ev.evaluate()


def test_predict_batch_with_groundtruth(cuda, models):
    from multiposenet_amd.pose_metrics import OksMatcher
    det = _detector(models)
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.0)
    n0 = len(det._graphs)
    sizes = [(H, W)] * len(images)
    gts = _groundtruth(plain, sizes, 0.01)
    assert sum(len(g['keypoints']) for g in gts) >= 12 and len(gts[2]['keypoints']) == 0
    outs = det.predict_batch(images, score_threshold=0.0, groundtruth=gts)
    assert len(det._graphs) == n0 + 1
    for a, b in zip(plain, outs):
        assert set(b) == set(a) | {'oks'}
        _assert_same(a, {k: v for k, v in b.items() if k != 'oks'}, "groundtruth=:")
    matcher = OksMatcher(len(images), det.params['max_boxes'])
    _check_tables(outs, gts, matcher(plain, gts), "first call")
    matched = sum(int((o['oks']['matches'][:, 0, 0] >= 0).sum()) for o in outs)
    assert matched >= 8                                              # a hundredth of the person's size off: they match at OKS .5
    # other ground truth: the same graph follows it
    gts2 = _groundtruth(plain, sizes, 0.04, without=0)
    outs2 = det.predict_batch(images, score_threshold=0.0, groundtruth=gts2)
    assert len(det._graphs) == n0 + 1
    _check_tables(outs2, gts2, matcher(plain, gts2), "second call")
    assert any(not np.array_equal(a['oks']['matches'], b['oks']['matches']) for a, b in zip(outs, outs2))
    # the evaluator fed from 'oks' and from the plain dicts
    stats = _stats(outs, gts)
    assert stats == _stats(plain, gts) == ref.evaluate(plain, gts)
    assert 0.0 < stats['AP'] <= 1.0 and _stats(outs2, gts2) == ref.evaluate(plain, gts2)
    # without groundtruth nothing changed: the first graph, the same dicts
    for a, b in zip(plain, det.predict_batch(images, score_threshold=0.0)):
        _assert_same(a, b, "after groundtruth=:")
    assert len(det._graphs) == n0 + 1
    with pytest.raises(ValueError, match="groundtruth"):
        det.predict_batch(images, score_threshold=0.0, groundtruth=gts[:2])
    crowded = [dict(g) for g in gts]
    crowded[1] = {'keypoints': np.zeros((65, 17, 3)), 'boxes': np.ones((65, 4))}
    with pytest.raises(ValueError, match="65 persons"):
        det.predict_batch(images, score_threshold=0.0, groundtruth=crowded)


def test_predict_images_with_groundtruth_in_source_pixels(cuda, models):
    """Two frame sizes: the network's own (the resize is the identity) and twice that (each pixel doubled)."""
    from multiposenet_amd.pose_metrics import OksMatcher
    det = _detector(models)
    images = _images()
    frames = [images[0], np.repeat(np.repeat(images[1], 2, axis=0), 2, axis=1), images[2]]
    sizes = [f.shape[:2] for f in frames]
    plain = det.predict_images(frames, size=(H, W), score_threshold=0.0)
    assert len(plain[0]['boxes']) >= 3 and sizes[1] == (2 * H, 2 * W)
    gts = _groundtruth(plain, sizes, 0.01)
    n0 = len(det._graphs)
    outs = det.predict_images(frames, size=(H, W), score_threshold=0.0, groundtruth=gts)
    assert len(det._graphs) == n0 + 1
    for a, b in zip(plain, outs):
        assert set(b) == set(a) | {'oks'}
        _assert_same(a, {k: v for k, v in b.items() if k != 'oks'}, "predict_images groundtruth=:")
    matcher = OksMatcher(len(frames), det.params['max_boxes'])
    _check_tables(outs, gts, matcher(plain, gts), "predict_images")
    assert sum(int((o['oks']['matches'][:, 0, 0] >= 0).sum()) for o in outs) >= 3
    assert _stats(outs, gts) == ref.evaluate(plain, gts)
