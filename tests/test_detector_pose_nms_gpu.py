"""GPU: `pose_nms=` of Detector.predict_batch / predict_images - mpn_pose_nms behind the gather inside the captured graph,
every later launch reading the filtered record - against the plain-loop reference (tests/pose_nms_ref.py) on the dicts a call
without it returns. Image size, variables and score threshold are those of tests/test_detector_batch_gpu.py.

The threshold is the test's choice from the data: the midpoint of the widest gap between neighbouring values of the sorted
similarities at which the reference suppresses somebody and keeps two persons in some image. The gap must be wider than 2e-6,
so that neither rounding the threshold to float32 (below 6e-8) nor the last bit of exp (below 1e-15) can move a decision."""
import numpy as np
import pytest

import pose_nms_ref as ref
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, models  # noqa: F401 (models: a fixture)
from test_detector_oks_gpu import _groundtruth

pytestmark = pytest.mark.gpu

PER_PERSON = ('boxes', 'scores', 'keypoint_scores', 'keypoint_positions', 'keypoints')
MIN_GAP = 2e-6


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _survivors(outs, threshold):
    return [ref.survivors(o['keypoints'], o['scores'], o['keypoint_scores'], threshold, 0.0, 0) for o in outs]


def _choose_threshold(outs):
    """The midpoint of the widest gap between neighbouring similarities of the calls' persons at which the reference
    suppresses at least one person and keeps at least two in some image; the gap is wider than MIN_GAP."""
    values = {0.0, 1.0}
    for _, _, sim in _survivors(outs, 1.0):
        values.update(sim[p][q] for p in range(len(sim)) for q in range(p))
    values = np.array(sorted(values))
    gaps = np.diff(values)
    for at in np.argsort(-gaps, kind='stable'):
        if not gaps[at] > MIN_GAP:
            break
        threshold = float(np.float32((values[at] + values[at + 1]) / 2))
        if not values[at] + MIN_GAP / 2 < threshold < values[at + 1] - MIN_GAP / 2:
            continue
        if any(len(kept) >= 2 and len(kept) < len(o['scores']) for o, (kept, _, _) in zip(outs, _survivors(outs, threshold))):
            return threshold
    raise AssertionError("no gap between the similarities is wide enough for a threshold that suppresses and keeps")


def _expected(outs, threshold):
    want = []
    for o, (kept, absorbed, _) in zip(outs, _survivors(outs, threshold)):
        w = dict(o)
        for k in PER_PERSON:
            w[k] = np.ascontiguousarray(o[k][kept])
        w.update({'pose_nms_source': np.array(kept, np.int32), 'pose_nms_absorbed': np.array([absorbed[p] for p in kept], np.int32),
                  'pose_nms_suppressed': np.int32(len(o['scores']) - len(kept))})
        want.append(w)
    return want


def _nms(threshold):
    from multiposenet_amd.inference import PoseNms
    nms = PoseNms(threshold)
    assert nms.threshold == threshold                               # already a float32 value
    return nms


def test_batch_returns_the_reference_survivors(det, models):
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.0)
    threshold = _choose_threshold(plain)
    want = _expected(plain, threshold)
    assert any(w['pose_nms_suppressed'] >= 1 and len(w['scores']) >= 2 for w in want)
    n0 = len(det._graphs)
    first = det.predict_batch(images, score_threshold=0.0, pose_nms=_nms(threshold))
    assert len(det._graphs) == n0 + 1
    for w, o in zip(want, first):
        _assert_same(w, o, "pose_nms=:")
        assert type(o['pose_nms_suppressed']) is np.int32 and o['num_boxes'] >= len(o['scores']) + o['pose_nms_suppressed']
    again = det.predict_batch(images, score_threshold=0.0, pose_nms=_nms(threshold))       # an equal PoseNms: the same entry
    assert len(det._graphs) == n0 + 1
    for w, o in zip(want, again):
        _assert_same(w, o, "pose_nms= replayed:")
    for a, o in zip(plain, det.predict_batch(images, score_threshold=0.0)):
        _assert_same(a, o, "after pose_nms=:")
    assert len(det._graphs) == n0 + 1
    # the eager path gives the same
    eager = _detector(models, graph=False)
    for w, o in zip(want, eager.predict_batch(images, score_threshold=0.0, pose_nms=_nms(threshold))):
        _assert_same(w, o, "pose_nms= eager:")
    assert not eager._graphs


def test_predict_images_on_ragged_frames(det):
    images = _images()
    frames = [images[0], np.repeat(np.repeat(images[1], 2, axis=0), 2, axis=1), images[2][:200, :300]]
    plain = det.predict_images(frames, size=(H, W), score_threshold=0.0)
    threshold = _choose_threshold(plain)
    want = _expected(plain, threshold)
    n0 = len(det._graphs)
    for c in range(2):
        got = det.predict_images(frames, size=(H, W), score_threshold=0.0, pose_nms=_nms(threshold))
        assert len(det._graphs) == n0 + 1
        for w, o in zip(want, got):
            _assert_same(w, o, f"predict_images pose_nms= call {c}:")
    for a, o in zip(plain, det.predict_images(frames, size=(H, W), score_threshold=0.0)):
        _assert_same(a, o, "predict_images after pose_nms=:")
    assert len(det._graphs) == n0 + 1


def test_every_later_launch_reads_the_filtered_record(det):
    """groundtruth=, track= and annotate=True in the same call: each result is what its stage gives on the filtered dicts."""
    from multiposenet_amd import pose_metrics as pm
    from multiposenet_amd.inference import PoseTracker, draw_everything
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.0)
    threshold = _choose_threshold(plain)
    want = _expected(plain, threshold)
    gts = _groundtruth(plain, [(H, W)] * len(images), 0.01)
    in_graph, on_host = PoseTracker(streams=4), PoseTracker(streams=4)
    matcher = pm.OksMatcher(len(images), det.params['max_boxes'])
    extra = ('oks', 'annotated', 'track_ids', 'track_hits', 'track_new', 'track_similarity')
    for c in range(2):
        outs = det.predict_batch(images, score_threshold=0.0, groundtruth=gts, track=in_graph, annotate=True,
                                 pose_nms=_nms(threshold))
        filtered = [{k: v for k, v in o.items() if k not in extra} for o in outs]
        for w, f in zip(want, filtered):
            _assert_same(w, f, f"call {c}:")
        for o, table in zip(outs, matcher(filtered, gts)):
            assert set(o['oks']) == set(table)
            for k in table:
                np.testing.assert_array_equal(o['oks'][k], table[k], err_msg=f"call {c} oks {k}")
        for o, rows in zip(outs, on_host.update(filtered)):
            for k in rows:
                np.testing.assert_array_equal(o[k], rows[k], err_msg=f"call {c} {k}")
            assert (o['track_hits'] == c + 1).all() and len(o['track_ids']) == len(o['scores'])
        for im, o, f in zip(images, outs, filtered):
            np.testing.assert_array_equal(o['annotated'], draw_everything(im, f), err_msg=f"call {c} annotated")
    # the unfiltered persons would have drawn something else on an image that lost a person
    lost = [i for i, w in enumerate(want) if w['pose_nms_suppressed'] > 0]
    assert lost and any(not np.array_equal(outs[i]['annotated'], draw_everything(images[i], plain[i])) for i in lost)
