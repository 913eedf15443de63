"""GPU: `track_eval=` of Detector.predict_batch / predict_images - mpn_track_eval behind the tracker's launch inside the captured
graph, the evaluator's state advanced once per call outside it. Image size, variables and score threshold are those of
tests/test_detector_batch_gpu.py; the ground truth is made of the frames' own detections."""
import json

import numpy as np
import pytest

import track_eval_ref as ref
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, models  # noqa: F401 (models: a fixture)

pytestmark = pytest.mark.gpu

MAX_TRACKS = 32


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


@pytest.fixture(scope="module")
def plain(det):
    return det.predict_batch(_images(), score_threshold=0.0)


def _pair(streams, det):
    from multiposenet_amd.inference import PoseTracker, TrackEvaluator
    return (PoseTracker(streams=streams, max_tracks=MAX_TRACKS, new_track_score=0.0),
            TrackEvaluator(streams=streams, max_boxes=det.params['max_boxes']))


def _groundtruth(outs, h=H, w=W, swap=None):
    """Every image's own persons as its annotated persons, in a permuted order, with the ids 100 + the person's index (swap:
    (image, p, q) - the ids of persons p and q of that image exchanged)."""
    gts = []
    for i, o in enumerate(outs):
        n = len(o['keypoints'])
        order = np.random.RandomState(40 + i).permutation(n)
        kp = o['keypoints'][order].astype(np.float64)
        kp[:, :, 2] = 2
        b = o['boxes'][order].astype(np.float64)
        ids = 100 + order
        if swap is not None and swap[0] == i:
            ids = np.where(ids == 100 + swap[1], 100 + swap[2], np.where(ids == 100 + swap[2], 100 + swap[1], ids))
        gts.append({'keypoints': kp, 'boxes': np.stack([b[:, 1] * w, b[:, 0] * h, (b[:, 3] - b[:, 1]) * w, (b[:, 2] - b[:, 0]) * h], 1),
                    'track_ids': ids})
    return gts


def test_own_detections_as_ground_truth(det, plain):
    """Three calls over four cameras: every person is matched in every frame, there is no switch, MOTA = IDF1 = 1; the first
    call - an eager pass and the replay - counts once; one graph for the key; everything else as without track_eval=."""
    images = _images()
    gts = _groundtruth(plain)
    tracker, evaluator = _pair(4, det)
    alone = _pair(4, det)[0]
    n0 = len(det._graphs)
    for call in range(3):
        outs = det.predict_batch(images, score_threshold=0.0, track=tracker, groundtruth=gts, track_eval=evaluator)
        assert len(det._graphs) == n0 + (2 if call else 1)          # one graph for the key, captured by the first call
        assert [evaluator.state(s)['frames'] for s in range(4)] == [call + 1] * 4
        without = det.predict_batch(images, score_threshold=0.0, track=alone, groundtruth=gts, track_eval=None)
        assert len(det._graphs) == n0 + 2
        evaluator.collect(outs)
        for i, (o, a, gt) in enumerate(zip(outs, without, gts)):
            assert set(o) == set(a) | {'track_eval'} and 'track_eval' not in a
            rows = o.pop('track_eval')
            for k in ('track_ids', 'track_hits', 'boxes', 'keypoints', 'scores'):
                np.testing.assert_array_equal(o[k], a[k], err_msg=k)
            for k in o['oks']:
                np.testing.assert_array_equal(o['oks'][k], a['oks'][k], err_msg=k)
            n = len(o['boxes'])
            assert n >= 3 and (o['track_ids'] > 0).all()
            assert rows['num_gt'] == rows['num_hyp'] == rows['matches'] == n and rows['switches'] == rows['misses'] == 0
            assert rows['false_positives'] == rows['untracked'] == rows['ignored_hyp'] == 0 and rows['stream'] == i
            assert rows['gt_matched'].all() and not rows['gt_switch'].any() and rows['gt_kept'].all() == (call > 0)
            assert (rows['gt_stored'] != 0).all() == (call > 0)
            np.testing.assert_array_equal(np.sort(rows['person_gt']), np.arange(n))
            # the person a ground truth is matched to is similar enough by the definition's own arithmetic
            for g in range(n):
                s = ref.oks(o['keypoints'][rows['gt_rows'][g]], gt['keypoints'][g], gt['boxes'][g], gt['boxes'][g][2] * gt['boxes'][g][3])[0]
                assert s >= 0.5 and abs(rows['gt_similarity'][g] - s) <= 1e-12 * s
                assert rows['gt_track_ids'][g] == o['track_ids'][rows['gt_rows'][g]]
    keys = [key for key in det._graphs if 'track_eval' in key]
    assert len(keys) == 1 and ('track_eval', evaluator.serial) == keys[0][-2:]
    stats = evaluator.evaluate()
    total = 3 * sum(len(p['boxes']) for p in plain)
    assert stats['num_frames'] == 12 and stats['num_objects'] == stats['num_predictions'] == stats['num_matches'] == total
    assert stats['num_switches'] == stats['num_misses'] == stats['num_false_positives'] == stats['num_fragmentations'] == 0
    assert stats['mota'] == 1.0 and stats['idf1'] == 1.0 and stats['idtp'] == total and stats['mostly_tracked'] == total // 3


def test_swapped_identities_are_two_switches(det, plain):
    """From the second call on two annotated persons of camera 0 carry each other's id: one switch each in that call, none after."""
    images = _images()
    kp = plain[0]['keypoints']
    b = plain[0]['boxes'].astype(np.float64)
    area = (b[:, 3] - b[:, 1]) * W * (b[:, 2] - b[:, 0]) * H
    n = len(kp)
    truths = np.concatenate([kp[:, :, :2], np.full((n, 17, 1), 2.0, np.float32)], 2).astype(np.float64)
    nowhere = np.zeros(4)                                           # (the box counts only for a ground truth without keypoints)
    cross = {(p, q): max(ref.oks(kp[p], truths[q], nowhere, area[q])[0], ref.oks(kp[q], truths[p], nowhere, area[p])[0])
             for p in range(n) for q in range(p + 1, n)}
    (p, q), least = min(cross.items(), key=lambda item: item[1])
    assert least < 0.4                                              # the two do not overlap: the old correspondence cannot be kept
    tracker, evaluator = _pair(4, det)
    switches = []
    for call in range(3):
        gts = _groundtruth(plain, swap=(0, p, q) if call else None)
        outs = det.predict_batch(images, score_threshold=0.0, track=tracker, groundtruth=gts, track_eval=evaluator)
        evaluator.collect(outs)
        switches.append([o['track_eval']['switches'] for o in outs])
        assert all(o['track_eval']['gt_matched'].all() for o in outs)
    assert switches == [[0, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0]]
    stats = evaluator.evaluate()
    assert stats['num_switches'] == 2 and stats['num_misses'] == 0 and stats['mota'] == 1 - 2 / stats['num_objects']
    assert stats['idfn'] == 2 and stats['idf1'] < 1.0


def test_predict_images_scores_in_source_pixels(det, plain):
    """A frame at twice the network size (each pixel doubled) with its ground truth in its own pixels."""
    images = _images()
    frames = [images[0], np.repeat(np.repeat(images[1], 2, axis=0), 2, axis=1)]
    first = det.predict_images(frames, size=(H, W), score_threshold=0.0)
    gts = [_groundtruth(first[:1])[0], _groundtruth(first[1:], 2 * H, 2 * W)[0]]
    tracker, evaluator = _pair(2, det)
    for _ in range(2):
        evaluator.collect(det.predict_images(frames, size=(H, W), score_threshold=0.0, track=tracker, groundtruth=gts,
                                             track_eval=evaluator))
    stats = evaluator.evaluate()
    assert stats['mota'] == 1.0 and stats['idf1'] == 1.0 and stats['num_objects'] == 2 * sum(len(o['boxes']) for o in first)


def test_refusals_come_before_any_device_work(det, plain, models):
    from multiposenet_amd.inference import TrackEvaluator
    images = _images()
    gts = _groundtruth(plain)
    tracker, evaluator = _pair(4, det)
    n0 = len(det._graphs)
    with pytest.raises(ValueError, match="needs track="):
        det.predict_batch(images, groundtruth=gts, track_eval=evaluator)
    with pytest.raises(ValueError, match="needs groundtruth="):
        det.predict_batch(images, track=tracker, track_eval=evaluator)
    bare = [{k: v for k, v in gt.items() if k != 'track_ids'} for gt in gts]
    with pytest.raises(ValueError, match="'track_ids'"):
        det.predict_batch(images, track=tracker, groundtruth=bare, track_eval=evaluator)
    with pytest.raises(ValueError, match="2 streams, the tracker for 4"):
        det.predict_batch(images, track=tracker, groundtruth=gts, track_eval=TrackEvaluator(streams=2, max_boxes=det.params['max_boxes']))
    with pytest.raises(ValueError, match="max_boxes"):
        det.predict_batch(images, track=tracker, groundtruth=gts, track_eval=TrackEvaluator(streams=4, max_boxes=20))
    with pytest.raises(ValueError, match="max_gt"):
        det.predict_batch(images, track=tracker, groundtruth=gts,
                          track_eval=TrackEvaluator(streams=4, max_gt=32, max_boxes=det.params['max_boxes']))
    with pytest.raises(ValueError, match="TrackEvaluator"):
        det.predict_batch(images, track=tracker, groundtruth=gts, track_eval=True)
    with pytest.raises(ValueError, match="needs track="):
        det.predict_images(list(images), size=(H, W), groundtruth=gts, track_eval=evaluator)
    assert len(det._graphs) == n0 and not tracker.prev.cpu().numpy().any() and not evaluator.prev.cpu().numpy().any()
    assert evaluator.state(0)['identities'] == {} and evaluator.num_frames == 0


def test_track_frames_with_annotations(det, models, tmp_path, capsys):
    """python -m multiposenet_amd.track_frames --annotations over three copies of one frame, annotated with its own persons."""
    import io
    from PIL import Image
    from multiposenet_amd import track_frames
    image = _images()[0]
    own = det.predict_images([image], size=(H, W), score_threshold=0.0)[0]
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "PNG")
    frames = tmp_path / "frames"
    frames.mkdir()
    data = {'images': [], 'annotations': []}
    for i in range(3):
        (frames / f"frame_{i:03d}.png").write_bytes(buf.getvalue())
        data['images'].append({'id': 10 + i, 'file_name': f"video/frame_{i:03d}.png", 'vid_id': 1, 'frame_id': i})
        for p, (kp, box) in enumerate(zip(own['keypoints'], own['boxes'].astype(np.float64))):
            data['annotations'].append({'image_id': 10 + i, 'track_id': 50 - p, 'bbox': [box[1] * W, box[0] * H, (box[3] - box[1]) * W, (box[2] - box[0]) * H],
                                        'keypoints': [float(v) for x, y, _ in kp for v in (x, y, 2)]})
    annotations = tmp_path / "annotations.json"
    annotations.write_text(json.dumps(data))
    paths = models["paths"]
    capsys.readouterr()
    track_frames.main(["--images", str(frames), "--out", str(tmp_path / "tracks.jsonl"), "--model", paths["k"], "--detector", paths["d"],
                       "--prn", paths["p"], "--size", str(W), str(H), "--batch", "2", "--dtype", "f32", "--score-threshold", "0.0",
                       "--new-track-score", "0.0", "--annotations", str(annotations), "--eval-threshold", "0.5"])
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    n = len(own['boxes'])
    got = summary["track_eval"]
    assert got["num_frames"] == 3 and got["num_objects"] == got["num_matches"] == got["num_predictions"] == 3 * n
    assert got["mota"] == 1.0 and got["idf1"] == 1.0 and got["num_switches"] == 0 and got["threshold"] == 0.5
