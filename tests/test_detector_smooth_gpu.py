"""GPU: a smoothing tracker as `track=` of Detector.predict_batch / predict_images - mpn_pose_smooth behind mpn_pose_track inside
the captured graph, both states advanced once per call outside it - against the plain-loop reference (tests/smooth_ref.py) run
on the returned dicts, byte for byte. Image size, variables and score threshold are those of tests/test_detector_batch_gpu.py."""
import numpy as np
import pytest

import smooth_ref as ref
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, models  # noqa: F401 (models: a fixture)

pytestmark = pytest.mark.gpu

TRACK_KEYS = ('track_ids', 'track_hits', 'track_new', 'track_similarity')
SMOOTH_KEYS = ('keypoints_smoothed', 'keypoint_velocities')


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _tracker(streams, smooth=True, **kw):
    from multiposenet_amd.inference import OneEuro, PoseTracker
    return PoseTracker(streams=streams, smooth=OneEuro() if smooth else None, **kw)


def _without(out, keys):
    return {k: v for k, v in out.items() if k not in keys}


def _check_against_reference(calls, streams, p=None):
    """calls: the lists of dicts of consecutive calls on one tracker. The two new keys equal the reference run on those dicts'
    'keypoints' and 'track_ids'. Returns the number of nonzero velocities seen."""
    p = p or ref.Params()                                           # OneEuro's defaults
    state, moving = ref.new_id_state(streams), 0
    for c, outs in enumerate(calls):
        for i, (o, w) in enumerate(zip(outs, ref.run(outs, state, p))):
            n = len(o['boxes'])
            assert o['keypoints_smoothed'].shape == (n, 17, 3) and o['keypoints_smoothed'].dtype == np.float32
            assert o['keypoint_velocities'].shape == (n, 17, 2) and o['keypoint_velocities'].dtype == np.float32
            for k in SMOOTH_KEYS:
                assert o[k].tobytes() == w[k].tobytes(), f"call {c} image {i} {k}"
            moving += int(np.count_nonzero(o['keypoint_velocities']))
    return moving


def test_one_stream_of_four_frames(det):
    """One stream, four frames a call (the same image rolled by 0, 3, 6 and 9 pixels), two calls."""
    im = _images()[0]
    frames = np.stack([np.roll(im, 3 * f, axis=1) for f in range(4)])
    plain = det.predict_batch(frames, score_threshold=0.0)
    base_tracker, tracker = _tracker(1, smooth=False), _tracker(1)
    base = [det.predict_batch(frames, score_threshold=0.0, track=base_tracker) for _ in range(2)]
    n0 = len(det._graphs)
    calls = [det.predict_batch(frames, score_threshold=0.0, track=tracker) for _ in range(2)]
    assert len(det._graphs) == n0 + 1                               # one graph per (tracker, b): the smooth launch is inside it
    for outs, base_outs in zip(calls, base):
        for a, t, o in zip(plain, base_outs, outs):
            assert set(o) == set(a) | set(TRACK_KEYS) | set(SMOOTH_KEYS) and len(o['boxes']) >= 3
            _assert_same(t, _without(o, SMOOTH_KEYS), "smooth=:")
            _assert_same(a, _without(o, TRACK_KEYS + SMOOTH_KEYS), "smooth=:")
    moving = _check_against_reference(calls, 1)
    assert moving > 0                                               # the frames move: some filter did run
    # 12 would be the eager pass plus the replay of the first call stepping the filters twice
    assert tracker.tracks(0)['frames'] == 8
    first = calls[0][0]                                             # the stream's first frame: every track is new
    assert first['keypoints_smoothed'].tobytes() == first['keypoints'].tobytes() and not first['keypoint_velocities'].any()
    states = (tracker.prev.cpu().numpy().tobytes(), tracker.smooth_prev.cpu().numpy().tobytes())
    n1 = len(det._graphs)
    for a, o in zip(plain, det.predict_batch(frames, score_threshold=0.0)):
        _assert_same(a, o, "after smooth=:")
    for t, o in zip(base[0], det.predict_batch(frames, score_threshold=0.0, track=_tracker(1, smooth=False))):
        _assert_same(t, o, "a plain tracker after smooth=:")
    assert len(det._graphs) == n1 + 1                               # (the new plain tracker's own graph)
    assert (tracker.prev.cpu().numpy().tobytes(), tracker.smooth_prev.cpu().numpy().tobytes()) == states


def test_streams_of_single_frames(det):
    """Four cameras, one frame each, three calls: raw keypoints and zero velocities first, the reference afterwards."""
    images = _images()
    tracker = _tracker(4)
    calls = [det.predict_batch(batch, score_threshold=0.0, track=tracker) for batch in (images, images, np.roll(images, 2, axis=2))]
    for o in calls[0]:
        assert o['keypoints_smoothed'].tobytes() == o['keypoints'].tobytes() and not o['keypoint_velocities'].any()
    moving = _check_against_reference(calls, 4)
    assert moving > 0                                               # the frames move: some filter did run
    for o in calls[1]:                                              # the same frames again: every track goes on, at rest
        assert (o['track_hits'] == 2).all()
        assert o['keypoints_smoothed'].tobytes() == o['keypoints'].tobytes() and not o['keypoint_velocities'].any()
    assert [tracker.tracks(s)['frames'] for s in range(4)] == [3] * 4
    last = tracker.tracks(0)
    assert (last['keypoint_last'][last['hits'] == 3] == 3).all()


def test_predict_images_smooths_in_source_pixels(det):
    """Frames at two source sizes (one at twice the network size): the smoothed keypoints are in the source pixels of the call's
    own 'keypoints', and equal the reference run on them."""
    images = _images()
    frames = [images[0], np.repeat(np.repeat(images[1], 2, axis=0), 2, axis=1), images[2]]
    tracker = _tracker(3)
    calls = [det.predict_images(fr, size=(H, W), score_threshold=0.0, track=tracker) for fr in (frames, frames, frames[::-1])]
    plain = det.predict_images(frames, size=(H, W), score_threshold=0.0)
    for a, o in zip(plain, calls[1]):
        _assert_same(a, _without(o, TRACK_KEYS + SMOOTH_KEYS), "predict_images smooth=:")
    moving = _check_against_reference(calls, 3)
    assert moving > 0                                               # the frames move: some filter did run
    big = calls[0][1]                                               # first samples are the frame's own keypoints: source pixels
    assert big['keypoints_smoothed'].tobytes() == big['keypoints'].tobytes()
    assert big['keypoints'][..., 0].max() > W or big['keypoints'][..., 1].max() > H


def test_a_detector_without_a_prn_refuses_a_smoothing_tracker(det, models):
    images = _images()
    noprn = _detector(models, prn=False)
    tracker = _tracker(4, similarity='iou')
    with pytest.raises(ValueError, match="smooth=.*PRN"):
        noprn.predict_batch(images, score_threshold=0.0, track=tracker)
    with pytest.raises(ValueError, match="smooth=.*PRN"):
        noprn.predict_images(list(images), size=(H, W), track=tracker)
    assert not noprn._graphs and not tracker.prev.cpu().numpy().any() and not tracker.smooth_prev.cpu().numpy().any()
    assert tracker.tracks(0)['frames'] == 0


def test_track_frames_command_line_with_smooth(cuda, models, tmp_path):
    """python -m multiposenet_amd.track_frames --smooth over four frames (one image rolled by 0, 2, 4 and 6 pixels, PNG files),
    batches of two: every line carries the two new keys, equal to the reference run on the lines themselves; the summary names
    the parameters."""
    import io
    import json
    from PIL import Image
    from multiposenet_amd import track_frames
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in range(4):
        buf = io.BytesIO()
        Image.fromarray(np.roll(_images()[0], 2 * i, axis=1)).save(buf, "PNG")
        (frames / f"frame_{i:03d}.png").write_bytes(buf.getvalue())
    out = tmp_path / "tracks.jsonl"
    paths = models["paths"]
    argv = ["--images", str(frames), "--out", str(out), "--model", paths["k"], "--detector", paths["d"], "--prn", paths["p"],
            "--size", str(W), str(H), "--batch", "2", "--dtype", "f32", "--similarity", "iou", "--score-threshold", "0.0"]
    state = track_frames.main(argv + ["--smooth", "--fps", "25", "--min-cutoff", "0.5", "--beta", "0.01", "--min-keypoint-score", "0.1"])
    assert state["frames"] == 4
    lines = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert len(lines) == 4
    ids, p = ref.new_id_state(1), ref.Params(rate=25, min_cutoff=0.5, beta=0.01, min_keypoint_score=0.1)
    for ln in lines:
        o = {'keypoints': np.array(ln["keypoints"], np.float32).reshape(-1, 17, 3), 'track_ids': ln["ids"]}
        w = ref.run([o], ids, p)[0]
        assert np.array(ln["keypoints_smoothed"], np.float32).reshape(-1, 17, 3).tobytes() == w['keypoints_smoothed'].tobytes()
        assert np.array(ln["keypoint_velocities"], np.float32).reshape(-1, 17, 2).tobytes() == w['keypoint_velocities'].tobytes()
    track_frames.main(argv)                                         # without --smooth the lines are as before
    assert set(json.loads(out.read_text().splitlines()[0])) == {"name", "ids", "boxes", "keypoints"}
    with pytest.raises(SystemExit):
        track_frames.main(argv + ["--smooth", "--fps", "0"])
