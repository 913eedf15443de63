"""GPU: `track=PoseTracker(motion=ConstantVelocity(...))` through the Detector - mpn_pose_track_motion inside the captured
graph, its coasting rows behind the track rows (and the smoothed rows) in the record's one copy - against `update()` of a
twin tracker on the returned dicts (which tests/test_pose_motion_gpu.py holds against the reference); `smooth=`, `annotate`
and `track_style=` with a motion tracker; a tracker without motion returns no new key. Image size, variables and score
threshold are those of tests/test_detector_batch_gpu.py."""
import numpy as np
import pytest

from test_detector_batch_gpu import H, W, _detector, _images, models  # noqa: F401 (models: a fixture)

pytestmark = pytest.mark.gpu

TRACK_KEYS = {'track_ids', 'track_hits', 'track_new', 'track_similarity'}
COAST_KEYS = {'coasting_ids', 'coasting_misses', 'coasting_boxes', 'coasting_keypoints'}
MAX_TRACKS = 32


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _tracker(streams, similarity='oks', motion=True, **kw):
    from multiposenet_amd.inference import ConstantVelocity, PoseTracker
    return PoseTracker(streams=streams, max_tracks=MAX_TRACKS, similarity=similarity, motion=ConstantVelocity() if motion else None, **kw)


def _check_shapes(o):
    m = len(o['coasting_ids'])
    assert o['coasting_ids'].dtype == np.int32 and o['coasting_misses'].dtype == np.int32 and o['coasting_misses'].shape == (m,)
    assert o['coasting_boxes'].dtype == np.float32 and o['coasting_boxes'].shape == (m, 4)
    assert o['coasting_keypoints'].dtype == np.float32 and o['coasting_keypoints'].shape == (m, 17, 2)
    assert (o['coasting_ids'] > 0).all() and (o['coasting_misses'] >= 1).all()
    assert not set(o['coasting_ids']) & set(o['track_ids'])         # a track is detected in a frame or coasts, never both


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_motion_tracker_in_the_captured_graph(det, similarity):
    """Four cameras: the same frames twice, a call in which nothing passes the score threshold (every track coasts at its
    stored pose: nothing has moved yet), the frames again, then rotated among the cameras. A twin tracker's `update()` on the
    returned dicts gives the same ids and coasting rows."""
    images = _images()
    tracker, twin = _tracker(4, similarity), _tracker(4, similarity)
    n0 = len(det._graphs)
    calls = [det.predict_batch(images, score_threshold=0.0, track=tracker) for _ in range(2)]
    assert len(det._graphs) == n0 + 1
    calls.append(det.predict_batch(images, score_threshold=2.0, track=tracker))
    calls.append(det.predict_batch(images, score_threshold=0.0, track=tracker))
    calls.append(det.predict_batch(np.roll(images, 1, axis=0), score_threshold=0.0, track=tracker))
    assert len(det._graphs) == n0 + 2                               # one entry per threshold, each replayed
    for c, outs in enumerate(calls):
        for i, (o, w) in enumerate(zip(outs, twin.update(outs))):
            assert TRACK_KEYS | COAST_KEYS <= set(o)
            _check_shapes(o)
            for k in ('track_ids', 'track_hits', 'track_new'):
                np.testing.assert_array_equal(o[k], w[k], err_msg=f"{similarity} call {c} image {i} {k}")
            for k in sorted(COAST_KEYS):
                assert o[k].tobytes() == w[k].tobytes(), f"{similarity} call {c} image {i} {k}"
    assert tracker.prev.cpu().numpy().tobytes() == twin.prev.cpu().numpy().tobytes()
    assert tracker.motion_prev.cpu().numpy().tobytes() == twin.motion_prev.cpu().numpy().tobytes()
    for first, second, hidden, back in zip(*calls[:4]):
        n = len(first['boxes'])
        assert n >= 3 and len(first['coasting_ids']) == 0 and len(second['coasting_ids']) == 0
        np.testing.assert_array_equal(second['track_hits'], np.full(n, 2))      # the first call stepped the state once
        assert len(hidden['boxes']) == 0 and len(hidden['track_ids']) == 0
        np.testing.assert_array_equal(hidden['coasting_ids'], np.arange(1, n + 1))
        np.testing.assert_array_equal(hidden['coasting_misses'], np.ones(n))
        assert hidden['coasting_boxes'].tobytes() == second['boxes'].astype(np.float32).tobytes()
        assert hidden['coasting_keypoints'].tobytes() == np.ascontiguousarray(second['keypoints'][:, :, :2], np.float32).tobytes()
        np.testing.assert_array_equal(back['track_ids'], np.arange(1, n + 1))
        np.testing.assert_array_equal(back['track_hits'], np.full(n, 3))


def test_smooth_annotate_and_style_with_a_motion_tracker(det):
    """One camera, one frame per call (25 slots: the smoothed rows end off a multiple of 8 bytes and the coasting rows are
    padded behind them): a tracker with smooth= and motion= returns and draws what one with smooth= alone does while nothing
    moves, plus the coasting keys."""
    from multiposenet_amd.inference import OneEuro, TrackStyle
    style = TrackStyle(keypoints='smoothed')
    both, smooth = _tracker(1, smooth=OneEuro(rate=30.0)), _tracker(1, motion=False, smooth=OneEuro(rate=30.0))
    assert both.coast_offset(1) % 8 == 0 and both.coast_offset(1) == smooth.out_bytes(1) + 4
    image = _images()[:1]
    for c in range(3):
        got = det.predict_batch(image, score_threshold=0.0, annotate=True, track=both, track_style=style)[0]
        want = det.predict_batch(image, score_threshold=0.0, annotate=True, track=smooth, track_style=style)[0]
        assert set(got) == set(want) | COAST_KEYS and 'keypoints_smoothed' in got
        _check_shapes(got)
        for k in want:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (c, k)
        np.testing.assert_array_equal(got['track_hits'], np.full(len(got['boxes']), c + 1))
    plain = det.predict_batch(image, score_threshold=0.0, annotate=True, track=_tracker(1))[0]
    assert COAST_KEYS <= set(plain) and 'annotated' in plain and 'keypoints_smoothed' not in plain


def _value(v):
    """A result value as something `==` compares byte for byte: arrays with dtype and shape, the tables of 'oks' key by key."""
    if isinstance(v, dict):
        return {k: _value(x) for k, x in v.items()}
    if isinstance(v, bytes):
        return v
    v = np.asarray(v)
    return v.dtype.str, v.shape, v.tobytes()


def test_every_row_block_behind_one_record(det):
    """One predict_images call over two frames of one camera with groundtruth=, annotate='jpeg', a tracker with smooth= and
    motion= and a style that draws the smoothed keypoints: the OKS rows, the track rows, the smoothed rows and the coasting
    rows (padded: 25 slots) all lie behind the one record, and the drawing reads two of the blocks in place. Every key equals,
    byte for byte, the key of the call that switches on only the option it belongs to, with a fresh tracker of its own."""
    from multiposenet_amd.inference import ConstantVelocity, OneEuro, PoseTracker, TrackStyle
    from test_detector_oks_gpu import _groundtruth
    style = TrackStyle(keypoints='smoothed')
    frames = list(_images()[:2])

    def call(tracked=False, **options):
        if tracked:
            options['track'] = PoseTracker(streams=1, max_tracks=MAX_TRACKS, smooth=OneEuro(), motion=ConstantVelocity())
        return det.predict_images(frames, size=(H, W), score_threshold=0.0, **options)
    plain = call()
    gts = _groundtruth(plain, [(H, W)] * 2, 0.01, without=1)
    assert len(gts[0]['keypoints']) >= 3
    alone = {'oks': call(groundtruth=gts), 'annotated_jpeg': call(True, annotate='jpeg', track_style=style)}
    tracked = call(True)
    n0 = len(det._graphs)
    got = call(True, groundtruth=gts, annotate='jpeg', track_style=style)
    assert len(det._graphs) == n0 + 1
    smooth_keys = {'keypoints_smoothed', 'keypoint_velocities'}
    for i, o in enumerate(got):
        assert set(o) == set(plain[i]) | {'oks', 'annotated_jpeg'} | TRACK_KEYS | smooth_keys | COAST_KEYS
        _check_shapes(o)
        for k, v in o.items():
            want = plain[i] if k in plain[i] else alone[k][i] if k in alone else tracked[i]
            assert _value(v) == _value(want[k]), f"image {i} {k}"
    n = len(got[0]['boxes'])
    np.testing.assert_array_equal(got[0]['track_ids'], np.arange(1, n + 1))      # the first frame starts a track per person
    assert n >= 3 and got[0]['annotated_jpeg'][:2] == b"\xff\xd8" and (got[0]['oks']['matches'][:, 0, 0] >= 0).any()


def test_a_plain_tracker_returns_no_new_key(det):
    from multiposenet_amd.inference import PoseTracker
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.0, track=_tracker(4, motion=False))
    untracked = det.predict_batch(images, score_threshold=0.0)
    for o, u in zip(plain, untracked):
        assert set(o) == set(u) | TRACK_KEYS
    tracker = PoseTracker(streams=4, max_tracks=MAX_TRACKS)
    assert tracker.motion is None and not hasattr(tracker, 'motion_prev') and tracker.out_bytes(4) == tracker.track_bytes(4)
    assert tracker.coast_offset(4) == tracker.track_bytes(4)


def test_track_frames_command_line(cuda, models, tmp_path):
    """python -m multiposenet_amd.track_frames --motion over three copies of one frame, batches of two: every line carries the
    coasting keys (nobody coasts in a video that stands still), the ids stay."""
    import io
    import json
    from PIL import Image
    from multiposenet_amd import track_frames
    buf = io.BytesIO()
    Image.fromarray(_images()[0]).save(buf, "PNG")
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in range(3):
        (frames / f"frame_{i:03d}.png").write_bytes(buf.getvalue())
    out = tmp_path / "tracks.jsonl"
    paths = models["paths"]
    state = track_frames.main(["--images", str(frames), "--out", str(out), "--model", paths["k"], "--detector", paths["d"],
                               "--prn", paths["p"], "--size", str(W), str(H), "--batch", "2", "--dtype", "f32",
                               "--similarity", "iou", "--motion", "--velocity-gain", "0.25", "--score-threshold", "0.0"])
    lines = [json.loads(ln) for ln in out.read_text().splitlines()]
    n = len(lines[0]["ids"])
    assert n >= 3 and all(ln["ids"] == list(range(1, n + 1)) for ln in lines)
    for ln in lines:
        assert set(ln) == {"name", "ids", "boxes", "keypoints", "coasting_ids", "coasting_boxes", "coasting_keypoints"}
        assert ln["coasting_ids"] == [] and ln["coasting_boxes"] == [] and ln["coasting_keypoints"] == []
    # (the boxes of a frame do not depend on the batch it came in; the PRN's keypoints may, in their last bits)
    assert (state["hits"] == 3).all() and state["velocities"].shape == (n, 6) and not state["velocities"][:, :4].any()
    assert (state["seen"] == 2).all() and state["boxes_predicted"].tobytes() == state["boxes"].tobytes()
