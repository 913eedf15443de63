"""GPU: `trails=` of Detector.predict_batch / predict_images - mpn_track_trails behind the tracker's launches inside the captured
graph, mpn_draw_trails behind the drawing, the state advanced once per call outside the graph. Image size, variables and score
threshold are those of tests/test_detector_zones_gpu.py. 'trails' is held against tests/trails_ref.py applied to the returned
dicts, 'annotated' against the call without trails= with the reference's `draw` applied to it, byte for byte; every other key is
what the call without trails= returns."""
import json

import numpy as np
import pytest

import trails_cases as cases
import trails_ref as ref
from test_detector_batch_gpu import H, W, _detector, _images, models  # noqa: F401 (models: a fixture)
from test_detector_zones_gpu import _bare, _geo, _tracker

pytestmark = pytest.mark.gpu

KEYS = ('points', 'count', 'tracked', 'appended', 'restarted', 'anchor_from_keypoints')
PARAMS = dict(frame_size=(H, W), length=5, every=1, max_gap=30)


def _repeated():
    """Four frames for two streams: each stream sees one image twice a call, so that the tracker finds every person again and
    the trails have segments (of no length: the persons do not move)."""
    return _images()[[0, 0, 1, 1]]


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _trails(det, streams, **more):
    from multiposenet_amd.inference import TrackTrails
    return TrackTrails(streams=streams, max_boxes=det.params['max_boxes'], **dict(PARAMS, **more))


def _check_against_reference(outs, params, state, max_boxes, keypoints=True):
    """'trails' of a call's dicts against the reference over those dicts, continuing `state`."""
    rows = ref.run(cases.reference_params(params), [_bare(o, keypoints) for o in outs], state, max_boxes)
    want = ref.unpacked(rows, [len(o['boxes']) for o in outs])
    for i, (o, w) in enumerate(zip(outs, want)):
        assert set(KEYS) == set(o['trails'])
        for k in KEYS:
            assert o['trails'][k].dtype == w[k].dtype and o['trails'][k].shape == w[k].shape, (i, k)
            np.testing.assert_array_equal(o['trails'][k], w[k], err_msg=f"image {i} {k}")
        np.testing.assert_array_equal(o['trails']['tracked'], o['track_ids'] > 0)
    return want


def _drawn(frame, o, t, palette=None):
    from multiposenet_amd.inference.draw import DEFAULT_PALETTE
    return ref.draw(frame.copy(), o['trails'], o['track_ids'], t.length, palette or DEFAULT_PALETTE, t.fade, t.min_alpha)


def _same_but_trails(with_trails, without, t, draw=True):
    """Every key but 'trails' is that of the call without trails=; 'annotated' is that call's with the trails drawn on it.
    -> the number of frames the trails changed."""
    changed = 0
    for o, a in zip(with_trails, without):
        assert set(o) == set(a) | {'trails'} and 'trails' not in a
        for k in a:
            if k == 'annotated' and draw:
                want = _drawn(a[k], o, t)
                changed += int((want != a[k]).any())
                assert o[k].dtype == want.dtype and o[k].tobytes() == want.tobytes(), k
            elif isinstance(a[k], dict):
                for kk in a[k]:
                    np.testing.assert_array_equal(o[k][kk], a[k][kk], err_msg=f"{k}.{kk}")
            elif isinstance(a[k], bytes):
                assert o[k] == a[k], k
            else:
                assert np.asarray(o[k]).dtype == np.asarray(a[k]).dtype and np.asarray(o[k]).tobytes() == np.asarray(a[k]).tobytes(), k
    return changed


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("method", ["batch", "images"])
def test_two_calls_equal_the_reference_and_change_no_other_key(det, models, graph, method):
    """Two consecutive calls of 4 frames: 'trails' is the reference over the returned dicts, the second call continues the first
    (the first call's eager pass and replay count once), the trails are in 'annotated', every other key is what the call without
    trails= gives. Two streams of two frames a call, each stream one image again and again."""
    d = det if graph else _detector(models, graph=False)
    streams = 2
    images = _repeated()
    tracker, alone, trails = _tracker(streams), _tracker(streams), _trails(d, streams)
    state = ref.new_state(streams, trails.length)
    n0 = len(d._graphs)

    def call(track, t):
        if method == "batch":
            return d.predict_batch(images, score_threshold=0.0, annotate=True, track=track, trails=t)
        return d.predict_images(list(images), size=(H, W), score_threshold=0.0, return_heatmaps=True, annotate=True, track=track,
                                trails=t)
    changed = segments = 0
    for c in range(2):
        outs = call(tracker, trails)
        without = call(alone, None)
        changed += _same_but_trails(outs, without, trails)
        want = _check_against_reference(outs, PARAMS, state, d.params['max_boxes'])
        segments += sum(int((w['count'][w['tracked']] >= 2).sum()) for w in want)
        assert trails.prev.cpu().numpy().tobytes() == state.tobytes()
        assert [int(trails.state(s)['frames']) for s in range(streams)] == [(c + 1) * 4 // streams] * streams
    assert segments > 4 and changed >= 2
    if graph:
        keys = [key for key in d._graphs if key[-2:] == ('trails', trails.serial)]
        assert len(d._graphs) == n0 + 2 and len(keys) == 1                 # one graph per TrackTrails, captured by the first call


def test_with_zones_pose_nms_and_a_track_style(det):
    """Beside zones=, behind pose_nms= and over mpn_draw_tracks' picture: the rows of the filtered record, zones' rows unchanged."""
    from multiposenet_amd.inference import PoseNms, TrackStyle, ZoneCounter
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.0)
    geo, nms, style = _geo(plain), PoseNms(threshold=0.3), TrackStyle()
    tracker, alone, trails = _tracker(4), _tracker(4), _trails(det, 4, every=2, fade=False)
    counters = [ZoneCounter(streams=4, max_boxes=det.params['max_boxes'], **geo) for _ in range(2)]
    state = ref.new_state(4, trails.length)
    changed = 0
    for _ in range(3):
        common = dict(score_threshold=0.0, annotate=True, pose_nms=nms, track_style=style)
        outs = det.predict_batch(images, track=tracker, trails=trails, zones=counters[0], **common)
        without = det.predict_batch(images, track=alone, zones=counters[1], **common)
        changed += _same_but_trails(outs, without, trails)
        _check_against_reference(outs, dict(PARAMS, every=2), state, det.params['max_boxes'])
        assert trails.prev.cpu().numpy().tobytes() == state.tobytes()
    assert changed >= 2
    assert counters[0].prev.cpu().numpy().tobytes() == counters[1].prev.cpu().numpy().tobytes()


def test_the_trails_are_in_the_jpeg(det):
    """annotate='jpeg': the file is `encode_jpegs` of the frame annotate=True gives with the trails drawn on it."""
    from multiposenet_amd.inference import encode_jpegs
    images = _images()
    tracker, alone, trails = _tracker(4), _tracker(4), _trails(det, 4, min_alpha=0)
    for c in range(2):
        outs = det.predict_images(list(images), size=(H, W), score_threshold=0.0, annotate='jpeg', jpeg_quality=90, track=tracker,
                                  trails=trails)
        frames = det.predict_images(list(images), size=(H, W), score_threshold=0.0, annotate=True, track=alone)
        drawn = [_drawn(f['annotated'], o, trails) for f, o in zip(frames, outs)]
        want = encode_jpegs([f[..., :3].copy() for f in drawn], 90, '4:2:0')
        assert all('annotated' not in o and o['annotated_jpeg'] == w for o, w in zip(outs, want))
    assert any((f != a['annotated']).any() for f, a in zip(drawn, frames))


def test_without_the_prn_the_anchor_is_the_box(models, cuda):
    d = _detector(models, prn=False)
    images = _images()
    tracker, alone, trails = _tracker(4, similarity='iou'), _tracker(4, similarity='iou'), _trails(d, 4)
    state = ref.new_state(4, trails.length)
    for _ in range(2):
        outs = d.predict_batch(images, score_threshold=0.0, annotate=True, track=tracker, trails=trails)
        without = d.predict_batch(images, score_threshold=0.0, annotate=True, track=alone)
        _same_but_trails(outs, without, trails)
        _check_against_reference(outs, PARAMS, state, d.params['max_boxes'], keypoints=False)
    assert all(not o['trails']['anchor_from_keypoints'].any() and len(o['boxes']) >= 3 for o in outs)
    o = outs[0]
    box = o['boxes'][0].astype(np.float64)
    assert o['trails']['points'][0, 0].tolist() == [np.float32((box[1] + box[3]) * 0.5 * W), np.float32(box[2] * H)]


def test_overlay_false_and_draw_false_return_the_rows_and_draw_nothing(det):
    from multiposenet_amd.inference import Anonymize
    images = _images()
    spec = Anonymize(overlay=False)
    for more, options in ((dict(), dict(anonymize=spec)), (dict(draw=False), dict())):
        tracker, alone, trails = _tracker(4), _tracker(4), _trails(det, 4, **more)
        state = ref.new_state(4, trails.length)
        for _ in range(2):
            outs = det.predict_batch(images, score_threshold=0.0, annotate=True, track=tracker, trails=trails, **options)
            without = det.predict_batch(images, score_threshold=0.0, annotate=True, track=alone, **options)
            _same_but_trails(outs, without, trails, draw=False)
            want = _check_against_reference(outs, PARAMS, state, det.params['max_boxes'])
        assert sum(int((w['count'] >= 2).sum()) for w in want) > 4


def test_update_and_draw_trails_on_returned_dicts_equal_the_graph(det):
    """`TrackTrails.update` over what the Detector returned, with an object of its own: the rows the graph wrote; `draw_trails`
    over the frame without trails: the frame the graph drew."""
    from multiposenet_amd.inference import draw_trails
    images = _repeated()
    tracker, alone, trails, host = _tracker(2), _tracker(2), _trails(det, 2), _trails(det, 2)
    for _ in range(2):
        outs = det.predict_batch(images, score_threshold=0.0, annotate=True, track=tracker, trails=trails)
        without = det.predict_batch(images, score_threshold=0.0, annotate=True, track=alone)
        again = host.update([_bare(o) for o in outs])
        for o, a, w in zip(outs, again, without):
            assert set(o['trails']) == set(a)
            for k in a:
                assert o['trails'][k].tobytes() == a[k].tobytes(), k
            assert draw_trails(w['annotated'], o, host).tobytes() == o['annotated'].tobytes()
            assert draw_trails(w['annotated'][..., :3], o, host).tobytes() == o['annotated'].tobytes()
        assert trails.prev.cpu().numpy().tobytes() == host.prev.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="needs 'trails' and 'track_ids'"):
        draw_trails(without[0]['annotated'], without[0], host)
    with pytest.raises(ValueError, match="image must be uint8"):
        draw_trails(np.zeros((4, 4), np.uint8), outs[0], host)


def test_refusals_come_before_any_device_work(det):
    from multiposenet_amd.inference import TrackTrails
    images = _images()
    tracker, trails = _tracker(4), _trails(det, 4)
    n0 = len(det._graphs)
    with pytest.raises(ValueError, match="needs track="):
        det.predict_batch(images, trails=trails)
    with pytest.raises(ValueError, match="needs track="):
        det.predict_images(list(images), size=(H, W), trails=trails)
    with pytest.raises(ValueError, match="2 streams, the tracker for 4"):
        det.predict_batch(images, track=tracker, trails=_trails(det, 2))
    with pytest.raises(ValueError, match="max_boxes"):
        det.predict_batch(images, track=tracker, trails=TrackTrails(streams=4, max_boxes=20, **PARAMS))
    with pytest.raises(ValueError, match="TrackTrails"):
        det.predict_batch(images, track=tracker, trails=True)
    with pytest.raises(ValueError, match=f"{2 * H} x {W}.*{H} x {W}"):
        det.predict_batch(images, track=tracker, trails=_trails(det, 4, frame_size=(2 * H, W)))
    frames = [images[0], np.repeat(images[1], 2, axis=0), images[2], images[3]]
    with pytest.raises(ValueError, match=f"{H} x {W}.*{2 * H} x {W}"):
        det.predict_images(frames, size=(H, W), track=tracker, trails=trails)
    assert len(det._graphs) == n0 and not tracker.prev.cpu().numpy().any() and not trails.prev.cpu().numpy().any()


def test_track_frames_with_trails(det, tmp_path, models, capsys):
    """python -m multiposenet_amd.track_frames --trails over three copies of one frame: a person who does not move has a trail of
    1, 2, 3 equal points; with --frames-out the frames are written."""
    import io
    from PIL import Image
    from multiposenet_amd import track_frames
    image = _images()[0]
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "PNG")
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in range(3):
        (frames / f"frame_{i:03d}.png").write_bytes(buf.getvalue())
    paths = models["paths"]
    capsys.readouterr()
    track_frames.main(["--images", str(frames), "--out", str(tmp_path / "tracks.jsonl"), "--model", paths["k"], "--detector", paths["d"],
                       "--prn", paths["p"], "--size", str(W), str(H), "--batch", "2", "--dtype", "f32", "--score-threshold", "0.0",
                       "--new-track-score", "0.0", "--trails", "2", "--trail-max-gap", "0", "--frames-out", str(tmp_path / "drawn")])
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    lines = [json.loads(ln) for ln in (tmp_path / "tracks.jsonl").read_text().splitlines()]
    assert summary["trails"] == {"length": 2, "every": 1, "max_gap": 0, "anchor": "feet", "fade": True, "draw": True}
    assert len(lines) == 3 and all(len(ln["trail"]) == len(ln["ids"]) > 0 for ln in lines)
    for i, ln in enumerate(lines):
        assert [len(t) for t, tid in zip(ln["trail"], ln["ids"]) if tid > 0] == [min(i + 1, 2)] * sum(t > 0 for t in ln["ids"])
        assert all(t == [] for t, tid in zip(ln["trail"], ln["ids"]) if tid <= 0)
        assert all(all(p == t[0] for p in t) for t in ln["trail"] if t)
    assert sorted(p.name for p in (tmp_path / "drawn").iterdir()) == [f"frame_{i:03d}.jpg" for i in range(3)]
