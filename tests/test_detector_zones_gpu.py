"""GPU: `zones=` of Detector.predict_batch / predict_images - mpn_zone_events behind the tracker's launches inside the captured
graph, the counter's state advanced once per call outside it. Image size, variables and score threshold are those of
tests/test_detector_batch_gpu.py; the zones are cut through the first call's own anchors, and the rows are held against
tests/zones_ref.py applied to the returned dicts, byte for byte."""
import json

import numpy as np
import pytest

import zones_cases as cases
import zones_ref as ref
from test_detector_batch_gpu import H, W, _detector, _images, models  # noqa: F401 (models: a fixture)

pytestmark = pytest.mark.gpu

MAX_TRACKS = 32
KEYS = ('inside', 'entered', 'exited', 'crossed_positive', 'crossed_negative', 'anchor', 'anchor_from_keypoints', 'dwell_frames',
        'occupancy', 'entries', 'exits', 'total_entries', 'total_exits', 'line_positive', 'line_negative', 'total_line_positive',
        'total_line_negative')


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


@pytest.fixture(scope="module")
def plain(det):
    return det.predict_batch(_images(), score_threshold=0.0)


def _anchors(outs, keypoints=True):
    geo = ref.Geometry((H, W))
    return np.array([ref.anchor_of(geo, o['boxes'][r], o['keypoints'][r] if keypoints else None)[:2]
                     for o in outs for r in range(len(o['boxes']))], np.float64)


def _geo(outs, keypoints=True, **more):
    """Two zones and two lines cut through the median anchor of `outs`: some persons are inside and some are out."""
    a = _anchors(outs, keypoints)
    mx, my = float(np.median(a[:, 0])) + 0.25, float(np.median(a[:, 1])) + 0.25
    far = 4.0 * max(H, W)
    return dict(frame_size=(H, W), zones={'left': [(-far, -far), (mx, -far), (mx, far), (-far, far)],
                                          'upper': [(-far, -far), (far, -far), (far, my), (mx, my + 40.0), (-far, my)]},
                lines={'vertical': ((mx, -far), (mx, far)), 'level': ((-far, my), (far, my))}, **more)


def _tracker(streams, **more):
    from multiposenet_amd.inference import PoseTracker
    return PoseTracker(streams=streams, max_tracks=MAX_TRACKS, new_track_score=0.0, **more)


def _counter(det, geo, streams):
    from multiposenet_amd.inference import ZoneCounter
    return ZoneCounter(streams=streams, max_boxes=det.params['max_boxes'], **geo)


def _bare(o, keypoints=True):
    keep = ('boxes', 'scores', 'track_ids') + (('keypoints',) if keypoints else ())
    return {k: o[k] for k in keep}


def _check_against_reference(outs, geo, state, max_boxes, keypoints=True):
    """'zones' of a call's dicts against the reference over those dicts, continuing `state`."""
    g = cases.geometry(geo)
    bare = [_bare(o, keypoints) for o in outs]
    persons, images = ref.run(g, bare, state, max_boxes)
    want = ref.unpacked(g, persons, images, [len(o['boxes']) for o in outs], max_boxes)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert set(KEYS) <= set(o['zones'])
        for k in KEYS:
            assert o['zones'][k].dtype == w[k].dtype and o['zones'][k].shape == w[k].shape, (i, k)
            np.testing.assert_array_equal(o['zones'][k], w[k], err_msg=f"image {i} {k}")
        np.testing.assert_array_equal(o['zones']['tracked'], o['track_ids'] > 0)
    return want


def _same_but_zones(with_zones, without):
    for o, a in zip(with_zones, without):
        assert set(o) == set(a) | {'zones'} and 'zones' not in a
        for k in a:
            if isinstance(a[k], dict):
                for kk in a[k]:
                    np.testing.assert_array_equal(o[k][kk], a[k][kk], err_msg=f"{k}.{kk}")
            elif isinstance(a[k], bytes):
                assert o[k] == a[k], k
            else:
                assert np.asarray(o[k]).dtype == np.asarray(a[k]).dtype and np.asarray(o[k]).tobytes() == np.asarray(a[k]).tobytes(), k


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("method", ["batch", "images"])
def test_two_calls_equal_the_reference_and_change_no_other_key(det, models, plain, graph, method):
    """Two consecutive calls of 4 frames: 'zones' is the reference over the returned dicts, the second call continues the
    first (the first call's eager pass and replay count once), every other key is what the call without zones= gives."""
    d = det if graph else _detector(models, graph=False)
    streams = 1 if method == "batch" else 2
    geo = _geo(plain, min_frames=1 if method == "batch" else 2)
    images = _images()
    tracker, alone, counter = _tracker(streams), _tracker(streams), _counter(d, geo, streams)
    state = ref.new_state(streams)
    n0 = len(d._graphs)

    def call(track, zones):
        if method == "batch":
            return d.predict_batch(images, score_threshold=0.0, track=track, zones=zones)
        return d.predict_images(list(images), size=(H, W), score_threshold=0.0, return_heatmaps=True, track=track, zones=zones)
    seen_inside = seen_outside = 0
    for c in range(2):
        outs = call(tracker, counter)
        without = call(alone, None)
        _same_but_zones(outs, without)
        want = _check_against_reference(outs, geo, state, d.params['max_boxes'])
        seen_inside += sum(int(w['inside'].sum()) for w in want)
        seen_outside += sum(int((~w['inside']).sum()) for w in want)
        assert counter.prev.cpu().numpy().tobytes() == ref.pack_state(state)
        assert [counter.totals(s)['frames'] for s in range(streams)] == [(c + 1) * 4 // streams] * streams
    assert seen_inside > 4 and seen_outside > 4
    assert sum(int(state[s]['zone_entries'].sum()) for s in range(streams)) > 0
    if graph:
        keys = [key for key in d._graphs if key[-2:] == ('zones', counter.serial)]
        assert len(d._graphs) == n0 + 2 and len(keys) == 1                 # one graph per counter, captured by the first call


def test_zones_read_the_filtered_record_of_pose_nms(det, plain):
    from multiposenet_amd.inference import PoseNms
    geo = _geo(plain)
    images = _images()
    nms = PoseNms(threshold=0.3)
    tracker, alone, counter = _tracker(1), _tracker(1), _counter(det, geo, 1)
    outs = det.predict_batch(images, score_threshold=0.0, track=tracker, pose_nms=nms, zones=counter)
    _same_but_zones(outs, det.predict_batch(images, score_threshold=0.0, track=alone, pose_nms=nms))
    state = ref.new_state(1)
    _check_against_reference(outs, geo, state, det.params['max_boxes'])
    assert counter.prev.cpu().numpy().tobytes() == ref.pack_state(state)


def test_without_the_prn_the_anchor_is_the_box(models, cuda):
    d = _detector(models, prn=False)
    images = _images()
    first = d.predict_batch(images, score_threshold=0.0)
    geo = _geo(first, keypoints=False)
    tracker, counter = _tracker(1, similarity='iou'), _counter(d, geo, 1)
    outs = d.predict_batch(images, score_threshold=0.0, track=tracker, zones=counter)
    state = ref.new_state(1)
    want = _check_against_reference(outs, geo, state, d.params['max_boxes'], keypoints=False)
    assert all(not o['zones']['anchor_from_keypoints'].any() and len(o['boxes']) >= 3 for o in outs)
    assert sum(int(w['inside'].sum()) for w in want) > 0
    a = _anchors(outs, keypoints=False)
    got = np.concatenate([o['zones']['anchor'] for o in outs])
    assert got.tobytes() == a.tobytes()                             # ((xmin + xmax) * 0.5 * width, ymax * height)


def test_update_on_returned_dicts_equals_the_graph(det, plain):
    """`ZoneCounter.update` over what the Detector returned, with a counter of its own: the rows the graph wrote."""
    geo = _geo(plain, min_frames=2)
    images = _images()
    tracker, counter, host = _tracker(2), _counter(det, geo, 2), _counter(det, geo, 2)
    for _ in range(2):
        outs = det.predict_batch(images, score_threshold=0.0, track=tracker, zones=counter)
        again = host.update([_bare(o) for o in outs])
        for o, a in zip(outs, again):
            assert set(o['zones']) == set(a)
            for k in a:
                assert o['zones'][k].tobytes() == a[k].tobytes(), k
        assert counter.prev.cpu().numpy().tobytes() == host.prev.cpu().numpy().tobytes()


def test_refusals_come_before_any_device_work(det, plain):
    from multiposenet_amd.inference import ZoneCounter
    geo = _geo(plain)
    images = _images()
    tracker, counter = _tracker(4), _counter(det, geo, 4)
    n0 = len(det._graphs)
    with pytest.raises(ValueError, match="needs track="):
        det.predict_batch(images, zones=counter)
    with pytest.raises(ValueError, match="needs track="):
        det.predict_images(list(images), size=(H, W), zones=counter)
    with pytest.raises(ValueError, match="2 streams, the tracker for 4"):
        det.predict_batch(images, track=tracker, zones=_counter(det, geo, 2))
    with pytest.raises(ValueError, match="max_boxes"):
        det.predict_batch(images, track=tracker, zones=ZoneCounter(streams=4, max_boxes=20, **geo))
    with pytest.raises(ValueError, match="ZoneCounter"):
        det.predict_batch(images, track=tracker, zones=True)
    other = _counter(det, dict(geo, frame_size=(2 * H, W)), 4)
    with pytest.raises(ValueError, match=f"{2 * H} x {W}.*{H} x {W}"):
        det.predict_batch(images, track=tracker, zones=other)
    frames = [images[0], np.repeat(images[1], 2, axis=0), images[2], images[3]]
    with pytest.raises(ValueError, match=f"{H} x {W}.*{2 * H} x {W}"):
        det.predict_images(frames, size=(H, W), track=tracker, zones=counter)
    assert len(det._graphs) == n0 and not tracker.prev.cpu().numpy().any() and not counter.prev.cpu().numpy().any()


def test_track_frames_with_zones(det, models, tmp_path, capsys):
    """python -m multiposenet_amd.track_frames --zones over three copies of one frame."""
    import io
    from PIL import Image
    from multiposenet_amd import track_frames
    image = _images()[0]
    own = det.predict_images([image], size=(H, W), score_threshold=0.0)
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "PNG")
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in range(3):
        (frames / f"frame_{i:03d}.png").write_bytes(buf.getvalue())
    geo = _geo(own, min_frames=2)
    spec = tmp_path / "zones.json"
    spec.write_text(json.dumps(dict(geo, frame_size=[H, W])))
    paths = models["paths"]
    capsys.readouterr()
    track_frames.main(["--images", str(frames), "--out", str(tmp_path / "tracks.jsonl"), "--model", paths["k"], "--detector", paths["d"],
                       "--prn", paths["p"], "--size", str(W), str(H), "--batch", "2", "--dtype", "f32", "--score-threshold", "0.0",
                       "--new-track-score", "0.0", "--zones", str(spec)])
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    lines = [json.loads(ln) for ln in (tmp_path / "tracks.jsonl").read_text().splitlines()]
    assert len(lines) == 3
    inside = int((_anchors(own)[:, 0] < geo['zones']['left'][1][0]).sum())
    assert 0 < inside < len(own[0]['boxes'])
    for i, ln in enumerate(lines):
        z = ln["zones"]
        assert set(z) == {"inside", "entered", "exited", "crossed_positive", "crossed_negative", "occupancy", "entries", "exits",
                          "line_positive", "line_negative"}
        assert len(z["inside"]) == len(ln["ids"]) and set(z["occupancy"]) == {"left", "upper"} and set(z["line_positive"]) == {"vertical", "level"}
        # min_frames = 2: the persons, who do not move, are inside from the second frame on
        assert z["occupancy"]["left"] == (inside if i else 0) and z["entries"]["left"] == (inside if i == 1 else 0)
        assert sum('left' in names for names in z["inside"]) == z["occupancy"]["left"]
    assert summary["zones"]["frames"] == 3 and summary["zones"]["entries"]["left"] == inside and summary["zones"]["exits"]["left"] == 0
    assert summary["zones"]["line_positive"] == {"vertical": 0, "level": 0}
