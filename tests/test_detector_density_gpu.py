"""GPU: `density=` of Detector.predict_batch / predict_images - mpn_density_map behind the tracker's launches inside the captured
graph, mpn_draw_density behind the drawing, the state advanced once per call outside the graph. Image size, variables and score
threshold are those of tests/test_detector_trails_gpu.py. 'density' is held against tests/density_ref.py applied to the returned
dicts, 'annotated' against the call without density= with the reference's `draw` applied to it, byte for byte; every other key
is what the call without density= returns."""
import json

import numpy as np
import pytest

import density_cases as cases
import density_ref as ref
from test_detector_batch_gpu import H, W, _detector, _images, models  # noqa: F401 (models: a fixture)
from test_detector_zones_gpu import _bare, _geo, _tracker

pytestmark = pytest.mark.gpu

KEYS = ('cell', 'cells', 'tracked', 'visit', 'outside', 'anchor_from_keypoints', 'max_dwell', 'max_visits', 'counted', 'visits')
PARAMS = dict(frame_size=(H, W), cell=16)


def _repeated():
    """Four frames for two streams: each stream sees one image twice a call, so that the tracker finds every person again: the
    second sight of a person is no visit."""
    return _images()[[0, 0, 1, 1]]


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _density(det, streams, **more):
    from multiposenet_amd.inference import DensityMap
    return DensityMap(streams=streams, max_boxes=det.params['max_boxes'], **dict(PARAMS, **more))


def _check_against_reference(outs, params, state, max_boxes, keypoints=True, tracked=True):
    """'density' of a call's dicts against the reference over those dicts, continuing `state` -> (what it wants, its snapshots)."""
    bare = [_bare(o, keypoints) if tracked else {k: o[k] for k in ('boxes', 'scores') + (('keypoints',) if keypoints else ())}
            for o in outs]
    rows, images, snaps = ref.run(cases.reference_params(params), bare, state, max_boxes, tracked=tracked)
    want = ref.unpacked(rows, images, [len(o['boxes']) for o in outs])
    for i, (o, w) in enumerate(zip(outs, want)):
        assert set(KEYS) == set(o['density'])
        for k in KEYS:
            if isinstance(w[k], int):
                assert type(o['density'][k]) is int and o['density'][k] == w[k], (i, k)
            else:
                assert o['density'][k].dtype == w[k].dtype and o['density'][k].shape == w[k].shape, (i, k)
                np.testing.assert_array_equal(o['density'][k], w[k], err_msg=f"image {i} {k}")
        if tracked:
            np.testing.assert_array_equal(o['density']['tracked'], o['track_ids'] > 0)
    return want, snaps


def _drawn(frame, grid, want, d):
    most = want['max_visits'] if d.show == 'visits' else want['max_dwell']
    return ref.draw_arrays(frame, grid, most, d.cell, d.smooth, d.full_scale, d.opacity, d.colormap)


def _same_but_density(with_density, without, d, wants, snaps, draw=True):
    """Every key but 'density' is that of the call without density=; 'annotated' is that call's with the map drawn on it.
    -> the number of frames the map changed."""
    changed = 0
    for o, a, want, grid in zip(with_density, without, wants, snaps):
        assert set(o) == set(a) | {'density'} and 'density' not in a
        for k in a:
            if k == 'annotated' and draw:
                picture = _drawn(a[k], grid, want, d)
                changed += int((picture != a[k]).any())
                assert o[k].dtype == picture.dtype and o[k].tobytes() == picture.tobytes(), k
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
    """Two consecutive calls of 4 frames: 'density' is the reference over the returned dicts, the second call continues the
    first (the first call's eager pass and replay count once), the map is in 'annotated', every other key is what the call
    without density= gives. Two streams of two frames a call, each stream one image again and again."""
    d = det if graph else _detector(models, graph=False)
    streams = 2
    images = _repeated()
    tracker, alone, density = _tracker(streams), _tracker(streams), _density(d, streams)
    params = cases.reference_params(PARAMS)
    state = ref.new_state(streams, params)
    n0 = len(d._graphs)

    def call(track, m):
        if method == "batch":
            return d.predict_batch(images, score_threshold=0.0, annotate=True, track=track, density=m)
        return d.predict_images(list(images), size=(H, W), score_threshold=0.0, return_heatmaps=True, annotate=True, track=track,
                                density=m)
    changed = counted = visits = 0
    for c in range(2):
        outs = call(tracker, density)
        without = call(alone, None)
        want, snaps = _check_against_reference(outs, PARAMS, state, d.params['max_boxes'])
        changed += _same_but_density(outs, without, density, want, snaps)
        counted += sum(w['counted'] for w in want)
        visits += sum(w['visits'] for w in want)
        assert density.prev.cpu().numpy().tobytes() == state.tobytes()
        assert [int(density.state(s)['frames']) for s in range(streams)] == [(c + 1) * 4 // streams] * streams
        np.testing.assert_array_equal(density.grid(1, 'visits'), state[1]['visits'])
    assert counted > 0 and 0 < visits < counted and changed >= 4
    if graph:
        keys = [key for key in d._graphs if key[-2:] == ('density', density.serial)]
        assert len(d._graphs) == n0 + 2 and len(keys) == 1          # one graph per DensityMap, captured by the first call


def test_without_a_tracker_only_the_dwell_plane_counts(det):
    images = _images()
    density = _density(det, 1, footprint='box', smooth=False, full_scale=3)
    params = dict(PARAMS, footprint='box')
    state = ref.new_state(1, cases.reference_params(params))
    changed = 0
    for _ in range(2):
        outs = det.predict_batch(images, score_threshold=0.0, annotate=True, density=density)
        without = det.predict_batch(images, score_threshold=0.0, annotate=True)
        assert all('track_ids' not in o for o in outs)
        want, snaps = _check_against_reference(outs, params, state, det.params['max_boxes'], tracked=False)
        changed += _same_but_density(outs, without, density, want, snaps)
        assert density.prev.cpu().numpy().tobytes() == state.tobytes()
    assert changed >= 4 and not density.grid(0, 'visits').any() and density.grid(0).max() >= 2
    assert sum(int(w['cells'].sum()) for w in want) > sum(w['counted'] for w in want) > 0        # boxes over several cells


def test_with_zones_trails_pose_nms_and_a_track_style(det):
    """Beside zones= and trails=, behind pose_nms= and over mpn_draw_tracks' and mpn_draw_trails' picture: the rows of the
    filtered record; the other stages' rows and states unchanged. The visits are shown."""
    from multiposenet_amd.inference import PoseNms, TrackStyle, TrackTrails, ZoneCounter
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.0)
    geo, nms, style = _geo(plain), PoseNms(threshold=0.3), TrackStyle()
    tracker, alone = _tracker(4), _tracker(4)
    density = _density(det, 4, show='visits', half_life=2, opacity=255)
    counters = [ZoneCounter(streams=4, max_boxes=det.params['max_boxes'], **geo) for _ in range(2)]
    trails = [TrackTrails(streams=4, max_boxes=det.params['max_boxes'], frame_size=(H, W), length=5) for _ in range(2)]
    params = dict(PARAMS, show='visits', half_life=2)
    state = ref.new_state(4, cases.reference_params(params))
    changed = 0
    for _ in range(3):
        common = dict(score_threshold=0.0, annotate=True, pose_nms=nms, track_style=style)
        outs = det.predict_batch(images, track=tracker, density=density, trails=trails[0], zones=counters[0], **common)
        without = det.predict_batch(images, track=alone, trails=trails[1], zones=counters[1], **common)
        want, snaps = _check_against_reference(outs, params, state, det.params['max_boxes'])
        changed += _same_but_density(outs, without, density, want, snaps)
        assert density.prev.cpu().numpy().tobytes() == state.tobytes()
    assert changed >= 2
    assert counters[0].prev.cpu().numpy().tobytes() == counters[1].prev.cpu().numpy().tobytes()
    assert trails[0].prev.cpu().numpy().tobytes() == trails[1].prev.cpu().numpy().tobytes()


def test_the_map_is_in_the_jpeg(det):
    """annotate='jpeg': the file is `encode_jpegs` of the frame annotate=True gives with the map drawn on it."""
    from multiposenet_amd.inference import encode_jpegs
    images = _images()
    tracker, alone, density = _tracker(4), _tracker(4), _density(det, 4, cell=32)
    params = dict(PARAMS, cell=32)
    state = ref.new_state(4, cases.reference_params(params))
    for c in range(2):
        outs = det.predict_images(list(images), size=(H, W), score_threshold=0.0, annotate='jpeg', jpeg_quality=90, track=tracker,
                                  density=density)
        frames = det.predict_images(list(images), size=(H, W), score_threshold=0.0, annotate=True, track=alone)
        want, snaps = _check_against_reference(outs, params, state, det.params['max_boxes'])
        drawn = [_drawn(f['annotated'], grid, w, density) for f, grid, w in zip(frames, snaps, want)]
        files = encode_jpegs([f[..., :3].copy() for f in drawn], 90, '4:2:0')
        assert all('annotated' not in o and o['annotated_jpeg'] == w for o, w in zip(outs, files))
    assert any((f != a['annotated']).any() for f, a in zip(drawn, frames))


def test_without_the_prn_the_anchor_is_the_box(models, cuda):
    d = _detector(models, prn=False)
    images = _images()
    tracker, alone, density = _tracker(4, similarity='iou'), _tracker(4, similarity='iou'), _density(d, 4)
    state = ref.new_state(4, cases.reference_params(PARAMS))
    for _ in range(2):
        outs = d.predict_batch(images, score_threshold=0.0, annotate=True, track=tracker, density=density)
        without = d.predict_batch(images, score_threshold=0.0, annotate=True, track=alone)
        want, snaps = _check_against_reference(outs, PARAMS, state, d.params['max_boxes'], keypoints=False)
        _same_but_density(outs, without, density, want, snaps)
    assert all(not o['density']['anchor_from_keypoints'].any() and len(o['boxes']) >= 3 for o in outs)
    o = outs[0]
    inside = ~o['density']['outside']
    box = o['boxes'][inside][0].astype(np.float64)
    assert o['density']['cell'][inside][0].tolist() == [int(box[2] * H) // 16, int((box[1] + box[3]) * 0.5 * W) // 16]


def test_overlay_false_and_draw_false_return_the_rows_and_draw_nothing(det):
    from multiposenet_amd.inference import Anonymize
    images = _images()
    spec = Anonymize(overlay=False)
    for more, options in ((dict(), dict(anonymize=spec)), (dict(draw=False), dict())):
        tracker, alone, density = _tracker(4), _tracker(4), _density(det, 4, **more)
        state = ref.new_state(4, cases.reference_params(PARAMS))
        for _ in range(2):
            outs = det.predict_batch(images, score_threshold=0.0, annotate=True, track=tracker, density=density, **options)
            without = det.predict_batch(images, score_threshold=0.0, annotate=True, track=alone, **options)
            want, snaps = _check_against_reference(outs, PARAMS, state, det.params['max_boxes'])
            _same_but_density(outs, without, density, want, snaps, draw=False)
        assert sum(w['counted'] for w in want) > 4 and density.grid(0).max() >= 2


def test_update_and_draw_density_on_returned_dicts_equal_the_graph(det):
    """`DensityMap.update` over what the Detector returned, with an object of its own: the rows and the state the graph wrote;
    `draw_density` over the last frame without the map: the frame the graph drew."""
    from multiposenet_amd.inference import draw_density
    images = _repeated()
    tracker, alone, density, host = _tracker(2), _tracker(2), _density(det, 2), _density(det, 2)
    for _ in range(2):
        outs = det.predict_batch(images, score_threshold=0.0, annotate=True, track=tracker, density=density)
        without = det.predict_batch(images, score_threshold=0.0, annotate=True, track=alone)
        again = host.update([_bare(o) for o in outs])
        for o, a in zip(outs, again):
            assert set(o['density']) == set(a)
            for k in a:
                assert np.asarray(o['density'][k]).tobytes() == np.asarray(a[k]).tobytes(), k
        assert density.prev.cpu().numpy().tobytes() == host.prev.cpu().numpy().tobytes()
        for s, last in ((0, 1), (1, 3)):                            # the current grid is what the stream's last frame shows
            assert draw_density(without[last]['annotated'], host, stream=s).tobytes() == outs[last]['annotated'].tobytes()
            assert draw_density(without[last]['annotated'][..., :3], host, s).tobytes() == outs[last]['annotated'].tobytes()
    with pytest.raises(ValueError, match="image must be uint8"):
        draw_density(np.zeros((4, 4), np.uint8), host)
    with pytest.raises(ValueError, match=f"grid covers {H} x {W} frames.*the image is 4 x 4"):
        draw_density(np.zeros((4, 4, 3), np.uint8), host)


def test_refusals_come_before_any_device_work(det, models):
    from multiposenet_amd.inference import DensityMap
    images = _images()
    tracker, density = _tracker(4), _density(det, 4)
    n0 = len(det._graphs)
    with pytest.raises(ValueError, match="show='visits'.*needs track="):
        det.predict_batch(images, density=_density(det, 4, show='visits'))
    with pytest.raises(ValueError, match="show='visits'.*needs track="):
        det.predict_images(list(images), size=(H, W), density=_density(det, 4, show='visits'))
    with pytest.raises(ValueError, match="2 streams, the tracker for 4"):
        det.predict_batch(images, track=tracker, density=_density(det, 2))
    with pytest.raises(ValueError, match="4 images are not a whole number of frames for each of 3 streams"):
        det.predict_batch(images, density=_density(det, 3))
    with pytest.raises(ValueError, match="max_boxes"):
        det.predict_batch(images, track=tracker, density=DensityMap(streams=4, max_boxes=20, **PARAMS))
    with pytest.raises(ValueError, match="DensityMap"):
        det.predict_batch(images, track=tracker, density=True)
    with pytest.raises(ValueError, match=f"{2 * H} x {W}.*{H} x {W}"):
        det.predict_batch(images, track=tracker, density=_density(det, 4, frame_size=(2 * H, W)))
    frames = [images[0], np.repeat(images[1], 2, axis=0), images[2], images[3]]
    with pytest.raises(ValueError, match=f"{H} x {W}.*{2 * H} x {W}"):
        det.predict_images(frames, size=(H, W), track=tracker, density=density)
    with pytest.raises(ValueError, match="no person detector"):
        _detector(models, detector=False, prn=False).predict_batch(images, density=density)
    assert len(det._graphs) == n0 and not tracker.prev.cpu().numpy().any() and not density.prev.cpu().numpy().any()


def test_track_frames_with_density(det, tmp_path, models, capsys):
    """python -m multiposenet_amd.track_frames --density --density-out over three copies of one frame: persons who do not move
    dwell three frames in their cells and visit them once; the planes are written."""
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
                       "--new-track-score", "0.0", "--density", "32", "--density-out", str(tmp_path / "map.npz"),
                       "--frames-out", str(tmp_path / "drawn")])
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    lines = [json.loads(ln) for ln in (tmp_path / "tracks.jsonl").read_text().splitlines()]
    assert summary["density"] == {"cell": 32, "grid": [H // 32, W // 32], "footprint": "anchor", "half_life": 0, "show": "dwell",
                                  "draw": True, "max_dwell": summary["density"]["max_dwell"], "max_visits": summary["density"]["max_visits"],
                                  "out": str(tmp_path / "map.npz")}
    assert len(lines) == 3 and all(len(ln["density"]["cell"]) == len(ln["ids"]) > 0 for ln in lines)
    assert lines[0]["density"]["cell"] == lines[1]["density"]["cell"] == lines[2]["density"]["cell"]
    assert [ln["density"]["visits"] for ln in lines][1:] == [0, 0] and lines[0]["density"]["visits"] > 0
    planes = np.load(tmp_path / "map.npz")
    assert int(planes["cell"]) == 32 and planes["dwell"].shape == planes["visits"].shape == (H // 32, W // 32)
    assert planes["dwell"].dtype == np.uint32 and int(planes["dwell"].sum()) == sum(ln["density"]["counted"] for ln in lines) > 0
    assert int(planes["visits"].sum()) == sum(ln["density"]["visits"] for ln in lines) and (planes["visits"] <= planes["dwell"]).all()
    assert summary["density"]["max_dwell"] == int(planes["dwell"].max()) and summary["density"]["max_visits"] == int(planes["visits"].max())
    assert sorted(p.name for p in (tmp_path / "drawn").iterdir()) == [f"frame_{i:03d}.jpg" for i in range(3)]
