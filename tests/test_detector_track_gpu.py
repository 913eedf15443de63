"""GPU: `track=` of Detector.predict_batch / predict_images - mpn_pose_track inside the captured graph, the state advanced
once per call outside it - against the plain-loop reference (tests/track_ref.py) on the returned dicts. Image size, variables
and score threshold are those of tests/test_detector_batch_gpu.py."""
import numpy as np
import pytest

import pil_resize_ref as P
import track_ref as ref
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, models  # noqa: F401 (models: a fixture)
from test_detector_oks_gpu import _groundtruth

pytestmark = pytest.mark.gpu

TRACK_KEYS = ('track_ids', 'track_hits', 'track_new', 'track_similarity')
MAX_TRACKS = 32


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _tracker(streams, similarity='oks', **kw):
    from multiposenet_amd.inference import PoseTracker
    return PoseTracker(streams=streams, max_tracks=MAX_TRACKS, similarity=similarity, **kw)


def _plain(out):
    return {k: v for k, v in out.items() if k not in TRACK_KEYS}


def _check_against_reference(calls, streams, similarity):
    """calls: the lists of dicts of consecutive calls on one tracker. Ids, hits and the new flag equal the reference run on
    those dicts; for OKS no decision of the reference is within 1e-9 of flipping, so a mismatch is not an ulp artefact."""
    p = ref.Params(MAX_TRACKS, similarity, 0.3, 10, 0.3)            # PoseTracker's defaults
    state, log = ref.new_state(streams, MAX_TRACKS), []
    for c, outs in enumerate(calls):
        want = ref.run(outs, state, p, log)
        for i, (o, w) in enumerate(zip(outs, want)):
            for k in ('track_ids', 'track_hits', 'track_new'):
                np.testing.assert_array_equal(o[k], w[k], err_msg=f"{similarity} call {c} image {i} {k}")
            if similarity == 'iou':
                assert o['track_similarity'].tobytes() == w['track_similarity'].tobytes()
            else:
                np.testing.assert_allclose(o['track_similarity'], w['track_similarity'], rtol=1e-12, atol=0)
    if similarity == 'oks':
        assert ref.undecided(log) == []
    return state


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_streams_of_single_frames(det, similarity):
    """(a) four cameras, one frame each, the same frames three times; (c) then the frames rotated among the cameras; (f) every
    other key as without track=, and a call without it leaves the tracker alone."""
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.0)
    n0 = len(det._graphs)
    tracker = _tracker(4, similarity)
    calls = [det.predict_batch(images, score_threshold=0.0, track=tracker) for _ in range(3)]
    assert len(det._graphs) == n0 + 1
    for c, outs in enumerate(calls):
        for a, o in zip(plain, outs):
            assert set(o) == set(a) | set(TRACK_KEYS)
            _assert_same(a, _plain(o), "track=:")
            n = len(o['boxes'])
            assert n >= 3 and o['track_ids'].shape == (n,) and o['track_ids'].dtype == np.int32
            assert o['track_hits'].dtype == np.int32 and o['track_new'].dtype == bool and o['track_similarity'].dtype == np.float64
            # hits == 2 after the first call would be the eager pass plus the replay stepping the state twice
            np.testing.assert_array_equal(o['track_hits'], np.full(n, c + 1))
            np.testing.assert_array_equal(o['track_ids'], np.arange(1, n + 1))
            assert o['track_new'].all() == (c == 0) and o['track_new'].any() == (c == 0)
            if c:
                np.testing.assert_array_equal(o['track_similarity'], np.ones(n))
    state = tracker.prev.cpu().numpy().tobytes()
    for a, o in zip(plain, det.predict_batch(images, score_threshold=0.0)):
        _assert_same(a, o, "after track=:")
    assert len(det._graphs) == n0 + 1 and tracker.prev.cpu().numpy().tobytes() == state
    calls.append(det.predict_batch(np.roll(images, 1, axis=0), score_threshold=0.0, track=tracker))
    assert len(det._graphs) == n0 + 1
    final = _check_against_reference(calls, 4, similarity)
    assert tracker.prev.cpu().numpy().tobytes() == ref.pack_state(final)


def test_one_stream_of_consecutive_frames(det):
    """(b) one camera, the same frame four times in one call: hits 1..4 inside the call, the ids of four single-frame calls."""
    im = _images()[0]
    batch = det.predict_batch(np.stack([im] * 4), score_threshold=0.0, track=_tracker(1))
    single = _tracker(1)
    for f, o in enumerate(batch):
        n = len(o['boxes'])
        np.testing.assert_array_equal(o['track_hits'], np.full(n, f + 1))
        one = det.predict_batch(im[None], score_threshold=0.0, track=single)[0]
        for k in TRACK_KEYS:
            np.testing.assert_array_equal(o[k], one[k], err_msg=f"frame {f} {k}")
    np.testing.assert_array_equal(batch[0]['track_ids'], np.arange(1, len(batch[0]['boxes']) + 1))


def test_eager_path_and_reloaded_variables(det, models):
    """(d) use_graph False gives the same ids over the same calls; (e) after load_state_dict the graph path runs an eager pass
    and the replay in one call: the state still advances once."""
    images = _images()
    eager = _detector(models, graph=False)
    t_graph, t_eager = _tracker(4), _tracker(4)
    for batch in (images, images, np.roll(images, 1, axis=0)):
        for a, b in zip(det.predict_batch(batch, score_threshold=0.0, track=t_graph),
                        eager.predict_batch(batch, score_threshold=0.0, track=t_eager)):
            _assert_same(a, b, "graph vs eager, track=:")
    assert not eager._graphs and t_graph.prev.cpu().numpy().tobytes() == t_eager.prev.cpu().numpy().tobytes()
    tracker = _tracker(4)
    det.predict_batch(images, score_threshold=0.0, track=tracker)
    versions = det._variable_versions()
    det.net.load_state_dict(models["bb"])                           # the same values: only the versions move
    assert det._variable_versions() != versions
    for o in det.predict_batch(images, score_threshold=0.0, track=tracker):
        np.testing.assert_array_equal(o['track_hits'], np.full(len(o['boxes']), 2))
        assert not o['track_new'].any()


def test_track_with_groundtruth(det):
    """(g) both tables, each equal to what it is alone."""
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.0)
    gts = _groundtruth(plain, [(H, W)] * len(images), 0.01)
    only_gt = det.predict_batch(images, score_threshold=0.0, groundtruth=gts)
    t_alone, t_both = _tracker(4), _tracker(4)
    for _ in range(2):
        only_track = det.predict_batch(images, score_threshold=0.0, track=t_alone)
        both = det.predict_batch(images, score_threshold=0.0, track=t_both, groundtruth=gts)
        for g, t, o in zip(only_gt, only_track, both):
            assert set(o) == set(t) | {'oks'}
            _assert_same(t, {k: v for k, v in o.items() if k != 'oks'}, "track= + groundtruth=:")
            for k in g['oks']:
                np.testing.assert_array_equal(o['oks'][k], g['oks'][k], err_msg=k)
    assert (both[0]['track_hits'] == 2).all()


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_predict_images_tracks_in_source_pixels(det, similarity):
    """(h) a frame at twice the network size (each pixel doubled): boxes are normalised, so IoU gives the ids (and the
    similarities) of the network-size batch; OKS sees the keypoints in source pixels, as the reference does on the returned dicts."""
    images = _images()
    frames = [images[0], np.repeat(np.repeat(images[1], 2, axis=0), 2, axis=1), images[2]]
    tracker = _tracker(3, similarity)
    calls = [det.predict_images(fr, size=(H, W), score_threshold=0.0, track=tracker) for fr in (frames, frames, frames[::-1])]
    plain = det.predict_images(frames, size=(H, W), score_threshold=0.0)
    for a, o in zip(plain, calls[1]):
        _assert_same(a, _plain(o), "predict_images track=:")
        assert (o['track_hits'] == 2).all() and len(o['boxes']) >= 3
    _check_against_reference(calls, 3, similarity)
    if similarity == 'iou':
        # the network-size batch is the resized canvas (pil_resize_ref: what the device resize equals byte for byte); the doubled
        # frame's canvas is a bicubic reduction, not images[1] itself
        canvas = np.stack([P.canvas(f, H, W, False) for f in frames])
        assert np.array_equal(canvas[0], images[0]) and not np.array_equal(canvas[1], images[1])
        same_size = _tracker(3, similarity)
        for batch, outs in zip((canvas, canvas, canvas[::-1]), calls):
            for a, o in zip(det.predict_batch(batch, score_threshold=0.0, track=same_size), outs):
                for k in TRACK_KEYS:
                    np.testing.assert_array_equal(a[k], o[k], err_msg=k)


def test_track_argument_errors(det, models):
    """(i) raised before any device work: the tracker's state does not move, no graph is added."""
    import torch
    images = _images()
    n0 = len(det._graphs)
    with pytest.raises(ValueError, match="person detector"):
        _detector(models, detector=False, prn=False).predict_batch(images, track=_tracker(4))
    with pytest.raises(ValueError, match="PRN"):
        _detector(models, prn=False).predict_batch(images, track=_tracker(4, 'oks'))
    with pytest.raises(ValueError, match="whole number of frames"):
        det.predict_batch(images, track=_tracker(3))
    with pytest.raises(ValueError, match="max_boxes"):
        det.predict_batch(images, track=_tracker(4, max_boxes=20))
    with pytest.raises(ValueError, match="PoseTracker"):
        det.predict_batch(images, track=True)
    elsewhere = _tracker(4)
    elsewhere.device = torch.device("cuda", 1)
    with pytest.raises(ValueError, match="lives on"):
        det.predict_batch(images, track=elsewhere)
    with pytest.raises(ValueError, match="whole number of frames"):
        det.predict_images(list(images), size=(H, W), track=_tracker(3))
    assert len(det._graphs) == n0 and not elsewhere.prev.cpu().numpy().any()
    # a detector without a PRN tracks by IoU
    noprn = _detector(models, prn=False)
    tracker = _tracker(4, 'iou')
    for c in range(2):
        for o in noprn.predict_batch(images, score_threshold=0.0, track=tracker):
            assert (o['track_hits'] == c + 1).all() and len(o['track_ids']) >= 3


def test_track_frames_command_line(cuda, models, tmp_path):
    """python -m multiposenet_amd.track_frames over five copies of one frame (PNG files: the pixels of the batch tests, through
    Pillow and predict_images), batches of two: two full batches and a short one at its own size; a video that stands still
    keeps every id."""
    import io
    import json
    from PIL import Image
    from multiposenet_amd import track_frames
    buf = io.BytesIO()
    Image.fromarray(_images()[0]).save(buf, "PNG")
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in (3, 1, 4, 0, 2):
        (frames / f"frame_{i:03d}.png").write_bytes(buf.getvalue())
    (frames / "notes.txt").write_text("not a frame")
    out = tmp_path / "tracks.jsonl"
    paths = models["paths"]
    state = track_frames.main(["--images", str(frames), "--out", str(out), "--model", paths["k"], "--detector", paths["d"],
                               "--prn", paths["p"], "--size", str(W), str(H), "--batch", "2", "--dtype", "f32",
                               "--similarity", "iou", "--score-threshold", "0.0"])
    lines = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert [ln["name"] for ln in lines] == [f"frame_{i:03d}.png" for i in range(5)]
    n = len(lines[0]["ids"])
    assert n >= 3 and all(ln["ids"] == list(range(1, n + 1)) for ln in lines)
    assert np.asarray(lines[0]["boxes"]).shape == (n, 4) and np.asarray(lines[0]["keypoints"]).shape == (n, 17, 3)
    assert state["next_id"] == n + 1 and (state["hits"] == 5).all() and state["dropped"] == 0
