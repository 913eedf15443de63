"""GPU: `track=PoseTracker(assignment='optimal')` through the Detector - mpn_pose_track_optimal inside the captured graph -
against the plain-loop reference (tests/track_assign_ref.py) on the returned dicts, next to a greedy tracker on the same
Detector, and `track_frames --assignment optimal`. Image size, variables and score threshold are those of
tests/test_detector_batch_gpu.py."""
import numpy as np
import pytest

import track_assign_ref as opt
import track_ref as ref
from test_detector_batch_gpu import H, W, _detector, _images, models  # noqa: F401 (models: a fixture)

pytestmark = pytest.mark.gpu

TRACK_KEYS = ('track_ids', 'track_hits', 'track_new', 'track_similarity')
MAX_TRACKS = 32


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _tracker(streams, assignment, similarity='oks'):
    from multiposenet_amd.inference import PoseTracker
    return PoseTracker(streams=streams, max_tracks=MAX_TRACKS, similarity=similarity, assignment=assignment)


def _check(calls, streams, similarity, module):
    """The calls' ids, hits and new flags equal `module`'s run on the returned dicts; no OKS decision is close to flipping."""
    p = ref.Params(MAX_TRACKS, similarity, 0.3, 10, 0.3)            # PoseTracker's defaults
    state, log = module.new_state(streams, MAX_TRACKS), []
    for c, outs in enumerate(calls):
        for i, (o, w) in enumerate(zip(outs, module.run(outs, state, p, log))):
            for k in ('track_ids', 'track_hits', 'track_new'):
                np.testing.assert_array_equal(o[k], w[k], err_msg=f"{module.__name__} {similarity} call {c} image {i} {k}")
            if similarity == 'iou':
                assert o['track_similarity'].tobytes() == w['track_similarity'].tobytes()
            else:
                np.testing.assert_allclose(o['track_similarity'], w['track_similarity'], rtol=1e-12, atol=0)
    if similarity == 'oks':
        assert module.undecided(log) == []
    return state


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_optimal_tracker_in_the_captured_graph(det, similarity):
    """Four cameras: the same frames three times, then rotated among the cameras. The first call returns hits == 1 (the eager
    pass and the replay do not step the state twice), the later calls replay one graph; a greedy tracker on the same Detector
    has a graph of its own and returns what the greedy reference gives."""
    images = _images()
    n0 = len(det._graphs)
    optimal, greedy = _tracker(4, 'optimal', similarity), _tracker(4, 'greedy', similarity)
    calls = {'optimal': [], 'greedy': []}
    for c in range(3):
        for name, tracker in (('greedy', greedy), ('optimal', optimal)):
            calls[name].append(det.predict_batch(images, score_threshold=0.0, track=tracker))
        assert len(det._graphs) == n0 + 2
        for g, o in zip(calls['greedy'][-1], calls['optimal'][-1]):
            assert set(o) == set(g) and set(TRACK_KEYS) <= set(o)
            n = len(o['boxes'])
            assert n >= 3 and o['track_ids'].dtype == np.int32 and o['track_similarity'].dtype == np.float64
            np.testing.assert_array_equal(o['track_hits'], np.full(n, c + 1))
            np.testing.assert_array_equal(o['track_ids'], np.arange(1, n + 1))
            assert o['track_new'].all() == (c == 0) and o['track_new'].any() == (c == 0)
            if c:
                np.testing.assert_array_equal(o['track_similarity'], np.ones(n))
    for name, tracker in (('greedy', greedy), ('optimal', optimal)):
        calls[name].append(det.predict_batch(np.roll(images, 1, axis=0), score_threshold=0.0, track=tracker))
    assert len(det._graphs) == n0 + 2
    final = _check(calls['optimal'], 4, similarity, opt)
    assert optimal.prev.cpu().numpy().tobytes() == opt.pack_state(final)
    final = _check(calls['greedy'], 4, similarity, ref)
    assert greedy.prev.cpu().numpy().tobytes() == ref.pack_state(final)


def test_one_stream_of_consecutive_frames(det):
    """One camera, the same frame four times in one call: hits 1..4 inside the call."""
    im = _images()[0]
    batch = det.predict_batch(np.stack([im] * 4), score_threshold=0.0, track=_tracker(1, 'optimal'))
    for f, o in enumerate(batch):
        np.testing.assert_array_equal(o['track_hits'], np.full(len(o['boxes']), f + 1))
        np.testing.assert_array_equal(o['track_ids'], np.arange(1, len(o['boxes']) + 1))


def test_track_frames_command_line(cuda, models, tmp_path):
    """python -m multiposenet_amd.track_frames --assignment optimal over three copies of one frame, batches of two: a video
    that stands still keeps every id."""
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
                               "--similarity", "iou", "--assignment", "optimal", "--score-threshold", "0.0"])
    lines = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert [ln["name"] for ln in lines] == [f"frame_{i:03d}.png" for i in range(3)]
    n = len(lines[0]["ids"])
    assert n >= 3 and all(ln["ids"] == list(range(1, n + 1)) for ln in lines)
    assert state["next_id"] == n + 1 and (state["hits"] == 3).all() and state["dropped"] == 0
