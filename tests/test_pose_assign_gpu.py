"""GPU: mpn_pose_track_optimal through tracking.PoseTracker(assignment='optimal') against the plain-loop reference
(tests/track_assign_ref.py): the box sequences of tests/track_assign_cases.py under IoU (float32 arithmetic, the same on both
sides: rows, `next` bytes and similarities equal), `track_cases`' table and a crowd of 48 under OKS and IoU (tests/
test_pose_assign_host.py asserts that no OKS decision of these inputs is close to flipping); cuts, streams, purity, `update`
and `reset`."""
import numpy as np
import pytest

import track_assign_cases as acases
import track_assign_ref as opt
import track_cases as cases

pytestmark = pytest.mark.gpu

CUTS = (1, 3, 4, 12)


def _tracker(streams, max_tracks, similarity, max_boxes=cases.MAX_BOXES, match_threshold=cases.MATCH_THRESHOLD, **kw):
    from multiposenet_amd.tracking import PoseTracker
    return PoseTracker(streams, max_tracks, similarity, match_threshold, cases.MAX_MISSES, cases.NEW_TRACK_SCORE, max_boxes,
                       assignment='optimal', **kw)


def _compare_rows(out, counts, want, similarity, msg):
    """The raw output rows of one call against the reference's rows of its images; rows behind the total are zero."""
    from multiposenet_amd import tracking
    rows = out.view(tracking._OUT)
    s = 0
    for i, (n, w) in enumerate(zip(counts, want)):
        r = rows[s:s + n]
        assert n == len(w['track_ids'])
        for field, key in (('track_id', 'track_ids'), ('slot', 'slots'), ('hits', 'track_hits'), ('flags', 'flags')):
            np.testing.assert_array_equal(r[field], w[key], err_msg=f"{msg} image {i} {key}")
        if similarity == 'iou':                                     # float32 arithmetic, every operation correctly rounded
            assert r['similarity'].tobytes() == w['track_similarity'].tobytes(), f"{msg} image {i} similarity"
        else:                                                       # a mean of 17 float64 exp values, each within 1 ulp
            np.testing.assert_allclose(r['similarity'], w['track_similarity'], rtol=1e-12, atol=0,
                                       err_msg=f"{msg} image {i} similarity")
        s += n
    assert not out[s * tracking._OUT.itemsize:].any(), f"{msg}: rows behind the total"


def _launch(tracker, outputs, b, max_boxes, cuda):
    """One launch over b result dicts on a poisoned `out`: (out bytes, counts, next bytes); `prev` must not move."""
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    record, counts = fill_record(outputs, b, max_boxes)
    out_dev = torch.full((tracker.out_bytes(b),), 255, dtype=torch.uint8, device=cuda)
    prev = tracker.prev.cpu().numpy().tobytes()
    tracker.launch(torch.from_numpy(record).to(cuda), out_dev, b)
    out = out_dev.cpu().numpy()
    assert tracker.prev.cpu().numpy().tobytes() == prev, "the launch wrote prev"
    return out, counts, tracker.next.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", [c[0] for c in acases.iou_cases()])
def test_box_cases_equal_the_reference(cuda, name):
    """Every case as one launch over all its frames and as one launch per frame."""
    _, max_tracks, max_boxes, thr, frames = next(c for c in acases.iou_cases() if c[0] == name)
    rows, packed = acases.iou_reference(name)
    F = len(frames)
    tracker = _tracker(1, max_tracks, 'iou', max_boxes, thr)
    assert tracker.assignment == 'optimal'
    out, counts, nxt = _launch(tracker, frames, F, max_boxes, cuda)
    _compare_rows(out, counts, rows, 'iou', f"{name} one launch")
    assert nxt == packed[-1], f"{name}: next state"
    tracker = _tracker(1, max_tracks, 'iou', max_boxes, thr)
    for f, o in enumerate(frames):
        out, counts, nxt = _launch(tracker, [o], 1, max_boxes, cuda)
        _compare_rows(out, counts, rows[f:f + 1], 'iou', f"{name} frame {f}")
        assert nxt == packed[f], f"{name} frame {f}: next state"
        tracker.commit()


def test_optimal_differs_from_greedy_on_the_device(cuda):
    """The chain of 16 and the 2 x 2 crossing through both entries: the greedy tracker still hands the ids on."""
    from multiposenet_amd.tracking import PoseTracker
    for name in ('chain16', 'crossing_2x2'):
        _, max_tracks, max_boxes, thr, frames = next(c for c in acases.iou_cases() if c[0] == name)
        got = {}
        for assignment in ('greedy', 'optimal'):
            tracker = PoseTracker(1, max_tracks, 'iou', thr, cases.MAX_MISSES, cases.NEW_TRACK_SCORE, max_boxes, assignment=assignment)
            got[assignment] = [list(o['track_ids']) for o in tracker.update(frames[:2])]
        assert got['optimal'][1] == [int(i) for i in acases.iou_reference(name)[0][1]['track_ids']]
        assert got['greedy'][1] == [int(i) for i in acases.iou_reference(name, acases.ref)[0][1]['track_ids']]
        assert got['greedy'][1] != got['optimal'][1] and got['greedy'][0] == got['optimal'][0]
    assert got['optimal'][1] == [2, 1] and got['greedy'][1] == [1, 3]


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_table_equals_the_reference(cuda, similarity, streams):
    """`track_cases`' table, one stream and paired as two, cut into calls of 1, 3, 4 and 12 frames."""
    for name, max_tracks, seqs in acases.table(streams):
        rows, packed = acases.table_reference(seqs, max_tracks, similarity)
        for F in CUTS:
            b = streams * F
            tracker = _tracker(streams, max_tracks, similarity)
            for at in range(0, cases.FRAMES, F):
                out, counts, nxt = _launch(tracker, [o for seq in seqs for o in seq[at:at + F]], b, cases.MAX_BOXES, cuda)
                msg = f"{name} {similarity} F={F} frames {at}..{at + F - 1}"
                _compare_rows(out, counts, [rows[i // F][at + i % F] for i in range(b)], similarity, msg)
                assert nxt == packed[at + F - 1], f"{msg}: next state"
                tracker.commit()
            assert tracker.prev.cpu().numpy().tobytes() == packed[-1]


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_launch_is_pure(cuda, similarity):
    """Two launches without a commit give the same bytes, and neither writes `prev`."""
    name, max_tracks, seqs = cases.pairs()[3]                       # four slots, six persons: births, frees and overflow
    F, b = 4, 8
    tracker = _tracker(2, max_tracks, similarity)
    for at in (0, 4, 8):
        outputs = [o for seq in seqs for o in seq[at:at + F]]
        prev = tracker.prev.cpu().numpy().tobytes()
        first = _launch(tracker, outputs, b, cases.MAX_BOXES, cuda)
        second = _launch(tracker, outputs, b, cases.MAX_BOXES, cuda)
        assert first[0].tobytes() == second[0].tobytes() and first[2] == second[2] and first[2] != prev, (name, at)
        tracker.commit()
    assert tracker.prev.cpu().numpy().tobytes() == acases.table_reference(seqs, max_tracks, similarity)[1][-1]


@pytest.mark.parametrize("max_tracks", [64, 40])
@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_crowd_at_the_kernels_limits(cuda, similarity, max_tracks):
    """max_boxes 64 with 48 persons, 64 slots (all tracked) and 40 (8 overflow), three frames in one call."""
    want, packed, dropped = acases.crowd_reference(max_tracks, similarity)
    assert max(want[0]['track_ids']) == min(48, max_tracks) and dropped == (23 if max_tracks == 40 else 0)
    if max_tracks == 40:
        assert (want[0]['flags'] == opt.FLAG_OVERFLOW).sum() == 8
    tracker = _tracker(1, max_tracks, similarity, max_boxes=64)
    out, counts, nxt = _launch(tracker, acases.crowd(), 3, 64, cuda)
    _compare_rows(out, counts, want, similarity, f"crowd {similarity} {max_tracks}")
    assert nxt == packed


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_update_equals_the_reference(cuda, similarity):
    name, max_tracks, seqs = cases.pairs()[2]
    rows, packed = acases.table_reference(seqs, max_tracks, similarity)
    tracker = _tracker(2, max_tracks, similarity)
    for at in range(0, cases.FRAMES, 3):
        got = tracker.update([o for seq in seqs for o in seq[at:at + 3]])
        assert len(got) == 6
        for i, g in enumerate(got):
            w = rows[i // 3][at + i % 3]
            assert set(g) == {'track_ids', 'track_hits', 'track_new', 'track_similarity'}
            for k in ('track_ids', 'track_hits', 'track_new'):
                np.testing.assert_array_equal(g[k], w[k], err_msg=f"{name} frame {at + i % 3} {k}")
            np.testing.assert_allclose(g['track_similarity'], w['track_similarity'], rtol=1e-12, atol=0)
    assert tracker.prev.cpu().numpy().tobytes() == packed[-1]


def test_reset_clears_one_stream_only(cuda):
    name, max_tracks, seqs = cases.pairs()[0]
    tracker = _tracker(2, max_tracks, 'iou')
    tracker.update([seqs[0][0], seqs[1][0]])
    before = [tracker.tracks(0), tracker.tracks(1)]
    assert len(before[0]['ids']) == 3 and len(before[1]['ids']) == 2 and before[1]['next_id'] == 3
    tracker.reset(1)
    after = [tracker.tracks(0), tracker.tracks(1)]
    assert len(after[1]['ids']) == 0 and after[1]['next_id'] == 1 and after[1]['dropped'] == 0
    for k in before[0]:
        np.testing.assert_array_equal(before[0][k], after[0][k])
    got = tracker.update([seqs[0][1], seqs[1][1]])
    assert list(got[0]['track_ids']) == [1, 2, 3] and list(got[0]['track_hits']) == [2, 2, 2]
    assert list(got[1]['track_ids']) == [1, 2] and list(got[1]['track_new']) == [True, True]
    tracker.reset()
    assert not tracker.prev.cpu().numpy().any() and not tracker.next.cpu().numpy().any()
