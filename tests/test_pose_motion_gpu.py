"""GPU: mpn_pose_track_motion through tracking.PoseTracker(motion=ConstantVelocity(...)) against the plain-loop reference
(tests/track_motion_ref.py) on the cases of tests/track_motion_cases.py, both assignments and both similarities: the track
rows (ids, slots, hits and flags equal; the similarity equal under IoU - float32 arithmetic that is the same on both sides -
and within 1e-12 under OKS), and the track state, the motion state and the coasting rows byte for byte
(tests/test_pose_motion_host.py asserts that no OKS decision of these inputs is close to flipping). Every case runs as one
launch over all its frames and as one launch per frame. Purity, velocity_gain = 0 against the entries without motion,
`update`, `tracks` and `reset`."""
import numpy as np
import pytest

import track_motion_cases as mc
import track_motion_ref as mref

pytestmark = pytest.mark.gpu


def _tracker(c, similarity, assignment, gain=None, damping=None, motion=True, **kw):
    from multiposenet_amd.tracking import ConstantVelocity, PoseTracker
    cv = ConstantVelocity(c.gain if gain is None else gain, c.damping if damping is None else damping) if motion else None
    return PoseTracker(len(c.seqs), c.max_tracks, similarity, c.match_threshold, c.max_misses, mc.NEW_TRACK_SCORE, c.max_boxes,
                       motion=cv, assignment=assignment, **kw)


def _compare_rows(tracker, out, counts, want, similarity, msg):
    """The raw output rows of one call against the reference's rows of its images; rows behind the total are zero; the
    coasting rows byte for byte."""
    from multiposenet_amd import tracking
    rows = out[:tracker.track_bytes(len(counts))].view(tracking._OUT)
    s = 0
    for i, (n, w) in enumerate(zip(counts, want)):
        r = rows[s:s + n]
        assert n == len(w['track_ids'])
        for field, key in (('track_id', 'track_ids'), ('slot', 'slots'), ('hits', 'track_hits'), ('flags', 'flags')):
            np.testing.assert_array_equal(r[field], w[key], err_msg=f"{msg} image {i} {key}")
        if similarity == 'iou':
            assert r['similarity'].tobytes() == w['track_similarity'].tobytes(), f"{msg} image {i} similarity"
        else:
            np.testing.assert_allclose(r['similarity'], w['track_similarity'], rtol=1e-12, atol=0,
                                       err_msg=f"{msg} image {i} similarity")
        s += n
    assert not out[s * tracking._OUT.itemsize:tracker.track_bytes(len(counts))].any(), f"{msg}: rows behind the total"
    if tracker.motion is not None:
        at = tracker.coast_offset(len(counts))
        assert out[at:].tobytes() == mref.pack_coast(want, tracker.max_tracks), f"{msg}: coasting rows"


def _launch(tracker, outputs, b, cuda):
    """One launch over b result dicts on a poisoned `out`: (out bytes, counts, next bytes, motion_next bytes); `prev` and
    `motion_prev` must not move."""
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    record, counts = fill_record(outputs, b, tracker.max_boxes)
    out_dev = torch.full((tracker.out_bytes(b),), 255, dtype=torch.uint8, device=cuda)
    prev = tracker.prev.cpu().numpy().tobytes()
    motion_prev = tracker.motion_prev.cpu().numpy().tobytes() if tracker.motion is not None else None
    tracker.launch(torch.from_numpy(record).to(cuda), out_dev, b)
    out = out_dev.cpu().numpy()
    assert tracker.prev.cpu().numpy().tobytes() == prev, "the launch wrote prev"
    motion_next = None
    if tracker.motion is not None:
        assert tracker.motion_prev.cpu().numpy().tobytes() == motion_prev, "the launch wrote motion_prev"
        motion_next = tracker.motion_next.cpu().numpy().tobytes()
    return out, counts, tracker.next.cpu().numpy().tobytes(), motion_next


@pytest.mark.parametrize("name,similarity,assignment", mc.combos())
def test_cases_equal_the_reference(cuda, name, similarity, assignment):
    """One launch over all frames (F = the sequence's length per stream), then one launch per frame with a commit between."""
    c = mc.case(name)
    want = mc.reference(name, similarity, assignment)
    streams, F = len(c.seqs), len(c.seqs[0])
    tracker = _tracker(c, similarity, assignment)
    out, counts, nxt, motion = _launch(tracker, [o for seq in c.seqs for o in seq], streams * F, cuda)
    _compare_rows(tracker, out, counts, [r for s in range(streams) for r in want.rows[s]], similarity, f"{name} one launch")
    assert nxt == want.packed[-1], f"{name}: next state"
    assert motion == want.motion[-1], f"{name}: next motion state"
    tracker = _tracker(c, similarity, assignment)
    for f in range(F):
        out, counts, nxt, motion = _launch(tracker, [seq[f] for seq in c.seqs], streams, cuda)
        _compare_rows(tracker, out, counts, [want.rows[s][f] for s in range(streams)], similarity, f"{name} frame {f}")
        assert nxt == want.packed[f], f"{name} frame {f}: next state"
        assert motion == want.motion[f], f"{name} frame {f}: next motion state"
        tracker.commit()
    assert tracker.motion_prev.cpu().numpy().tobytes() == want.motion[-1]


@pytest.mark.parametrize("assignment", mc.ASSIGNMENTS)
@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_launch_is_pure(cuda, similarity, assignment):
    """Two launches without a commit give the same bytes, and neither writes `prev` or `motion_prev` (`_launch` asserts it)."""
    name = 'table_crowd_of_six+entrants'                            # two streams, four slots: births, frees and overflow
    c = mc.case(name)
    want = mc.reference(name, similarity, assignment)
    tracker = _tracker(c, similarity, assignment)
    for at in (0, 4, 8):
        outputs = [o for seq in c.seqs for o in seq[at:at + 4]]
        before = (tracker.prev.cpu().numpy().tobytes(), tracker.motion_prev.cpu().numpy().tobytes())
        first = _launch(tracker, outputs, 8, cuda)
        second = _launch(tracker, outputs, 8, cuda)
        assert first[0].tobytes() == second[0].tobytes() and first[2:] == second[2:], (name, at)
        assert first[2] != before[0] and first[3] != before[1], (name, at)
        tracker.commit()
    assert tracker.prev.cpu().numpy().tobytes() == want.packed[-1] and tracker.motion_prev.cpu().numpy().tobytes() == want.motion[-1]


@pytest.mark.parametrize("assignment", mc.ASSIGNMENTS)
@pytest.mark.parametrize("name,similarity", [('occlusion', 'iou'), ('crossing_dropout', 'oks'), ('table_crowd_of_six+entrants', 'oks'),
                                             ('random64', 'iou'), ('crowd40', 'oks')])
def test_gain_zero_gives_the_plain_entrys_bytes(cuda, name, similarity, assignment):
    """velocity_gain = 0 on the device: the track rows and the track state of the entry without motion, byte for byte."""
    c = mc.case(name)
    b = len(c.seqs) * len(c.seqs[0])
    outputs = [o for seq in c.seqs for o in seq]
    moving = _tracker(c, similarity, assignment, gain=0.0)
    plain = _tracker(c, similarity, assignment, motion=False)
    assert plain.motion is None and plain.out_bytes(b) == plain.track_bytes(b)
    got, want = _launch(moving, outputs, b, cuda), _launch(plain, outputs, b, cuda)
    n = plain.track_bytes(b)
    assert got[0][:n].tobytes() == want[0].tobytes() and got[2] == want[2]
    slots = np.frombuffer(got[3], np.int32).reshape(len(c.seqs), -1)[:, 4:].reshape(-1, 8)
    assert not slots[:, 2:].any() and slots[:, 0].any()


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_update_and_tracks(cuda, similarity):
    """`update` returns the coasting keys; `tracks` the velocities and the next frame's prediction."""
    c = mc.case('crossing_dropout')
    want = mc.reference('crossing_dropout', similarity, 'greedy')
    tracker = _tracker(c, similarity, 'greedy')
    for at in range(0, 12, 3):
        got = tracker.update(c.seqs[0][at:at + 3])
        for i, g in enumerate(got):
            w = want.rows[0][at + i]
            assert set(g) == {'track_ids', 'track_hits', 'track_new', 'track_similarity', 'coasting_ids', 'coasting_misses',
                              'coasting_boxes', 'coasting_keypoints'}
            for k in ('track_ids', 'track_hits', 'track_new'):
                np.testing.assert_array_equal(g[k], w[k], err_msg=f"frame {at + i} {k}")
            for k in ('coasting_ids', 'coasting_misses', 'coasting_boxes', 'coasting_keypoints'):
                assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and g[k].tobytes() == w[k].tobytes(), (at + i, k)
        if at == 3:                                                 # after frame 5: person 1 hidden for one frame
            state = tracker.tracks(0)
            assert list(state['ids']) == [1, 2] and list(state['misses']) == [1, 0] and list(state['seen']) == [4, 5]
            assert state['velocities'].shape == (2, 6) and list(state['velocities'][:, 4]) == [8.0, -7.5]
            person = mc.person(200.0 + 8.0 * 6, 228.0)              # where frame 6 would show the hidden person
            assert state['keypoints_predicted'][0].tobytes() == person[2][:, :2].tobytes()
            assert state['boxes_predicted'].shape == (2, 4) and state['boxes_predicted'].dtype == np.float32
            np.testing.assert_allclose(state['boxes_predicted'][0], person[0], rtol=0, atol=1e-6)
    assert tracker.prev.cpu().numpy().tobytes() == want.packed[-1]
    assert tracker.motion_prev.cpu().numpy().tobytes() == want.motion[-1]


def test_reset_clears_one_streams_motion_state_only(cuda):
    c = mc.case('table_drift+crossing')
    tracker = _tracker(c, 'iou', 'greedy')
    tracker.update([o for seq in c.seqs for o in seq[:3]])
    before = [tracker.tracks(0), tracker.tracks(1)]
    assert before[0]['velocities'].any() and before[1]['velocities'].any()
    size = tracker.motion_stream_bytes
    motion = tracker.motion_prev.cpu().numpy().copy()
    tracker.reset(1)
    after = tracker.motion_prev.cpu().numpy()
    assert after[:size].tobytes() == motion[:size].tobytes() and not after[size:].any() and motion[size:].any()
    assert not tracker.motion_next.cpu().numpy()[size:].any()
    assert len(tracker.tracks(1)['ids']) == 0 and tracker.tracks(1)['velocities'].shape == (0, 6)
    for k in before[0]:
        np.testing.assert_array_equal(before[0][k], tracker.tracks(0)[k])
    got = tracker.update([seq[3] for seq in c.seqs])
    assert list(got[0]['track_ids']) == [1, 2, 3] and list(got[1]['track_new']) == [True, True]
    tracker.reset()
    assert not tracker.motion_prev.cpu().numpy().any() and not tracker.motion_next.cpu().numpy().any()
    assert not tracker.prev.cpu().numpy().any()


def test_velocities_another_track_left_read_as_zero(cuda):
    """A motion state whose slot ids are not the track state's (here: the track state alone was cleared and filled again) starts
    from nothing, as include/mpn.h states."""
    c = mc.case('occlusion')
    tracker = _tracker(c, 'iou', 'greedy')
    tracker.update(c.seqs[0][:4])
    assert list(tracker.tracks(0)['velocities'][0][:4]) == [0.0, 0.5, 0.0, 0.5]
    tracker.prev.zero_()                                            # id 1 again, in slot 0, at another place
    got = tracker.update([mc.boxes_of([[7.0]])[0], mc.boxes_of([[7.25]])[0]])
    assert list(got[0]['track_ids']) == [1] and list(got[0]['track_new']) == [True]
    assert list(got[1]['track_ids']) == [1] and list(got[1]['track_new']) == [False]       # matched unpredicted
    assert list(tracker.tracks(0)['velocities'][0][:4]) == [0.0, 0.25, 0.0, 0.25]
