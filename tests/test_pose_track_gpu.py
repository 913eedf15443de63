"""GPU: mpn_pose_track through tracking.PoseTracker against the plain-loop reference (tests/track_ref.py) over the case table
(tests/track_cases.py): every case as one stream and the cases paired as two streams, cut into calls of 1, 3, 4 and 12 frames,
for both similarities; the launch's purity; `update` and `reset`."""
import numpy as np
import pytest

import track_cases as cases
import track_ref as ref

pytestmark = pytest.mark.gpu

CUTS = (1, 3, 4, 12)


def _tracker(streams, max_tracks, similarity, max_boxes=cases.MAX_BOXES):
    from multiposenet_amd.tracking import PoseTracker
    return PoseTracker(streams, max_tracks, similarity, cases.MATCH_THRESHOLD, cases.MAX_MISSES, cases.NEW_TRACK_SCORE, max_boxes)


def _table(streams):
    return [(name, mt, [frames]) for name, mt, frames in cases.cases()] if streams == 1 else cases.pairs()


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
        else:                                                       # a mean of 17 float64 exp values, each within 1 ulp: a few
            np.testing.assert_allclose(r['similarity'], w['track_similarity'], rtol=1e-12, atol=0,     # 1e-16 relative; slack
                                       err_msg=f"{msg} image {i} similarity")
        s += n
    assert not out[s * tracking._OUT.itemsize:].any(), f"{msg}: rows behind the total"


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_kernel_equals_the_reference(cuda, similarity, streams):
    """id / slot / hits / flags equal, the `next` state byte-equal to the reference's packed state (integers and copied float32
    data: exact for OKS too; tests/test_pose_track_host.py asserts that no OKS decision is within 1e-9 of flipping)."""
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    for name, max_tracks, seqs in _table(streams):
        rows, packed = cases.reference(seqs, max_tracks, similarity)
        for F in CUTS:
            b = streams * F
            tracker = _tracker(streams, max_tracks, similarity)
            out_dev = torch.zeros(tracker.out_bytes(b), dtype=torch.uint8, device=cuda)
            for at in range(0, cases.FRAMES, F):
                record, counts = fill_record([o for seq in seqs for o in seq[at:at + F]], b, cases.MAX_BOXES)
                record_dev = torch.from_numpy(record).to(cuda)
                out_dev.fill_(255)                                  # rows behind the record's total must come back zero
                tracker.launch(record_dev, out_dev, b)
                msg = f"{name} {similarity} F={F} frames {at}..{at + F - 1}"
                want = [rows[i // F][at + i % F] for i in range(b)]
                _compare_rows(out_dev.cpu().numpy(), counts, want, similarity, msg)
                assert tracker.next.cpu().numpy().tobytes() == packed[at + F - 1], f"{msg}: next state"
                tracker.commit()
            assert tracker.prev.cpu().numpy().tobytes() == packed[-1]


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_launch_is_pure(cuda, similarity):
    """Two launches without a commit give the same bytes, and neither writes `prev`: the Detector's first call of an entry
    runs its device side eagerly and then replays the captured graph."""
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    name, max_tracks, seqs = cases.pairs()[3]                       # four slots, six persons: births, frees and overflow
    F, b = 4, 8
    tracker = _tracker(2, max_tracks, similarity)
    out_dev = torch.zeros(tracker.out_bytes(b), dtype=torch.uint8, device=cuda)
    for at in (0, 4, 8):
        record, _ = fill_record([o for seq in seqs for o in seq[at:at + F]], b, cases.MAX_BOXES)
        record_dev = torch.from_numpy(record).to(cuda)
        prev = tracker.prev.cpu().numpy().tobytes()
        tracker.launch(record_dev, out_dev, b)
        first = (out_dev.cpu().numpy().tobytes(), tracker.next.cpu().numpy().tobytes())
        assert tracker.prev.cpu().numpy().tobytes() == prev
        out_dev.fill_(255)
        tracker.launch(record_dev, out_dev, b)
        assert (out_dev.cpu().numpy().tobytes(), tracker.next.cpu().numpy().tobytes()) == first, (name, at)
        assert tracker.prev.cpu().numpy().tobytes() == prev and first[1] != prev
        tracker.commit()
    assert tracker.prev.cpu().numpy().tobytes() == cases.reference(seqs, max_tracks, similarity)[1][-1]


def _crowd(frames=3, columns=8, lines=6):
    """48 persons on a grid, drifting: more than one half-wave of slots and detections, every loop of the kernel more than
    one trip. Image 1000 x 1000; the last person of every line is missing in frame 1."""
    rng = np.random.RandomState(7)
    seq = []
    for f in range(frames):
        dets = [cases.person(80 + 120 * c + 3 * f, 90 + 150 * l + 2 * f, 100, 0.9 - 0.01 * (c + columns * l), rng)
                for l in range(lines) for c in range(columns) if not (f == 1 and c == columns - 1)]
        seq.append(cases._frame(dets))
    return seq


@pytest.mark.parametrize("max_tracks", [64, 40])
@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_crowd_at_the_kernels_limits(cuda, similarity, max_tracks):
    """max_boxes 64 with 48 persons, 64 slots (all tracked) and 40 (8 overflow), three frames in one call."""
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    seq = _crowd()
    p = ref.Params(max_tracks, similarity, cases.MATCH_THRESHOLD, cases.MAX_MISSES, cases.NEW_TRACK_SCORE)
    state, log = ref.new_state(1, max_tracks), []
    want = ref.run(seq, state, p, log)
    if similarity == 'oks':
        assert ref.undecided(log) == []                             # as tests/test_pose_track_host.py asserts for the table
    # 40 slots: 8 persons find none in frame 0, 7 in frame 1 (one of the 8 is away), 8 in frame 2
    assert max(want[0]['track_ids']) == min(48, max_tracks) and state[0].dropped == (23 if max_tracks == 40 else 0)
    tracker = _tracker(1, max_tracks, similarity, max_boxes=64)
    record, counts = fill_record(seq, 3, 64)
    out_dev = torch.full((tracker.out_bytes(3),), 255, dtype=torch.uint8, device=cuda)
    tracker.launch(torch.from_numpy(record).to(cuda), out_dev, 3)
    _compare_rows(out_dev.cpu().numpy(), counts, want, similarity, f"crowd {similarity} {max_tracks}")
    assert tracker.next.cpu().numpy().tobytes() == ref.pack_state(state)


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_update_equals_the_reference(cuda, similarity):
    name, max_tracks, seqs = cases.pairs()[2]
    rows, packed = cases.reference(seqs, max_tracks, similarity)
    tracker = _tracker(2, max_tracks, similarity)
    for at in range(0, cases.FRAMES, 3):
        got = tracker.update([o for seq in seqs for o in seq[at:at + 3]])
        assert len(got) == 6
        for i, g in enumerate(got):
            w = rows[i // 3][at + i % 3]
            assert set(g) == {'track_ids', 'track_hits', 'track_new', 'track_similarity'}
            assert g['track_ids'].dtype == np.int32 and g['track_hits'].dtype == np.int32 and g['track_new'].dtype == bool
            assert g['track_similarity'].dtype == np.float64
            for k in ('track_ids', 'track_hits', 'track_new'):
                np.testing.assert_array_equal(g[k], w[k], err_msg=f"{name} frame {at + i % 3} {k}")
            np.testing.assert_allclose(g['track_similarity'], w['track_similarity'], rtol=1e-12, atol=0)
    assert tracker.prev.cpu().numpy().tobytes() == packed[-1]
    for s in range(2):                                              # tracks(): the live slots of the final state
        t = tracker.tracks(s)
        last = rows[s][-1]
        assert {int(i) for i in last['track_ids'] if i} <= {int(i) for i in t['ids']}
        assert t['next_id'] > max(t['ids']) and t['keypoints'].shape == (len(t['ids']), 17, 3)
    with pytest.raises(ValueError, match="whole number of frames"):
        tracker.update(seqs[0][:3])


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
    with pytest.raises(ValueError, match="stream"):
        tracker.reset(2)
