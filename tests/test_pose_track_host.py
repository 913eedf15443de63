"""CPU: the reference of mpn_pose_track (tests/track_ref.py) on the case table (tests/track_cases.py) - hand-written ids, its
invariance to how a sequence is cut into calls, the decision margins the GPU comparison relies on - and the entry point's
argument checks, which run before any HIP call."""
import ctypes

import numpy as np
import pytest

import track_cases as cases
import track_ref as ref

CUTS = (1, 3, 4, 12)


def _case(name):
    return next(c for c in cases.cases() if c[0] == name)


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_hand_written_ids(similarity):
    expected = {
        'drift': [[1, 2, 3]] * 12,
        # the first person is away in frames 4 and 5: two misses, max_misses = 2 - the track survives
        'absent_max_misses': [[1, 2]] * 4 + [[2]] * 2 + [[1, 2]] * 6,
        # away in frames 4, 5 and 6: freed in frame 6, a new id (the third ever given) in the slot it left
        'absent_one_more': [[1, 2]] * 4 + [[2]] * 3 + [[3, 2]] * 5,
    }
    for name, want in expected.items():
        _, max_tracks, frames = _case(name)
        rows, _ = cases.reference([frames], max_tracks, similarity)
        assert [list(r['track_ids']) for r in rows[0]] == want, name
    rows, _ = cases.reference([_case('absent_one_more')[2]], 8, similarity)
    assert list(rows[0][7]['slots']) == [0, 1] and list(rows[0][7]['track_new']) == [True, False]
    assert list(rows[0][11]['track_hits']) == [5, 12]


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_the_scenarios_happen(similarity):
    """What the table is there to exercise does occur in the reference's run of it."""
    def run(name):
        _, max_tracks, frames = _case(name)
        rows, packed = cases.reference([frames], max_tracks, similarity)
        return rows[0], np.frombuffer(packed[-1], np.int32)
    rows, _ = run('crossing')
    assert all(list(r['track_ids']) == [1, 2] for r in rows)
    rows, _ = run('late_empty_weak')
    assert [list(r['track_ids']) for r in rows[1:6]] == [[1], [1, 0], [1, 0], [1, 0], [1, 2]]
    assert len(rows[8]['track_ids']) == 0 and list(rows[9]['track_ids']) == [1, 2] and list(rows[9]['track_hits']) == [9, 4]
    assert not rows[3]['flags'].any()                               # below new_track_score: untracked, no overflow
    rows, state = run('crowd_of_six')
    assert list(rows[0]['track_ids']) == [1, 2, 3, 4, 0, 0] and list(rows[0]['flags']) == [1, 1, 1, 1, 2, 2]
    assert list(rows[5]['track_ids']) == [1, 3, 4, 0, 0]
    assert list(rows[6]['track_ids']) == [1, 3, 4, 5, 0] and list(rows[6]['slots']) == [0, 2, 3, 1, -1]   # freed and reused
    assert state[0] == 6 and state[1] == 4 * 2 + 2 * 2 + 1 + 5      # next_id, dropped
    rows, _ = run('identical')
    assert list(rows[3]['track_ids']) == [1, 2, 3] and list(rows[3]['track_new']) == [False, False, True]
    assert list(rows[4]['track_ids']) == [1, 2, 3] and rows[4]['track_similarity'][0] == rows[4]['track_similarity'][2]
    assert list(rows[5]['track_ids']) == [1, 2] and list(rows[7]['track_ids']) == [1, 2, 3]


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_reference_does_not_depend_on_the_cut(similarity):
    table = [(name, mt, [frames]) for name, mt, frames in cases.cases()] + cases.pairs()
    for name, max_tracks, streams in table:
        rows, packed = cases.reference(streams, max_tracks, similarity)
        p = cases.params(max_tracks, similarity)
        for F in CUTS:
            state = ref.new_state(len(streams), max_tracks)
            for at in range(0, cases.FRAMES, F):
                got = ref.run([o for seq in streams for o in seq[at:at + F]], state, p)
                for i, g in enumerate(got):
                    want = rows[i // F][at + i % F]
                    for k in ('track_ids', 'slots', 'track_hits', 'flags'):
                        np.testing.assert_array_equal(g[k], want[k], err_msg=f"{name} F={F} frame {at + i % F} {k}")
                    assert g['track_similarity'].tobytes() == want['track_similarity'].tobytes()
                assert ref.pack_state(state) == packed[at + F - 1], (name, F, at)


def test_oks_decisions_have_a_margin():
    """Every comparison the reference makes on an OKS is an exact tie of bit-identical inputs or decided by a relative margin
    above 1e-9: the device's exp is within 1 ulp (about 1e-16), so the kernel cannot take another branch."""
    ties = 0
    table = [(name, mt, [frames]) for name, mt, frames in cases.cases()] + cases.pairs()
    for name, max_tracks, streams in table:
        log = []
        cases.reference(streams, max_tracks, 'oks', log)
        assert len(log) > 20, name
        assert ref.undecided(log) == [], name
        ties += sum(1 for kind, a, b, same in log if kind == 'winner' and a == b and same)
    assert ties >= 4                                                # the byte-identical detections do tie


def test_argument_checks_need_no_gpu():
    from multiposenet_amd import _lib
    lib = _lib.lib()
    assert lib.mpn_pose_track_state_bytes(1, 1) == 16 + 240 and lib.mpn_pose_track_state_bytes(3, 64) == 3 * (16 + 64 * 240)
    assert lib.mpn_pose_track_state_bytes(0, 8) == 0 and lib.mpn_pose_track_state_bytes(1, 0) == 0
    assert lib.mpn_pose_track_state_bytes(1, 65) == 0
    assert lib.mpn_pose_track_out_bytes(16, 25) == 16 * 25 * 24 and lib.mpn_pose_track_out_bytes(64, 64) == 4096 * 24
    assert lib.mpn_pose_track_out_bytes(0, 8) == 0 and lib.mpn_pose_track_out_bytes(1, 65) == 0
    assert lib.mpn_pose_track_out_bytes(65, 64) == 0 and lib.mpn_pose_track_out_bytes(1, 0) == 0
    P = lambda a=0: ctypes.c_void_p(4096 + a)

    def call(record=P(), B=4, max_boxes=8, streams=2, max_tracks=8, similarity=0, max_misses=2, prev=P(), next=P(1024), out=P(2048)):
        _lib.call("mpn_pose_track", record, B, max_boxes, streams, max_tracks, similarity, 0.3, 0.3, max_misses, prev, next, out, None)
    for null in ('record', 'prev', 'next', 'out'):
        with pytest.raises(ValueError, match="BAD_ARG.*null pointer"):
            call(**{null: None})
    for bad in ({'streams': 0}, {'streams': 3}, {'B': 0, 'streams': 1}, {'max_tracks': 0}, {'max_tracks': 65}, {'max_boxes': 0},
                {'max_boxes': 65}, {'B': 128, 'max_boxes': 64}, {'similarity': 2}, {'similarity': -1}, {'max_misses': -1}):
        with pytest.raises(ValueError, match="BAD_SHAPE"):
            call(**bad)
    for bad in ({'record': P(8)}, {'prev': P(4)}, {'next': P(1028)}, {'out': P(2052)}):
        with pytest.raises(ValueError, match="BAD_ALIGN"):
            call(**bad)
    with pytest.raises(ValueError, match="BAD_ARG.*pure function"):
        call(next=P())


def test_tracker_arguments_are_checked_before_any_device_work():
    from multiposenet_amd.tracking import PoseTracker
    for bad in ({'similarity': 'cosine'}, {'streams': 0}, {'max_tracks': 65}, {'max_tracks': 0}, {'max_boxes': 65}, {'max_misses': -1}):
        with pytest.raises(ValueError):
            PoseTracker(**bad)
