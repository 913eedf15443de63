"""CPU: the reference of mpn_pose_track_motion (tests/track_motion_ref.py) - the identities it keeps where the trackers without
motion lose them, its equality with `track_ref` / `track_assign_ref` at velocity_gain = 0, its purity and independence of how a
sequence is cut into calls, the decision margins the GPU comparison relies on - and what needs no GPU of the entry point and
its Python front end: argument checks, `ConstantVelocity`, the `PoseTracker` signature, the header's size formulas, the CLI."""
import copy
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import track_motion_cases as mc
import track_motion_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("assignment", mc.ASSIGNMENTS)
def test_occlusion_and_acceleration_keep_the_id(assignment):
    """The id sequences of the two box cases: lost without motion, kept with gain 0.5, lost again with damping 0.5."""
    lost = [1] * 8 + [None] * 3 + [2] * 4
    kept = [1] * 8 + [None] * 3 + [1] * 4
    assert mc.ids_of(mc.plain_reference('occlusion', 'iou', assignment)[0]) == lost
    assert mc.ids_of(mc.reference('occlusion', 'iou', assignment).rows) == kept
    assert mc.ids_of(mc.reference('occlusion_damped', 'iou', assignment).rows) == lost
    assert mc.ids_of(mc.plain_reference('acceleration', 'iou', assignment)[0]) == [1, 1, 1, 2, 3, 4, 5, 6, 7]
    assert mc.ids_of(mc.reference('acceleration', 'iou', assignment).rows) == [1] * 9


@pytest.mark.parametrize("assignment", mc.ASSIGNMENTS)
def test_keypoint_twins_keep_the_id_under_oks(assignment):
    plain = mc.ids_of(mc.plain_reference('occlusion_kp', 'oks', assignment)[0])
    assert plain == [1] * 8 + [None] * 3 + [2] * 4
    assert mc.ids_of(mc.reference('occlusion_kp', 'oks', assignment).rows) == [1] * 8 + [None] * 3 + [1] * 4
    assert max(mc.ids_of(mc.plain_reference('acceleration_kp', 'oks', assignment)[0])) > 1
    assert mc.ids_of(mc.reference('acceleration_kp', 'oks', assignment).rows) == [1] * 9
    # a steady walk on the quarter-pixel grid is predicted byte for byte: the OKS is exactly 1 from the third frame on
    sims = [float(r['track_similarity'][0]) for r in mc.reference('occlusion_kp', 'oks', assignment).rows[0] if len(r['track_ids'])]
    assert sims[0] == 0.0 and 0.3 < sims[1] < 1.0 and set(sims[2:]) == {1.0}


@pytest.mark.parametrize("assignment", mc.ASSIGNMENTS)
@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_crossing_with_a_drop_out(similarity, assignment):
    """The person hidden while the two pass comes back with its id; without motion it comes back as a third person."""
    got = [list(r['track_ids']) for r in mc.reference('crossing_dropout', similarity, assignment).rows[0]]
    assert got == [[1, 2]] * 5 + [[2]] * 2 + [[1, 2]] * 5
    if similarity == 'oks':
        plain = [list(r['track_ids']) for r in mc.plain_reference('crossing_dropout', similarity, assignment)[0][0]]
        assert plain == [[1, 2]] * 5 + [[2]] * 2 + [[3, 2]] * 5


def test_coasting_rows():
    """While the person is hidden the track coasts: one row per frame at 0.5 a frame beyond the last observation."""
    rows = mc.reference('occlusion', 'iou', 'greedy').rows[0]
    for f, r in enumerate(rows):
        if 8 <= f <= 10:
            assert list(r['coasting_ids']) == [1] and list(r['coasting_misses']) == [f - 7]
            assert list(r['coasting_boxes'][0]) == [0.0, 0.5 * f, 1.0, 0.5 * f + 1.0]
            assert r['coasting_keypoints'].shape == (1, 17, 2) and not r['coasting_keypoints'].any()
        else:
            assert len(r['coasting_ids']) == 0 and r['coasting_boxes'].shape == (0, 4)
    packed = mref.pack_coast(rows[8:10], 4)
    assert len(packed) == 2 * 4 * 160 and not any(packed[160:640]) and any(packed[:160])
    # the crossing: the hidden person is reported where it is expected
    rows = mc.reference('crossing_dropout', 'oks', 'greedy').rows[0]
    assert list(rows[5]['coasting_ids']) == [1] and list(rows[6]['coasting_misses']) == [2]
    want = mc.person(200.0 + 8.0 * 6, 228.0)[2][:, :2]
    assert rows[6]['coasting_keypoints'][0].tobytes() == want.tobytes()


def test_freed_slot_is_reused_and_seen_restarts():
    c = mc.case('reuse_slot')
    p = mc.params(c, 'iou', 'greedy')
    state = mref.new_state(1, c.max_tracks)
    seen = []
    for o in c.seqs[0]:
        mref.step(state[0], o, p)
        seen.append((int(state[0].id[1]), int(state[0].seen[1]), float(state[0].vel[1, 1])))
    # slot 1: B (id 2) seen once more, coasting, freed in frame 3 and taken by C (id 3) in that frame with nothing seen
    assert seen[:4] == [(2, 0, 0.0), (2, 1, 0.5), (2, 1, 0.5), (3, 0, 0.0)]
    assert seen[4:] == [(3, 1, -0.375), (3, 2, -0.375), (3, 3, -0.375), (3, 4, -0.375)]
    motion = np.frombuffer(mc.reference('reuse_slot', 'iou', 'greedy').motion[3], np.int32).reshape(-1)
    assert list(motion[:4]) == [0, 0, 0, 0] and list(motion[4:6]) == [1, 3] and list(motion[12:14]) == [3, 0]
    rows = mc.reference('one_slot', 'iou', 'greedy').rows[0]
    assert all(list(r['track_ids']) == [1, 0] and list(r['flags']) == [0 if f else 1, mref.FLAG_OVERFLOW] for f, r in enumerate(rows))


@pytest.mark.parametrize("name,similarity,assignment", mc.combos())
def test_gain_zero_is_the_reference_without_motion(name, similarity, assignment):
    """velocity_gain = 0: rows and packed track state byte for byte those of track_ref / track_assign_ref, every velocity 0."""
    got = mc.reference(name, similarity, assignment, gain=0.0)
    rows, packed = mc.plain_reference(name, similarity, assignment)
    assert got.packed == packed
    for s, seq in enumerate(rows):
        for f, w in enumerate(seq):
            g = got.rows[s][f]
            for k in ('track_ids', 'slots', 'track_hits', 'flags'):
                np.testing.assert_array_equal(g[k], w[k], err_msg=f"{name} frame {f} {k}")
            assert g['track_similarity'].tobytes() == w['track_similarity'].tobytes()
    for m in got.motion:
        slots = np.frombuffer(m, np.int32).reshape(len(rows), -1)[:, 4:].reshape(-1, 8)
        assert not slots[:, 2:].any()


def test_motion_changes_the_multi_person_cases():
    """The table and the crowd are not cases motion leaves alone: some similarity differs from the plain reference's."""
    for name in ('table_drift', 'table_crossing', 'crowd64'):
        got = mc.reference(name, 'oks', 'greedy').rows
        want = mc.plain_reference(name, 'oks', 'greedy')[0]
        assert any(g['track_similarity'].tobytes() != w['track_similarity'].tobytes() for g, w in zip(got[0], want[0])), name


@pytest.mark.parametrize("assignment", mc.ASSIGNMENTS)
def test_reference_is_pure_and_independent_of_the_cut(assignment):
    """`run` over all frames of a stream at once and frame by frame leave the same bytes; a step on a copy of the state leaves
    the original alone."""
    for name in ('occlusion', 'crossing_dropout', 'table_crowd_of_six+entrants'):
        c = mc.case(name)
        similarity = c.similarities[-1]
        p = mc.params(c, similarity, assignment)
        want = mc.reference(name, similarity, assignment)
        state = mref.new_state(len(c.seqs), c.max_tracks)
        before = (mref.pack_state(state), mref.pack_motion(state))
        trial = copy.deepcopy(state)
        rows = mref.run([o for seq in c.seqs for o in seq], trial, p)
        assert (mref.pack_state(state), mref.pack_motion(state)) == before
        assert mref.pack_state(trial) == want.packed[-1] and mref.pack_motion(trial) == want.motion[-1]
        F = len(c.seqs[0])
        for i, g in enumerate(rows):
            w = want.rows[i // F][i % F]
            for k in g:
                assert g[k].tobytes() == w[k].tobytes(), (name, i, k)


def test_oks_inputs_of_the_gpu_tests_are_decided():
    """No OKS decision of a case the GPU test compares exactly is within reach of a last-bit difference in exp (the margins of
    `track_ref.undecided` and `track_assign_ref.undecided`), except a similarity of exactly 1.0 from keypoints that repeat the
    prediction byte for byte. IoU is float32 arithmetic that is the same on both sides: ties are welcome there."""
    checked = 0
    for name, similarity, assignment in mc.combos():
        if similarity != 'oks':
            continue
        log = mc.reference(name, similarity, assignment).log
        assert len(log) >= 8 and mref.undecided(log, assignment) == [], (name, assignment)
        checked += 1
    assert checked >= 2 * 17
    assert mref.undecided([('threshold', 0.3, 0.3 + 1e-11, False)], 'greedy') and mref.undecided([('quantum', 5.0 + 1e-7, 1e-7, False)], 'optimal')


def test_argument_checks_need_no_gpu():
    from multiposenet_amd import _lib
    P = lambda a=0: ctypes.c_void_p(4096 + a)

    def call(record=P(), B=4, max_boxes=8, streams=2, max_tracks=8, similarity=0, assignment=0, max_misses=2, gain=0.5, damping=1.0,
             prev=P(), next=P(1024), motion_prev=P(2048), motion_next=P(3072), out=P(4096), coast=P(8192)):
        _lib.call("mpn_pose_track_motion", record, B, max_boxes, streams, max_tracks, similarity, assignment, 0.3, 0.3, max_misses,
                  gain, damping, prev, next, motion_prev, motion_next, out, coast, None)
    for null in ('record', 'prev', 'next', 'out', 'motion_prev', 'motion_next', 'coast'):
        with pytest.raises(ValueError, match="BAD_ARG.*pose_track_motion: null pointer"):
            call(**{null: None})
    for bad in ({'streams': 0}, {'streams': 3}, {'B': 0, 'streams': 1}, {'max_tracks': 0}, {'max_tracks': 65}, {'max_boxes': 0},
                {'max_boxes': 65}, {'B': 128, 'max_boxes': 64}, {'similarity': 2}, {'similarity': -1}, {'assignment': 2},
                {'assignment': -1}, {'max_misses': -1}):
        with pytest.raises(ValueError, match="BAD_SHAPE.*pose_track_motion:"):
            call(**bad)
    for bad in ({'gain': -0.1}, {'gain': 1.5}, {'gain': float('nan')}, {'gain': float('inf')}, {'damping': -0.5}, {'damping': 1.25},
                {'damping': float('nan')}):
        with pytest.raises(ValueError, match="BAD_ARG.*pose_track_motion: (velocity_gain|damping)"):
            call(**bad)
    for bad in ({'record': P(8)}, {'prev': P(4)}, {'next': P(1028)}, {'out': P(4100)}, {'motion_prev': P(2052)},
                {'motion_next': P(3076)}, {'coast': P(8196)}):
        with pytest.raises(ValueError, match="BAD_ALIGN.*pose_track_motion:"):
            call(**bad)
    with pytest.raises(ValueError, match="BAD_ARG.*pose_track_motion: prev and next.*pure function"):
        call(next=P())
    with pytest.raises(ValueError, match="BAD_ARG.*pose_track_motion: motion_prev and motion_next.*pure function"):
        call(motion_next=P(2048))
    # the order of mpn_pose_track's checks, the new ones in their places: the first failing check names the error
    with pytest.raises(ValueError, match="BAD_SHAPE.*whole number of frames"):
        call(streams=3, max_tracks=65, record=P(8), gain=2.0)
    with pytest.raises(ValueError, match="BAD_SHAPE.*similarity"):
        call(similarity=2, assignment=2)
    with pytest.raises(ValueError, match="BAD_SHAPE.*assignment"):
        call(assignment=2, max_misses=-1)
    with pytest.raises(ValueError, match="BAD_SHAPE.*max_misses"):
        call(max_misses=-1, gain=2.0)
    with pytest.raises(ValueError, match="BAD_ARG.*velocity_gain"):
        call(gain=2.0, damping=2.0, record=P(8))
    with pytest.raises(ValueError, match="BAD_ALIGN.*record"):
        call(record=P(8), coast=P(8196))
    with pytest.raises(ValueError, match="BAD_ALIGN.*coast_out"):
        call(coast=P(8196), next=P())
    with pytest.raises(ValueError, match="BAD_ARG.*prev and next"):
        call(next=P(), motion_next=P(2048))


def test_header_formulas_and_declaration():
    from multiposenet_amd import _lib, tracking
    lib = _lib.lib()
    for streams, max_tracks in ((1, 1), (1, 64), (3, 32), (4096, 7)):
        assert lib.mpn_pose_track_motion_state_bytes(streams, max_tracks) == streams * (16 + 32 * max_tracks)
    for B, max_tracks in ((1, 1), (16, 32), (4096, 64)):
        assert lib.mpn_pose_track_coast_bytes(B, max_tracks) == B * max_tracks * 160
    for bad in ((0, 8), (4097, 8), (1, 0), (1, 65), (-1, 8)):
        assert lib.mpn_pose_track_motion_state_bytes(*bad) == 0 and lib.mpn_pose_track_coast_bytes(*bad) == 0
    assert tracking._COAST.itemsize == mref.COAST.itemsize == 160 and tracking._MOTION_SLOT.itemsize == 32
    assert len(_lib.SIGNATURES["mpn_pose_track_motion"][1]) == 19
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    m = re.search(r"\bint mpn_pose_track_motion\s*\(([^)]*)\)\s*;", text)
    names = [a.split()[-1].lstrip('*') for a in m.group(1).split(',')]
    assert names == ['record', 'B', 'max_boxes', 'streams', 'max_tracks', 'similarity', 'assignment', 'match_threshold',
                     'new_track_score', 'max_misses', 'velocity_gain', 'damping', 'prev', 'next', 'motion_prev', 'motion_next', 'out',
                     'coast_out', 'stream']
    assert _lib.MPN_VERSION == 600


def test_constant_velocity_is_validated_and_immutable():
    from multiposenet_amd.inference import ConstantVelocity
    from multiposenet_amd.tracking import ConstantVelocity as same
    assert ConstantVelocity is same
    cv = ConstantVelocity()
    assert cv.astuple() == (0.5, 1.0) and cv == ConstantVelocity(0.5, 1.0) and hash(cv) == hash(ConstantVelocity(0.5, 1.0))
    assert cv != ConstantVelocity(0.25) and "velocity_gain=0.5" in repr(cv) and "damping=1.0" in repr(cv)
    assert ConstantVelocity(0, 0).astuple() == (0.0, 0.0) and ConstantVelocity(1, 1).astuple() == (1.0, 1.0)
    assert ConstantVelocity(velocity_gain=0.1).velocity_gain == float(np.float32(0.1))         # what the launch receives
    for bad in (dict(velocity_gain=-0.1), dict(velocity_gain=1.1), dict(damping=-1), dict(damping=2), dict(velocity_gain=float('nan')),
                dict(damping=float('inf')), dict(velocity_gain='fast'), dict(damping=None)):
        with pytest.raises(ValueError, match="ConstantVelocity: " + next(iter(bad))):
            ConstantVelocity(**bad)
    with pytest.raises(AttributeError, match="immutable"):
        cv.damping = 0.5
    with pytest.raises(AttributeError, match="immutable"):
        del cv.velocity_gain
    assert "NOT tuned" in ConstantVelocity.__doc__


def test_tracker_motion_keyword():
    from multiposenet_amd import tracking
    from multiposenet_amd.tracking import PoseTracker
    parameters = inspect.signature(PoseTracker).parameters
    names = list(parameters)
    assert parameters['motion'].default is None and names[-1] == 'assignment' and names[-3:] == ['smooth', 'motion', 'assignment']
    assert tracking.ASSIGNMENTS == {'greedy': 'mpn_pose_track', 'optimal': 'mpn_pose_track_optimal'}
    for bad in (0.5, 'cv', tracking.OneEuro(), (0.5, 1.0)):
        with pytest.raises(ValueError, match="motion must be None or a tracking.ConstantVelocity"):
            PoseTracker(motion=bad)


def test_track_frames_has_the_switch(capsys):
    from multiposenet_amd import track_frames
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--help"])
    out = capsys.readouterr().out
    assert e.value.code == 0 and "--motion" in out and "--velocity-gain" in out and "--damping" in out
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--images", ".", "--motion", "--velocity-gain", "1.5"])
    assert e.value.code == 2
