"""CPU: the properties of the reference of mpn_pose_smooth (tests/smooth_ref.py) that make it a One-Euro filter worth comparing
with, the entry point's size functions and argument checks (before any HIP call), and the Python-side validation."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import smooth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 17


def _rows(ids, slots):
    return {'track_id': np.asarray(ids, np.int32), 'slot': np.asarray(slots, np.int32)}


def _person(rng, scale=300.0, score=0.9):
    kp = np.zeros((K, 3), np.float32)
    kp[:, :2] = rng.uniform(-scale, scale, (K, 2))
    kp[:, 2] = score
    return kp


def test_constant_input_stays_that_constant_bit_for_bit():
    rng = np.random.RandomState(0)
    kp = _person(rng)[None]
    kp[0, 0, :2] = (1e4, -1e-3)
    for p in (ref.Params(), ref.Params(rate=24000 / 1001, min_cutoff=0.05, beta=1.0), ref.Params(min_cutoff=1e6)):
        state = ref.new_state(1, 2)
        for f in range(6):
            (got, vel), state = ref.launch(kp, [1], _rows([5], [1]), state, p)
            assert got.tobytes() == kp.tobytes() and vel.tobytes() == bytes(K * 2 * 4), f
        assert state[0].frames == 6 and (state[0].last[1] == 6).all() and state[0].id[1] == 5


def test_first_sample_is_the_identity_and_the_second_is_not():
    rng = np.random.RandomState(1)
    a, b = _person(rng)[None], _person(rng)[None]
    p = ref.Params()
    (got, vel), state = ref.launch(a, [1], _rows([1], [0]), ref.new_state(1, 1), p)
    assert got.tobytes() == a.tobytes() and not vel.any()
    assert state[0].hat[0, :, :2].tobytes() == a[0, :, :2].tobytes() and (state[0].last[0] == 1).all()
    (got, vel), state = ref.launch(b, [1], _rows([1], [0]), state, p)
    lo, hi = np.minimum(a, b)[..., :2], np.maximum(a, b)[..., :2]
    assert ((got[..., :2] > lo) & (got[..., :2] < hi)).all()        # a low-pass: strictly between the two samples
    assert (np.sign(vel) == np.sign((b - a)[..., :2])).all()
    assert got[..., 2].tobytes() == b[..., 2].tobytes()             # the score is the frame's own


def test_untracked_rows_are_the_identity_and_leave_the_state_alone():
    rng = np.random.RandomState(2)
    p = ref.Params()
    kp = np.stack([_person(rng), _person(rng)])
    (_, _), state = ref.launch(kp, [2], _rows([1, 2], [0, 1]), ref.new_state(1, 2), p)
    before = ref.pack_state(state)
    other = np.stack([_person(rng), _person(rng)])
    for ids, slots in (([0, 0], [0, 1]), ([-3, 0], [1, 0]), ([7, 7], [-1, 2]), ([7, 7], [2 ** 30, -5])):
        (got, vel), after = ref.launch(other, [2], _rows(ids, slots), state, p)
        assert got.tobytes() == other.tobytes() and not vel.any()
        want = copy.deepcopy(state)
        want[0].frames += 1                                         # the frame still counts
        assert ref.pack_state(after) == ref.pack_state(want)
    assert ref.pack_state(state) == before                          # launch does not modify its input


def test_a_low_score_resets_that_joint_only_and_the_threshold_itself_is_kept():
    rng = np.random.RandomState(3)
    p = ref.Params(min_keypoint_score=0.5)
    frames = [_person(rng)[None] for _ in range(4)]
    frames[1][0, 3, 2] = 0.49999997                                 # the float32 below 0.5
    frames[1][0, 4, 2] = 0.5
    frames[1][0, 5, 2] = np.nan                                     # not >=: rejected
    state = ref.new_state(1, 1)
    outs = []
    for kp in frames:
        (got, vel), state = ref.launch(kp, [1], _rows([1], [0]), state, p)
        outs.append((got, vel))
    got, vel = outs[1]
    for k in (3, 5):
        assert got[0, k].tobytes() == frames[1][0, k].tobytes() and not vel[0, k].any()
    assert vel[0, 4].all() and got[0, 4, :2].tobytes() != frames[1][0, 4, :2].tobytes()
    others = [k for k in range(K) if k not in (3, 5)]
    assert vel[0, others].all()
    got, vel = outs[2]                                              # the next good sample restarts joints 3 and 5: identity
    for k in (3, 5):
        assert got[0, k].tobytes() == frames[2][0, k].tobytes() and not vel[0, k].any()
    assert vel[0, others].all()
    assert outs[3][1].all() and (state[0].last[0] == 4).all()


def test_an_id_change_in_a_slot_resets_all_joints():
    rng = np.random.RandomState(4)
    p = ref.Params()
    a, b, c = (_person(rng)[None] for _ in range(3))
    state = ref.new_state(1, 3)
    for kp in (a, b):
        (_, vel), state = ref.launch(kp, [1], _rows([1], [2]), state, p)
    assert vel.all()
    (got, vel), state = ref.launch(c, [1], _rows([2], [2]), state, p)
    assert got.tobytes() == c.tobytes() and not vel.any()
    assert state[0].id[2] == 2 and (state[0].last[2] == 3).all() and not state[0].id[:2].any()


def test_gaps_count_frames_and_cuts_do_not_matter():
    """A person away for two frames is filtered with gap 3; F = 4 in one launch equals 2 + 2 and 1 + 1 + 1 + 1."""
    rng = np.random.RandomState(5)
    p = ref.Params(beta=0.05)
    persons = [_person(rng) for _ in range(6)]
    # frames: {A, B}, {A}, {}, {B, A}  (B away in frames 2 and 3)
    kp = np.stack([persons[0], persons[1], persons[2], persons[3], persons[4]])
    counts = [2, 1, 0, 2]
    rows = _rows([1, 2, 1, 2, 1], [0, 1, 0, 1, 0])
    (whole, whole_vel), whole_state = ref.launch(kp, counts, rows, ref.new_state(1, 2), p)
    for cut in (2, 1):
        state, at, got, vel = ref.new_state(1, 2), 0, [], []
        for f in range(0, 4, cut):
            n = sum(counts[f:f + cut])
            part = {k: v[at:at + n] for k, v in rows.items()}
            (g, v), state = ref.launch(kp[at:at + n], counts[f:f + cut], part, state, p)
            got.append(g), vel.append(v)
            at += n
        assert np.concatenate(got).tobytes() == whole.tobytes() and np.concatenate(vel).tobytes() == whole_vel.tobytes()
        assert ref.pack_state(state) == ref.pack_state(whole_state)
    # B's second sample: te = 3 / 30
    trace = []
    out, last, hat = ref.joint(persons[3][0], 1, np.array([*persons[1][0, :2], 0, 0], np.float32), 4, p, trace)
    assert np.float32(out[0]) == whole[3, 0, 0] and np.float32(out[2]) == whole_vel[3, 0, 0] and last == 4
    assert np.float32(np.float32(3) / np.float32(30)) in trace


def test_run_by_id_equals_launch_by_slot():
    """The (stream, id)-keyed `run` over result dicts equals the slot-keyed `launch`, slot reuse included."""
    rng = np.random.RandomState(6)
    p = ref.Params(min_keypoint_score=0.3)
    ids = [[1, 2], [1, 2], [3, 2], [3, 0], [3, 2]]                  # track 1 ends, its slot 0 goes to track 3; one untracked row
    slots = [[0, 1], [0, 1], [0, 1], [0, -1], [0, 1]]
    outputs = []
    for f in range(5):
        kp = np.stack([_person(rng, score=rng.choice([0.2, 0.9])) for _ in ids[f]])
        outputs.append({'keypoints': kp, 'track_ids': np.array(ids[f], np.int32)})
    id_state = ref.new_id_state(1)
    by_id = ref.run(outputs[:3], id_state, p) + ref.run(outputs[3:], id_state, p)
    kp = np.concatenate([o['keypoints'] for o in outputs])
    rows = _rows(np.concatenate(ids), np.concatenate(slots))
    (got, vel), state = ref.launch(kp, [2] * 5, rows, ref.new_state(1, 2), p)
    assert np.concatenate([o['keypoints_smoothed'] for o in by_id]).tobytes() == got.tobytes()
    assert np.concatenate([o['keypoint_velocities'] for o in by_id]).tobytes() == vel.tobytes()
    assert id_state.frames == [5] and state[0].frames == 5


def test_size_functions():
    from multiposenet_amd import _lib
    lib = _lib.lib()
    assert lib.mpn_pose_smooth_state_bytes(1, 1) == 16 + 352 and lib.mpn_pose_smooth_state_bytes(3, 64) == 3 * (16 + 64 * 352)
    assert lib.mpn_pose_smooth_state_bytes(0, 8) == 0 and lib.mpn_pose_smooth_state_bytes(1, 0) == 0
    assert lib.mpn_pose_smooth_state_bytes(1, 65) == 0 and lib.mpn_pose_smooth_state_bytes(-1, 8) == 0
    assert lib.mpn_pose_smooth_out_bytes(16, 25) == 16 * 25 * 340 and lib.mpn_pose_smooth_out_bytes(64, 64) == 4096 * 340
    assert lib.mpn_pose_smooth_out_bytes(0, 8) == 0 and lib.mpn_pose_smooth_out_bytes(1, 65) == 0
    assert lib.mpn_pose_smooth_out_bytes(65, 64) == 0 and lib.mpn_pose_smooth_out_bytes(1, 0) == 0
    assert len(ref.pack_state(ref.new_state(3, 7))) == lib.mpn_pose_smooth_state_bytes(3, 7)
    assert len(ref.pack_rows(np.zeros((0, K, 3)), np.zeros((0, K, 2)), 4, 5)) == lib.mpn_pose_smooth_out_bytes(4, 5) == 20 * ref.ROW_BYTES


def test_argument_checks_need_no_gpu():
    from multiposenet_amd import _lib
    P = lambda a=0: ctypes.c_void_p(4096 + a)
    inf, nan = float('inf'), float('nan')

    def call(record=P(), track=P(512), B=4, max_boxes=8, streams=2, max_tracks=8, rate=30.0, min_cutoff=1.0, beta=0.007,
             d_cutoff=1.0, min_score=0.0, prev=P(1024), next=P(2048), out=P(4096)):
        _lib.call("mpn_pose_smooth", record, track, B, max_boxes, streams, max_tracks, rate, min_cutoff, beta, d_cutoff,
                  min_score, prev, next, out, None)
    for null in ('record', 'track', 'prev', 'next', 'out'):
        with pytest.raises(ValueError, match="BAD_ARG.*null pointer"):
            call(**{null: None})
    with pytest.raises(ValueError, match="BAD_ARG.*pure function"):
        call(next=P(1024))
    for name in ('rate', 'min_cutoff', 'd_cutoff'):
        for v in (0.0, -1.0, inf, -inf, nan):
            with pytest.raises(ValueError, match="BAD_ARG.*> 0"):
                call(**{name: v})
    for v in (-1e-9, inf, nan):
        with pytest.raises(ValueError, match="BAD_ARG.*beta"):
            call(beta=v)
    for v in (inf, -inf, nan):
        with pytest.raises(ValueError, match="BAD_ARG.*min_keypoint_score"):
            call(min_score=v)
    for bad in ({'streams': 0}, {'streams': 3}, {'B': 0, 'streams': 1}, {'max_tracks': 0}, {'max_tracks': 65}, {'max_boxes': 0},
                {'max_boxes': 65}, {'B': 128, 'max_boxes': 64}):
        with pytest.raises(ValueError, match="BAD_SHAPE"):
            call(**bad)
    for bad in ({'record': P(8)}, {'track': P(516)}, {'prev': P(1028)}, {'next': P(2052)}, {'out': P(4100)}):
        with pytest.raises(ValueError, match="BAD_ALIGN"):
            call(**bad)


def test_one_euro_parameters_are_validated_and_immutable():
    from multiposenet_amd.inference import OneEuro, PoseTracker     # exported beside PoseTracker
    from multiposenet_amd import tracking
    assert OneEuro is tracking.OneEuro and PoseTracker is tracking.PoseTracker
    p = OneEuro()
    assert p.astuple() == (30.0, 1.0, float(np.float32(0.007)), 1.0, 0.0)
    assert OneEuro(beta=0).beta == 0.0 and OneEuro(min_keypoint_score=-1).min_keypoint_score == -1.0
    assert OneEuro(rate=25) == OneEuro(rate=25.0) and OneEuro(rate=25) != p and hash(OneEuro()) == hash(p)
    with pytest.raises(AttributeError):
        p.rate = 60.0
    inf, nan = float('inf'), float('nan')
    for bad in ({'rate': 0}, {'rate': -30}, {'rate': inf}, {'rate': nan}, {'min_cutoff': 0}, {'min_cutoff': nan}, {'d_cutoff': 0},
                {'d_cutoff': -inf}, {'beta': -0.1}, {'beta': inf}, {'beta': nan}, {'min_keypoint_score': nan},
                {'min_keypoint_score': inf}, {'rate': 1e39}, {'rate': 'fast'}, {'rate': 1e-46}):
        with pytest.raises(ValueError, match="OneEuro"):
            OneEuro(**bad)


def test_tracker_arguments_are_checked_before_any_device_work():
    from multiposenet_amd.tracking import OneEuro, PoseTracker
    for smooth in (True, 1.0, 'one-euro', {'rate': 30}):
        with pytest.raises(ValueError, match="smooth"):
            PoseTracker(smooth=smooth)
    for bad in ({'similarity': 'cosine'}, {'streams': 0}, {'max_tracks': 65}, {'max_boxes': 65}):
        with pytest.raises(ValueError):
            PoseTracker(smooth=OneEuro(), **bad)
    from multiposenet_amd import tracking
    assert tracking._SMOOTH_OUT.itemsize == ref.ROW_BYTES == 340
    assert tracking._SMOOTH_HEAD.itemsize == 16 and tracking._SMOOTH_SLOT.itemsize == 352


def test_header_declares_and_lib_binds_the_symbols():
    from multiposenet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in ("mpn_pose_smooth_state_bytes", "mpn_pose_smooth_out_bytes", "mpn_pose_smooth"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["mpn_pose_smooth"][1]) == 15
