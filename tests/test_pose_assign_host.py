"""CPU: the reference of mpn_pose_track_optimal (tests/track_assign_ref.py) - that its assignment is an optimum (brute force,
scipy), its invariants, the chain on which greedy matching hands every id on, its agreement with the greedy reference where
that is already optimal, the decision margins the GPU comparison relies on - and the entry point's argument checks, which
run before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_assign_cases as acases
import track_assign_ref as opt
import track_cases as cases
import track_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = (1, 3, 4, 12)


def _random_problems(count=240, seed=5):
    """(n, T, {(d, t): weight}) of seeded gated problems up to 7 x 7: a third with weights from three values (heavy ties), a
    third dense, a third sparse."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        n, T = rng.randint(1, 8), rng.randint(1, 8)
        density = (0.9, 0.4, 0.7)[k % 3]
        w = {}
        for d in range(n):
            for t in range(T):
                if rng.rand() < density:
                    w[d, t] = int(rng.choice([300001, 300002, 700001])) if k % 3 == 2 else int(rng.randint(1, (1 << 20) + 2))
        out.append((n, T, w))
    return out


def _solve(n, T, w):
    cost = {(d + 1, t + 1): -v for (d, t), v in w.items()}
    for d in range(n):
        cost[d + 1, T + d + 1] = 0
    p = opt.assign(cost, n, T)
    pairs = [(p[j] - 1, j - 1) for j in range(1, T + 1) if p[j] != 0]
    rows_on = sorted(p[j] for j in range(1, T + n + 1) if p[j] != 0)
    assert rows_on == list(range(1, n + 1))                         # every row sits on exactly one column
    assert all(pair in w for pair in pairs)                         # and only on an eligible one
    return sum(w[pair] for pair in pairs)


def _brute_force(n, T, w):
    def best(d, used):
        if d == n:
            return 0
        value = best(d + 1, used)                                   # detection d unmatched
        for t in range(T):
            if (d, t) in w and not (used >> t) & 1:
                value = max(value, w[d, t] + best(d + 1, used | 1 << t))
        return value
    return best(0, 0)


def test_the_assignment_is_an_optimum():
    problems = _random_problems()
    assert len(problems) >= 200 and sum(1 for n, T, w in problems if len(set(w.values())) < len(w)) >= 60
    for n, T, w in problems:
        assert _solve(n, T, w) == _brute_force(n, T, w), (n, T, w)


def test_the_assignment_equals_scipy_on_the_padded_matrix():
    optimize = pytest.importorskip('scipy.optimize')
    for n, T, w in _random_problems():
        big = (n + 1) * ((1 << 20) + 2)                             # an absent pair: never part of a minimum
        c = np.full((n, T + n), big, np.int64)
        for (d, t), v in w.items():
            c[d, t] = -v
        c[np.arange(n), T + np.arange(n)] = 0
        r, col = optimize.linear_sum_assignment(c)
        assert -int(c[r, col].sum()) == _solve(n, T, w), (n, T, w)


def test_quantum():
    assert opt.quantum(0.0) == 0 and opt.quantum(1.0) == 1 << 20 and opt.quantum(1.5) == 1 << 20 and opt.quantum(-0.25) == 0
    assert opt.quantum(0.3) == 314572 and opt.quantum(np.nextafter(0.5, 0)) == (1 << 19) - 1 and opt.quantum(0.5) == 1 << 19


def _check_frame(name, before, o, rows, p):
    """Matched pairs are eligible and no slot is matched twice."""
    n = len(o['scores'])
    boxes, _, kps = ref._arrays(o)
    taken = [int(s) for s, new in zip(rows['slots'], rows['track_new']) if s >= 0 and not new]
    assert len(taken) == len(set(taken)), name
    all_slots = [int(s) for s in rows['slots'] if s >= 0]
    assert len(all_slots) == len(set(all_slots)), name
    thr = np.float64(np.float32(p.match_threshold))
    for d in range(n):
        t = int(rows['slots'][d])
        if t < 0 or rows['track_new'][d]:
            assert rows['track_similarity'][d] == 0.0
            continue
        assert before.id[t] != 0 and rows['track_ids'][d] == before.id[t], name
        s = (np.float64(ref.iou(before.data[t, :4], boxes[d])) if p.similarity == 'iou'
             else ref.oks(before.data[t, 5:].reshape(17, 3), kps[d]))
        assert s >= thr and rows['track_similarity'][d] == s, name


def test_matched_pairs_are_eligible_and_slots_distinct():
    import copy
    for name, max_tracks, _, thr, frames in acases.iou_cases():
        p = acases.iou_params(max_tracks, thr)
        state = opt.new_state(1, max_tracks)
        with np.errstate(invalid='ignore'):
            for o in frames:
                before = copy.deepcopy(state[0])
                _check_frame(name, before, o, opt.step(state[0], o, p), p)
    for name, max_tracks, frames in cases.cases():
        p = cases.params(max_tracks, 'oks')
        state = opt.new_state(1, max_tracks)
        for o in frames:
            before = copy.deepcopy(state[0])
            _check_frame(name, before, o, opt.step(state[0], o, p), p)


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_reference_does_not_depend_on_the_cut(similarity):
    for name, max_tracks, streams in acases.table(1) + acases.table(2):
        rows, packed = acases.table_reference(streams, max_tracks, similarity)
        p = cases.params(max_tracks, similarity)
        for F in CUTS:
            state = opt.new_state(len(streams), max_tracks)
            for at in range(0, cases.FRAMES, F):
                got = opt.run([o for seq in streams for o in seq[at:at + F]], state, p)
                for i, g in enumerate(got):
                    want = rows[i // F][at + i % F]
                    for k in ('track_ids', 'slots', 'track_hits', 'flags'):
                        np.testing.assert_array_equal(g[k], want[k], err_msg=f"{name} F={F} frame {at + i % F} {k}")
                    assert g['track_similarity'].tobytes() == want['track_similarity'].tobytes()
                assert opt.pack_state(state) == packed[at + F - 1], (name, F, at)


def test_the_chain_keeps_its_ids_where_greedy_hands_them_on():
    log = []
    rows, _ = acases.iou_reference('chain16', log=log)
    assert list(rows[0]['track_ids']) == list(range(1, 17)) and list(rows[1]['track_ids']) == list(range(1, 17))
    assert list(rows[1]['track_hits']) == [2] * 16 and not rows[1]['track_new'].any()
    assert opt.longest_path(log) >= 16
    greedy, _ = acases.iou_reference('chain16', ref)
    assert list(greedy[1]['track_ids']) == list(range(2, 17)) + [17]       # the first track lost, the last person a new id
    assert list(greedy[1]['track_new']) == [False] * 15 + [True]


def test_the_long_chain_and_the_crossing():
    """64 in a row: 63 matches to the right-hand neighbour (0.3368 each) outweigh 64 to the own track (0.3299 each); the last
    detection stays unmatched after a search through 49 columns. The 2 x 2 crossing: 0.85 + 0.80 against greedy's 0.90."""
    log = []
    rows, _ = acases.iou_reference('chain64', log=log)
    assert list(rows[1]['slots'][:63]) == list(range(1, 64)) and rows[1]['track_similarity'][63] == 0.0
    assert opt.longest_search(log) == 49
    s = acases.iou_reference('crossing_2x2')[0][1]['track_similarity']
    g = acases.iou_reference('crossing_2x2', ref)[0][1]
    assert 0.84 < s[0] < 0.86 and 0.79 < s[1] < 0.81 and list(acases.iou_reference('crossing_2x2')[0][1]['track_ids']) == [2, 1]
    assert 0.89 < g['track_similarity'][0] < 0.91 and list(g['track_ids']) == [1, 3] and list(g['track_new']) == [False, True]


def test_the_cases_exercise_what_they_are_there_for():
    rows, _ = acases.iou_reference('more_and_fewer')
    assert sorted(rows[1]['track_ids']) == [1, 2, 3, 4, 5] and list(rows[2]['track_ids']) == [4, 1]
    rows, _ = acases.iou_reference('all_below')
    assert list(rows[1]['track_ids']) == [4, 5, 6] and list(rows[2]['track_ids']) == [4, 5, 6]
    rows, _ = acases.iou_reference('empty_frame')
    assert len(rows[1]['track_ids']) == 0 and list(rows[2]['track_ids']) == [2, 1] and list(rows[2]['track_hits']) == [2, 2]
    rows, _ = acases.iou_reference('nan_box')
    assert list(rows[1]['track_ids']) == [1, 4, 3] and list(rows[2]['track_ids']) == [1, 2, 3]      # the NaN box matches nothing
    rows, _ = acases.iou_reference('equal_boxes')
    assert list(rows[1]['track_ids']) == [1, 2, 3, 4, 5, 6] and set(rows[1]['track_similarity']) == {1.0}
    assert sorted(rows[2]['track_ids']) == [1, 2, 3, 4] and sorted(rows[3]['track_ids']) == [1, 2, 3, 4, 5, 6, 7]
    assert rows[3]['track_new'].sum() == 1 and set(rows[3]['track_similarity']) == {0.0, 1.0}
    log = []
    rows, _ = acases.iou_reference('random64', log=log)
    assert opt.longest_path(log) >= 4 and opt.longest_search(log) >= 8             # not a case greedy would solve
    greedy, _ = acases.iou_reference('random64', ref)
    assert any(list(a['track_ids']) != list(b['track_ids']) for a, b in zip(rows, greedy))


@pytest.mark.parametrize("similarity", ["iou", "oks"])
def test_agrees_with_greedy_where_greedy_is_optimal_and_untied(similarity):
    for name in ('drift', 'absent_max_misses', 'absent_one_more'):
        _, max_tracks, frames = next(c for c in cases.cases() if c[0] == name)
        rows, packed = acases.table_reference([frames], max_tracks, similarity)
        want, want_packed = cases.reference([frames], max_tracks, similarity)
        assert packed == want_packed, name
        for g, w in zip(rows[0], want[0]):
            for k in ('track_ids', 'slots', 'track_hits', 'flags'):
                np.testing.assert_array_equal(g[k], w[k], err_msg=f"{name} {k}")
            assert g['track_similarity'].tobytes() == w['track_similarity'].tobytes()


def test_oks_inputs_of_the_gpu_tests_are_decided():
    """No threshold comparison within a relative 1e-9 and no quantum within 1e-6 of an integer (the device's exp is within 1 ulp:
    a few 1e-16 of a similarity, 1e-10 of a quantum), except a similarity of exactly 1.0 from byte-identical keypoints: the
    kernel builds the same integer problem and, the algorithm being fixed, returns the same assignment."""
    quanta = 0
    for name, max_tracks, streams in acases.table(1) + acases.table(2):
        log = []
        acases.table_reference(streams, max_tracks, 'oks', log=log)
        assert len(log) > 20 and opt.undecided(log) == [], name
        quanta += sum(1 for e in log if e[0] == 'quantum')
    assert quanta > 200
    for max_tracks in (64, 40):
        log = []
        acases.crowd_reference(max_tracks, 'oks', log=log)
        assert opt.undecided(log) == []
    assert opt.undecided([('quantum', 5.0 + 1e-7, 1e-7, False)]) and not opt.undecided([('quantum', float(1 << 20), 0.0, True)])
    assert opt.undecided([('threshold', 0.3, 0.3 + 1e-11, False)]) and not opt.undecided([('threshold', 0.31, 0.3, False)])


def test_argument_checks_need_no_gpu():
    from multiposenet_amd import _lib
    P = lambda a=0: ctypes.c_void_p(4096 + a)

    def call(record=P(), B=4, max_boxes=8, streams=2, max_tracks=8, similarity=0, max_misses=2, prev=P(), next=P(1024), out=P(2048)):
        _lib.call("mpn_pose_track_optimal", record, B, max_boxes, streams, max_tracks, similarity, 0.3, 0.3, max_misses, prev, next,
                  out, None)
    for null in ('record', 'prev', 'next', 'out'):
        with pytest.raises(ValueError, match="BAD_ARG.*pose_track_optimal: null pointer"):
            call(**{null: None})
    for bad in ({'streams': 0}, {'streams': 3}, {'B': 0, 'streams': 1}, {'max_tracks': 0}, {'max_tracks': 65}, {'max_boxes': 0},
                {'max_boxes': 65}, {'B': 128, 'max_boxes': 64}, {'similarity': 2}, {'similarity': -1}, {'max_misses': -1}):
        with pytest.raises(ValueError, match="BAD_SHAPE.*pose_track_optimal:"):
            call(**bad)
    for bad in ({'record': P(8)}, {'prev': P(4)}, {'next': P(1028)}, {'out': P(2052)}):
        with pytest.raises(ValueError, match="BAD_ALIGN.*pose_track_optimal:"):
            call(**bad)
    with pytest.raises(ValueError, match="BAD_ARG.*pose_track_optimal:.*pure function"):
        call(next=P())
    # the same order as mpn_pose_track: the first failing check names the error
    with pytest.raises(ValueError, match="BAD_SHAPE.*whole number of frames"):
        call(streams=3, max_tracks=65, record=P(8))
    with pytest.raises(ValueError, match="BAD_ARG.*pose_track: null pointer"):     # the greedy entry keeps its own prefix
        _lib.call("mpn_pose_track", None, 4, 8, 2, 8, 0, 0.3, 0.3, 2, P(), P(1024), P(2048), None)


def test_tracker_assignment_keyword():
    import inspect
    from multiposenet_amd import tracking
    from multiposenet_amd.tracking import PoseTracker
    parameters = inspect.signature(PoseTracker).parameters
    assert list(parameters)[-1] == 'assignment' and parameters['assignment'].default == 'greedy'
    assert tracking.ASSIGNMENTS == {'greedy': 'mpn_pose_track', 'optimal': 'mpn_pose_track_optimal'}
    for bad in ('best', 'hungarian', None, 1):
        with pytest.raises(ValueError, match="assignment"):
            PoseTracker(assignment=bad)
    with pytest.raises(ValueError):
        PoseTracker(assignment='optimal', max_tracks=65)


def test_track_frames_has_the_switch(capsys):
    from multiposenet_amd import track_frames
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--help"])
    assert e.value.code == 0 and "--assignment" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--images", ".", "--assignment", "best"])
    assert e.value.code == 2


def test_the_entry_has_the_greedy_entrys_signature():
    from multiposenet_amd import _lib
    assert _lib.SIGNATURES["mpn_pose_track_optimal"] == _lib.SIGNATURES["mpn_pose_track"]
    assert hasattr(_lib.lib(), "mpn_pose_track_optimal")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    decl = {}
    for name in ("mpn_pose_track", "mpn_pose_track_optimal"):
        m = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        decl[name] = " ".join(m.group(1).split())
    assert decl["mpn_pose_track"] == decl["mpn_pose_track_optimal"]
