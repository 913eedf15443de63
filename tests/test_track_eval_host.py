"""CPU: the definition of mpn_track_eval (tests/track_eval_ref.py) against brute force, the metric formulas and the package's host
side on the handmade cases, the identity solver against scipy, the PoseTrack reader, the entry's argument checks and ABI sizes."""
import ctypes
import inspect
import json
import math
import os
import re

import numpy as np
import pytest

import track_eval_cases as cases
import track_eval_ref as ref
from track_assign_ref import QUANTA, assign, quantum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_IDENTITIES = 256
BY_NAME = {c['name']: c for c in cases.CASES}


@pytest.fixture(scope="module")
def reference():
    """name -> (results, packed state, log) of the plain-loop definition, computed once."""
    out = {}
    for c in cases.CASES:
        state, log = ref.new_state(c['streams'], MAX_IDENTITIES), []
        results = ref.run(c['outputs'], c['groundtruth'], c['identities'], state, c['threshold'], log)
        out[c['name']] = (results, ref.pack_state(state), log)
    return out


def as_unpacked(case, results):
    """`run`'s results in the shape of `TrackEvaluator.unpack`'s dicts."""
    F = len(results) // case['streams']
    out = []
    for i, r in enumerate(results):
        d = {k: int(r['frame'][k]) for k in ref.FRAME.names[:8]}
        d.update({'similarity_sum': float(r['frame']['similarity_sum']), 'gt_matched': (r['gt']['flags'] & ref.GT_MATCHED) != 0,
                  'gt_ignored': (r['gt']['flags'] & ref.GT_IGNORED) != 0, 'gt_overlaps': r['gt']['overlaps'],
                  'gt_identities': case['identities'][i], 'stream': i // F, 'epoch': 0})
        out.append(d)
    return out


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) < 1e-12


@pytest.mark.parametrize("seed", range(40))
def test_the_assignment_is_cardinality_first_then_the_quantised_sum(seed):
    """Step 2's weights through `track_assign_ref.assign` against every matching of seeded problems up to 6 x 6."""
    rng = np.random.RandomState(seed)
    ng, n = rng.randint(1, 7), rng.randint(1, 7)
    sim = rng.rand(ng, n)
    if seed % 3 == 0:
        sim = np.round(sim * 4) / 4                                 # ties
    thr = 0.4
    cost, weights = {}, {}
    for g in range(ng):
        for h in range(n):
            if sim[g, h] >= thr:
                cost[g + 1, h + 1] = -(quantum(sim[g, h]) + 1 + ref.BIAS)
                weights[g, h] = quantum(sim[g, h])
        cost[g + 1, n + g + 1] = 0
    on = assign(cost, ng, n)
    pairs = [(on[j] - 1, j - 1) for j in range(1, n + 1) if on[j] != 0]
    assert len({g for g, _ in pairs}) == len(pairs) and all(p in weights for p in pairs)
    assert (len(pairs), sum(weights[p] for p in pairs)) == ref.brute_force(weights)


def test_the_bias_outweighs_any_sum_of_quanta():
    assert 64 * (QUANTA + 1) < ref.BIAS


def test_two_by_two_takes_two_pairs_where_the_larger_sum_has_one(reference):
    c = BY_NAME['two_by_two']
    assert c['threshold'] == 0.3
    a, b, far = cases.oks_at(cases.D95), cases.oks_at(cases.D35), cases.oks_at(cases.D95 + 2 * cases.D35)
    assert 0.9 < a < 0.95 and 0.3 < b < 0.35 and far < 0.3 and a > 2 * b
    rows = reference['two_by_two'][0][0]['gt']
    assert rows['row'].tolist() == [1, 0] and abs(rows['similarity'][0] - b) < 1e-12


def test_kept_correspondence_wins_over_the_nearer_track(reference):
    second = reference['kept'][0][1]
    assert second['gt']['flags'][0] == ref.GT_MATCHED | ref.GT_KEPT and second['gt']['track_id'][0] == 1
    assert 0.5 < second['gt']['similarity'][0] < 0.6 and second['hyp']['flags'].tolist() == [ref.HYP_FALSE_POSITIVE, 0]


def test_an_identity_without_memory_stores_nothing(reference):
    results, state, _ = reference['no_memory']
    assert state == ref.pack_state([_frames(ref.Stream(MAX_IDENTITIES), 3)])
    assert all(r['gt']['stored'][0] == 0 and r['gt']['flags'][0] == ref.GT_MATCHED for r in results)


def _frames(stream, n):
    stream.frames = n
    return stream


def test_the_full_frame_sets_bit_63(reference):
    rows = reference['full'][0][0]['gt']
    assert (rows['flags'] == ref.GT_MATCHED).all() and sorted(rows['row'].tolist()) == list(range(64))
    assert int(rows['overlaps'][int(np.nonzero(rows['row'] == 63)[0][0])]) == 1 << 63


def test_streams_keep_their_own_memory(reference):
    one, four = reference['video_1'][0], reference['video_4'][0]
    assert sum(int(r['frame']['switches']) for r in one) > 0
    assert [int(r['gt']['stored'].sum()) for r in four[::4]] == [0, 0, 0, 0]     # every stream starts without memory
    assert any(r1['gt'].tobytes() != r4['gt'].tobytes() for r1, r4 in zip(one, four))


@pytest.mark.parametrize("name", [c['name'] for c in cases.CASES])
def test_no_decision_hangs_on_a_last_bit(reference, name):
    log = reference[name][2]
    assert any(e[0] == 'threshold' for e in log) or name == 'empty_frames'
    assert ref.undecided(log) == []


@pytest.mark.parametrize("name", [c['name'] for c in cases.CASES if c['expect']])
def test_metrics_of_the_handmade_cases(reference, name):
    """The numbers written out by hand in the case table: from the reference's brute definitions, and from the package's
    accumulator (`TrackAccumulator`, the host side of `TrackEvaluator`) fed with the reference's rows."""
    from multiposenet_amd.track_metrics import TrackAccumulator
    c = BY_NAME[name]
    results = reference[name][0]
    acc = TrackAccumulator()
    for rows, o in zip(as_unpacked(c, results), c['outputs']):
        acc.add_image(rows, o['track_ids'])
    got = acc.evaluate()
    brute = ref.metrics(results, c['outputs'], c['identities'], c['streams']) if name != 'full' else got
    for key, value in c['expect'].items():
        assert same(got[key], value), (key, got[key], value)
        assert same(brute[key], value), (key, brute[key], value)
    assert set(got) == set(brute) and all(same(got[k], brute[k]) for k in got)


def test_ratios_with_a_zero_denominator_are_nan():
    from multiposenet_amd.track_metrics import TrackAccumulator
    got = TrackAccumulator().evaluate()
    assert got['num_frames'] == 0 and got['idtp'] == 0
    for key in ('mota', 'motp', 'recall', 'precision', 'idp', 'idr', 'idf1'):
        assert math.isnan(got[key]), key


@pytest.mark.parametrize("seed", range(12))
def test_identity_solver_against_scipy(seed):
    optimize = pytest.importorskip("scipy.optimize")
    from multiposenet_amd.track_metrics import max_weight_matching
    rng = np.random.RandomState(seed)
    rows, cols = rng.randint(1, 14), rng.randint(1, 14)
    weight = rng.randint(0, 6 if seed % 2 else 60, (rows, cols)) * (rng.rand(rows, cols) < 0.6)
    table = {(('s', r), ('t', c)): int(weight[r, c]) for r in range(rows) for c in range(cols) if weight[r, c] > 0}
    r, c = optimize.linear_sum_assignment(weight, maximize=True)
    assert max_weight_matching(table) == int(weight[r, c].sum())
    if rows * cols <= 25:
        assert max_weight_matching(table) == ref.best_identity_matching(table)


def test_identity_solver_needs_no_scipy():
    import multiposenet_amd.track_metrics as tm
    assert 'scipy' not in inspect.getsource(tm)
    assert tm.max_weight_matching({}) == 0 and tm.max_weight_matching({('a', 'x'): 3, ('a', 'y'): 5, ('b', 'y'): 4}) == 7


def test_groundtruth_from_posetrack(tmp_path):
    from multiposenet_amd.track_metrics import groundtruth_from_posetrack, groundtruth_track_ids
    from multiposenet_amd.pose_metrics import groundtruth_arrays
    kp = [float(v) for k in range(17) for v in (10 + k, 20 + k, 2)]
    data = {'images': [{'id': 2, 'file_name': 'b.jpg', 'vid_id': 1, 'frame_id': 1},
                       {'id': 1, 'file_name': 'a.jpg', 'vid_id': 1, 'frame_id': 0},
                       {'id': 3, 'file_name': 'c.jpg', 'vid_id': 0, 'frame_id': 5}],
            'annotations': [{'image_id': 1, 'track_id': 4, 'keypoints': kp, 'bbox': [10, 20, 16, 16], 'area': 200.0},
                            {'image_id': 1, 'track_id': 9, 'keypoints': [0.0] * 51, 'bbox': [50, 50, 10, 10]},
                            {'image_id': 1, 'bbox': [70, 70, 5, 5]},
                            {'image_id': 2, 'track_id': 4, 'keypoints': kp, 'bbox': [10, 20, 16, 16]},
                            {'image_id': 7, 'track_id': 1, 'keypoints': kp, 'bbox': [0, 0, 1, 1]}]}
    path = tmp_path / 'tracks.json'
    path.write_text(json.dumps(data))
    frames = groundtruth_from_posetrack(str(path))
    assert [name for name, _ in frames] == ['c.jpg', 'a.jpg', 'b.jpg']
    a = frames[1][1]
    assert a['track_ids'].tolist() == [4, 9, 10] and a['area'].tolist() == [200.0, 100.0, 25.0]
    assert groundtruth_arrays(a)[4].tolist() == [False, True, True]              # no keypoint with v > 0: an ignore region
    assert groundtruth_track_ids(a, 3) == [4, 9, 10]
    assert len(frames[0][1]['track_ids']) == 0 and frames[2][1]['boxes'].shape == (1, 4)
    for image in data['images']:
        del image['vid_id']
    path.write_text(json.dumps(data))
    assert [name for name, _ in groundtruth_from_posetrack(str(path))] == ['b.jpg', 'a.jpg', 'c.jpg']
    with pytest.raises(ValueError, match="track_ids"):
        groundtruth_track_ids({'keypoints': a['keypoints'], 'boxes': a['boxes']}, 3)
    with pytest.raises(ValueError, match="unique"):
        groundtruth_track_ids(dict(a, track_ids=[1, 1, 2]), 3)


def test_argument_checks_need_no_gpu():
    from multiposenet_amd import _lib
    P = lambda a=0: ctypes.c_void_p(1 << 20 | a)
    big = 1 << 30

    def call(record=P(), track_rows=P(0x100), B=4, max_boxes=8, streams=2, gt=P(0x200), gt_counts=P(0x300), gt_identity=P(0x400),
             max_gt=8, max_identities=16, threshold=0.5, prev=P(0x500), next=P(0x600), state_bytes=big, out=P(0x700),
             out_bytes=big):
        _lib.call("mpn_track_eval", record, track_rows, B, max_boxes, streams, gt, gt_counts, gt_identity, max_gt, max_identities,
                  threshold, prev, next, state_bytes, out, out_bytes, None)
    for null in ('record', 'track_rows', 'gt', 'gt_counts', 'gt_identity', 'prev', 'next', 'out'):
        with pytest.raises(ValueError, match="BAD_ARG.*track_eval: null pointer"):
            call(**{null: None})
    for bad in ({'streams': 0}, {'streams': 3}, {'B': 0, 'streams': 1}, {'max_boxes': 0}, {'max_boxes': 65},
                {'B': 128, 'max_boxes': 64}, {'max_gt': 0}, {'max_gt': 65}, {'max_identities': 0}, {'max_identities': 1025}):
        with pytest.raises(ValueError, match="BAD_SHAPE.*track_eval:"):
            call(**bad)
    with pytest.raises(ValueError, match="BAD_ARG.*track_eval: threshold"):
        call(threshold=float('nan'))
    for bad in ({'record': P(8)}, {'track_rows': P(0x104)}, {'gt': P(0x204)}, {'gt_counts': P(0x302)}, {'gt_identity': P(0x401)},
                {'prev': P(0x504)}, {'next': P(0x604)}, {'out': P(0x704)}):
        with pytest.raises(ValueError, match="BAD_ALIGN.*track_eval:"):
            call(**bad)
    with pytest.raises(ValueError, match="BAD_ARG.*track_eval:.*pure function"):
        call(next=P(0x500))
    lib = _lib.lib()
    with pytest.raises(_lib.MpnError, match="WORKSPACE.*track_eval: state_bytes"):
        call(state_bytes=lib.mpn_track_eval_state_bytes(2, 16) - 1)
    with pytest.raises(_lib.MpnError, match="WORKSPACE.*track_eval: out_bytes"):
        call(out_bytes=lib.mpn_track_eval_out_bytes(4, 8, 8) - 1)
    with pytest.raises(ValueError, match="BAD_SHAPE.*whole number of frames"):   # the first failing check names the error
        call(streams=3, max_gt=65, record=P(8))


def test_abi_sizes():
    from multiposenet_amd import _lib, track_metrics as tm
    lib = _lib.lib()
    assert lib.mpn_track_eval_state_bytes(1, 1) == 20 and lib.mpn_track_eval_state_bytes(3, 1024) == 3 * (16 + 4096)
    for bad in ((0, 4), (4097, 4), (1, 0), (1, 1025)):
        assert lib.mpn_track_eval_state_bytes(*bad) == 0
    assert lib.mpn_track_eval_out_bytes(4, 25, 64) == 4 * (48 + 64 * 32 + 25 * 8)
    assert lib.mpn_track_eval_out_bytes(1, 1, 1) == 48 + 32 + 8
    for bad in ((0, 8, 8), (4, 0, 8), (4, 65, 8), (128, 64, 8), (4, 8, 0), (4, 8, 65)):
        assert lib.mpn_track_eval_out_bytes(*bad) == 0
    assert (tm._FRAME.itemsize, tm._GT.itemsize, tm._HYP.itemsize) == (48, 32, 8)
    assert tm._FRAME == ref.FRAME and tm._GT == ref.GT and tm._HYP == ref.HYP
    assert len(_lib.SIGNATURES["mpn_track_eval"][1]) == 17 and _lib.MPN_VERSION == 600
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    decl = re.search(r"\bint mpn_track_eval\s*\(([^)]*)\)\s*;", text)
    assert decl and len(decl.group(1).split(",")) == 17 and "double threshold" in decl.group(1)


def test_the_hungarian_method_is_shared_not_copied():
    csrc = os.path.join(ROOT, "multiposenet_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    holders = [f for f in sources if re.search(r"void assign_optimal\(", open(os.path.join(csrc, f)).read())]
    assert holders == ["hungarian.h"]
    for user, bias in (("pose_track.hip", "assign_optimal<0>"), ("track_eval.hip", "assign_optimal<kPairBias>")):
        text = open(os.path.join(csrc, user)).read()
        assert '#include "hungarian.h"' in text and bias in text


def test_public_names_and_keywords():
    from multiposenet_amd import inference
    from multiposenet_amd.track_metrics import TrackEvaluator, groundtruth_from_posetrack
    assert inference.TrackEvaluator is TrackEvaluator and inference.groundtruth_from_posetrack is groundtruth_from_posetrack
    parameters = inspect.signature(TrackEvaluator).parameters
    assert list(parameters)[:4] == ['streams', 'threshold', 'max_gt', 'max_identities']
    assert [parameters[k].default for k in list(parameters)[:4]] == [1, 0.5, 64, 256]
    for method in ('predict_batch', 'predict_images', 'predict_jpegs'):
        names = list(inspect.signature(getattr(inference.Detector, method)).parameters)
        assert names[-1] == 'track_eval', method
    for bad in (dict(streams=0), dict(threshold=float('nan')), dict(max_gt=65), dict(max_identities=1025), dict(max_boxes=65)):
        with pytest.raises(ValueError):
            TrackEvaluator(**bad)


def test_record_layout_keeps_its_four_slices():
    from multiposenet_amd.inference.detector import RecordLayout

    class Rows:
        def out_bytes(self, b):
            return 1000 + b
    base = lambda layout: (layout.record, layout.oks, layout.track, layout.nms)     # noqa: E731
    four = RecordLayout(4, 25)
    assert RecordLayout(4, 25, track_eval=None).astuple() == four.astuple()
    assert four.track_eval == slice(four.nms.stop, four.nms.stop) and four.nbytes == four.record.stop
    five = RecordLayout(4, 25, track_eval=Rows())
    assert base(five) == base(four) and five.track_eval.start % 16 == 0 and five.track_eval.start >= four.nms.stop
    assert five.track_eval.stop - five.track_eval.start == 1004 and five.nbytes == five.track_eval.stop


def test_track_frames_has_the_switches(capsys):
    from multiposenet_amd import track_frames
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--help"])
    text = capsys.readouterr().out
    assert e.value.code == 0 and "--annotations" in text and "--eval-threshold" in text
