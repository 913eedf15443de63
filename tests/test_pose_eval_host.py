"""CPU: the keypoint-AP yardstick (tests/pose_eval_ref.py) against closed-form answers, and the host side of
multiposenet_amd/pose_metrics.py (accumulate / summarize, ground-truth converters, argument checks) against it."""
import json

import numpy as np
import pytest

import pose_eval_cases as cases
import pose_eval_ref as ref
from multiposenet_amd import pose_metrics as pm


def _gt(kps, boxes, area=None, iscrowd=None):
    g = {'keypoints': np.array(kps, np.float64).reshape(-1, 17, 3), 'boxes': np.array(boxes, np.float64).reshape(-1, 4)}
    if area is not None:
        g['area'] = np.array(area, np.float64)
    if iscrowd is not None:
        g['iscrowd'] = np.array(iscrowd, np.int32)
    return g


def _det(kps, scores):
    kps = np.array(kps, np.float32).reshape(-1, 17, 3)
    return {'scores': np.array(scores, np.float32), 'keypoint_scores': np.ascontiguousarray(kps[:, :, 2]), 'keypoints': kps}


def _pose(x0, y0, side, v=2.0):
    """17 keypoints on a fixed lattice inside a side x side box; exactly representable in float32."""
    k = np.arange(17)
    return np.stack([x0 + (k % 5) * side / 4.0, y0 + (k // 5) * side / 4.0, np.full(17, v)], 1)


def test_constants_are_cocos():
    np.testing.assert_array_equal(pm.KEYPOINT_SIGMAS, ref.SIGMAS)
    np.testing.assert_array_equal(pm.OKS_THRESHOLDS, ref.IOU_THRS)
    np.testing.assert_array_equal(pm.RECALL_THRESHOLDS, ref.REC_THRS)
    assert [list(r[1:]) for r in pm.AREA_RANGES] == [[float(v) for v in r] for r in ref.AREA_RNG]
    assert pm.MAX_DETS == ref.MAX_DETS == 20 and pm.STAT_NAMES == ref.NAMES
    assert pm.OKS_THRESHOLDS[0] == .5 and pm.OKS_THRESHOLDS[5] == .75


def test_reference_detections_equal_to_groundtruth_score_one():
    # two persons per range: COCOeval's precision tp / (tp + fp + 2^-52) is exactly 1.0 from tp = 2 on (and 1 - 2^-52 at
    # tp = 1, which the right-to-left envelope then lifts to 1.0)
    poses = [_pose(10, 20, 64), _pose(300, 40, 128), _pose(100, 300, 200), _pose(900, 300, 256)]
    gt = _gt(poses, [[10, 20, 64, 64], [300, 40, 128, 128], [100, 300, 200, 200], [900, 300, 256, 256]],
             area=[40.0 ** 2, 70.0 ** 2, 150.0 ** 2, 200.0 ** 2])
    det = _det(poses, [0.9, 0.8, 0.7, 0.6])
    table = ref.evaluate_image(det, gt)
    assert np.all(np.diag(table['oks']) == 1.0)
    assert table['matches'][:, 0, :].tolist() == [[i] * 10 for i in range(4)]
    stats = ref.evaluate([det], [gt])
    assert stats == {k: 1.0 for k in ref.NAMES}


def test_reference_no_detections_and_no_groundtruth_in_a_range():
    gt = _gt([_pose(10, 20, 64)], [[10, 20, 64, 64]], area=[50.0 ** 2])          # medium only
    stats = ref.evaluate([_det([], [])], [gt])
    assert stats['AP'] == 0.0 and stats['AR'] == 0.0 and stats['APM'] == 0.0 and stats['ARM'] == 0.0
    assert stats['APL'] == -1.0 and stats['ARL'] == -1.0
    assert ref.evaluate([_det([_pose(0, 0, 50)], [0.5])], [_gt([], [])]) == {k: -1.0 for k in ref.NAMES}


def test_reference_oks_closed_form():
    d, area = 3.0, 5000.0
    pose = _pose(100, 100, 80)
    pose[::2, 2] = 0.0                                               # 8 of 17 visible
    shifted = pose.copy()
    shifted[:, 0] += d
    gt = _gt([pose], [[100, 100, 80, 80]], area=[area])
    table = ref.evaluate_image(_det([shifted], [0.5]), gt)
    vis = pose[:, 2] > 0
    want = np.mean(np.exp(-d * d / (2 * area * (2 * ref.SIGMAS[vis]) ** 2)))
    assert vis.sum() == 8 and abs(table['oks'][0, 0] - want) < 1e-15
    assert table['area'][0] == 80.0 * 60.0                           # the lattice spans 80 x 60; the shift moves both ends


def test_reference_bbox_branch_when_nothing_is_labelled():
    pose = _pose(100, 100, 40, v=0.0)
    gt = _gt([pose], [[100, 100, 40, 40]], area=[1600.0])           # doubled box: [60, 180] in x and y
    inside, outside = _pose(70, 70, 100), _pose(70, 70, 100)
    outside[:, 0] += 200.0                                           # x from 270: dx = x - 180 > 0 for every keypoint
    table = ref.evaluate_image(_det([inside, outside], [0.9, 0.8]), gt)
    assert table['oks'][0, 0] == 1.0
    dx = outside[:, 0] - 180.0
    want = np.mean(np.exp(-(dx ** 2) / (2 * ref.SIGMAS) ** 2 / (1600.0 + np.spacing(1)) / 2))
    assert abs(table['oks'][1, 0] - want) <= 1e-15 * max(want, 1e-300) + 1e-300
    assert table['gt_ignore'].all()                                  # no labelled keypoint: ignored in every range
    assert table['matches'][0, 0, 0] == 0 and table['ignore'][0, 0].all()


def test_reference_crowd_takes_two_detections():
    pose = _pose(100, 100, 100)
    gt = _gt([pose], [[100, 100, 100, 100]], area=[9000.0], iscrowd=[1])
    table = ref.evaluate_image(_det([pose, pose], [0.9, 0.8]), gt)
    assert (table['matches'][:, 0, :] == 0).all() and table['ignore'][:, 0, :].all()
    stats = ref.evaluate([_det([pose, pose], [0.9, 0.8])], [gt])
    assert stats['AP'] == -1.0                                       # nothing but an ignored person: no ground truth counted
    # with a plain twin: the first detection takes the plain person, the second the crowd - no false positive
    gt2 = _gt([pose, pose], [[100, 100, 100, 100]] * 2, area=[9000.0] * 2, iscrowd=[1, 0])
    table = ref.evaluate_image(_det([pose, pose], [0.9, 0.8]), gt2)
    assert table['matches'][:, 0, 0].tolist() == [1, 0] and table['ignore'][:, 0, 0].tolist() == [False, True]
    # one true positive, no false positive: COCOeval's precision tp / (tp + fp + 2^-52) at tp = 1
    assert ref.evaluate([_det([pose, pose], [0.9, 0.8])], [gt2])['AP'] == 1.0 / (1.0 + np.spacing(1))


def test_reference_max_dets_equal_scores_and_area_ranges():
    pose = _pose(100, 100, 100)
    gt = _gt([pose], [[100, 100, 100, 100]], area=[9000.0])
    far = _pose(5000, 5000, 100)
    scores = [0.5] * 21
    scores[20] = 0.4
    table = ref.evaluate_image(_det([far] * 20 + [pose], scores), gt)
    assert table['rank'].tolist() == list(range(21))                 # equal scores keep the record's order
    assert (table['matches'][20] == -1).all() and not table['ignore'][20].any() and table['oks'][20, 0] == 0.0
    assert ref.evaluate([_det([far] * 20 + [pose], scores)], [gt])['AR'] == 0.0     # the 21st would have matched
    # an unmatched detection of area 80 x 60 (medium): a false positive in 'all' and 'medium', ignored in 'large'
    small = _pose(5000, 5000, 20)                                    # 20 x 15 = 300 < 32^2
    table = ref.evaluate_image(_det([small, far], [0.9, 0.8]), gt)
    assert table['ignore'][0, :, 0].tolist() == [False, True, True]
    assert table['ignore'][1, :, 0].tolist() == [False, False, True]


def test_generator_terminates_and_keeps_its_margins():
    dets, gts, want = cases.cases()
    assert [len(d['scores']) for d in dets] == [0, 25, 7, 25, 5] and [len(g['keypoints']) for g in gts] == [2, 1, 0, 64, 3]
    for mode in (0, 1):
        t = want[mode]
        assert (t[1]['rank'] >= 20).sum() == 5
        assert t[3]['gt_ignore'][0].sum() >= 32 and (t[3]['matches'][:, 0, 0] >= 0).sum() >= 10
        assert (t[3]['ignore'][:, 0, 0] & (t[3]['matches'][:, 0, 0] >= 0)).any()       # matched to an ignored person
        assert len(set(t[3]['matches'][:, 0, 0].tolist()) - {-1}) >= 8
        assert np.array_equal(t[4]['oks'][:, 0], t[4]['oks'][:, 1]) and t[4]['matches'][:2, 0, 0].tolist() == [1, 0]
        assert t[4]['rank'][0] < t[4]['rank'][1] < t[4]['rank'][2]                          # equal scores: record order
    assert not np.array_equal(want[0][3]['rank'], want[1][3]['rank'])                   # the score mode changes the order


def _evaluator_from_tables(tables, gts, score='box'):
    ev = pm.PoseEvaluator(score=score)
    for t, g in zip(tables, gts):
        ev.add_image(t, g)
    return ev


def test_evaluator_equals_reference_accumulate():
    dets, gts, want = cases.cases()
    for mode, score in ((0, 'box'), (1, 'box*keypoints')):
        stats = _evaluator_from_tables(want[mode], gts, score).evaluate()
        assert stats == ref.summarize(*ref.accumulate(want[mode]))
        assert set(stats) == set(pm.STAT_NAMES) and 0.0 < stats['AP'] < 1.0 and stats['APM'] > -1.0 and stats['APL'] > -1.0
    # random match tables, precision and recall arrays entry by entry
    rng = np.random.default_rng(7)
    tables, gl = [], []
    for _ in range(6):
        n, g = int(rng.integers(0, 24)), int(rng.integers(0, 6))
        tables.append({'rank': rng.permutation(n).astype(np.int32), 'score': rng.choice([0.2, 0.5, 0.7, 0.9], n).astype(np.float32),
                       'matches': rng.integers(-1, max(g, 1), (n, 3, 10)).astype(np.int32), 'ignore': rng.random((n, 3, 10)) < 0.2,
                       'gt_ignore': np.zeros((3, g), bool)})
        gl.append(_gt([_pose(0, 0, 50)] * g, [[0, 0, 50, 50]] * g, area=rng.choice([500.0, 3000.0, 20000.0], g)))
        for a, (lo, hi) in enumerate(ref.AREA_RNG):
            tables[-1]['gt_ignore'][a] = (gl[-1]['area'] < lo) | (gl[-1]['area'] > hi)
    ev = _evaluator_from_tables(tables, gl)
    p, r = pm.evaluate_tables(np.concatenate(ev.scores), np.concatenate(ev.matched), np.concatenate(ev.ignored), ev.num_groundtruth)
    wp, wr = ref.accumulate(tables)
    np.testing.assert_array_equal(p, wp)
    np.testing.assert_array_equal(r, wr)
    assert ev.evaluate() == ref.summarize(wp, wr)
    # nothing collected; initialize() forgets
    assert pm.PoseEvaluator().evaluate() == {k: -1.0 for k in pm.STAT_NAMES} == ref.summarize(*ref.accumulate([]))
    ev.initialize()
    assert ev.evaluate() == {k: -1.0 for k in pm.STAT_NAMES}


def test_groundtruth_converters(tmp_path):
    example = {'boxes': np.array([[10, 20, 110, 70]], np.float32), 'keypoints': np.zeros((1, 17, 3), np.int32)}
    example['keypoints'][0, :, 0], example['keypoints'][0, :, 1], example['keypoints'][0, :, 2] = 30, 40, 2
    gt = pm.groundtruth_from_record(example)
    assert gt['boxes'].tolist() == [[20.0, 10.0, 50.0, 100.0]] and gt['area'].tolist() == [5000.0]
    assert gt['keypoints'][0, 0].tolist() == [40.0, 30.0, 2.0] and gt['iscrowd'].tolist() == [0]
    kp, boxes, area, crowd, ignore = pm.groundtruth_arrays({'keypoints': gt['keypoints'], 'boxes': gt['boxes']})
    assert area.tolist() == [5000.0] and not crowd.any() and not ignore.any()
    coco = {'images': [{'id': 7, 'file_name': 'a.jpg'}, {'id': 9, 'file_name': 'b.jpg'}],
            'annotations': [{'image_id': 7, 'keypoints': [1, 2, 2] * 17, 'bbox': [0, 0, 10, 20], 'area': 120.5, 'iscrowd': 0, 'num_keypoints': 17},
                            {'image_id': 7, 'keypoints': [0, 0, 0] * 17, 'bbox': [5, 5, 10, 20], 'area': 99.0, 'iscrowd': 0, 'num_keypoints': 0},
                            {'image_id': 7, 'keypoints': [3, 4, 1] * 17, 'bbox': [5, 5, 30, 20], 'area': 400.0, 'iscrowd': 1, 'num_keypoints': 17}]}
    path = tmp_path / "person_keypoints_tiny.json"
    path.write_text(json.dumps(coco))
    got = pm.groundtruth_from_coco(str(path))
    assert set(got) == {7, 9} and got[7][0] == 'a.jpg' and got[9][0] == 'b.jpg'
    assert got[9][1]['keypoints'].shape == (0, 17, 3) and got[9][1]['boxes'].shape == (0, 4)
    kp, boxes, area, crowd, ignore = pm.groundtruth_arrays(got[7][1])
    assert area.tolist() == [120.5, 99.0, 400.0] and crowd.tolist() == [False, False, True] and ignore.tolist() == [False, True, True]
    assert kp[2, 0].tolist() == [3.0, 4.0, 1.0] and boxes[2].tolist() == [5.0, 5.0, 30.0, 20.0]
    rows, counts = np.ones((1, 4, 64)), np.zeros(1, np.int32)
    pm.pack_groundtruth([got[7][1]], rows, counts)
    assert counts[0] == 3 and rows[0, 2, :3].tolist() == [3.0, 4.0, 1.0] and rows[0, 2, 51:58].tolist() == [5, 5, 30, 20, 400, 1, 1]
    assert not rows[0, 3].any() and not rows[0, :, 58:].any()
    with pytest.raises(ValueError, match="5 persons"):
        pm.pack_groundtruth([_gt([_pose(0, 0, 9)] * 5, [[0, 0, 9, 9]] * 5)], rows, counts)


def test_more_than_64_groundtruth_rows_raise_before_any_hip_call():
    import ctypes
    from multiposenet_amd import _lib
    P = ctypes.c_void_p(4096)
    with pytest.raises(ValueError, match="max_gt"):
        _lib.call("mpn_oks_match", P, 5, 25, P, P, 65, P, 10, 0, 20, P, None, None)
    with pytest.raises(ValueError, match="max_gt"):
        pm.OksMatcher(5, 25, max_gt=65)
    with pytest.raises(ValueError, match="max_gt"):
        pm.PoseEvaluator(max_gt=65)
    with pytest.raises(ValueError, match="max_dets"):
        _lib.call("mpn_oks_match", P, 5, 25, P, P, 64, P, 10, 0, 21, P, None, None)
    lib = _lib.lib()
    assert lib.mpn_oks_gt_row_bytes() == 512 and lib.mpn_oks_match_out_bytes(5, 25) == 5 * 25 * pm._OUT.itemsize == 5 * 25 * 152
    assert lib.mpn_oks_match_out_bytes(1, 257) == 0 and lib.mpn_oks_match_out_bytes(64, 65) == 0
