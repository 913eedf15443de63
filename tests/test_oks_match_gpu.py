"""GPU: mpn_oks_match through pose_metrics.OksMatcher against the plain-loop COCOeval transcription (tests/pose_eval_ref.py)
on the five images of tests/pose_eval_cases.py: no detections, detections past max_dets, no ground truth, 64 ground-truth
persons mixing ignore / crowd / unlabelled / partly visible, bit-identical ground-truth rows under equal scores."""
import numpy as np
import pytest

import pose_eval_cases as cases
import pose_eval_ref as ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("score", ["box", "box*keypoints"])
def test_kernel_equals_the_reference(cuda, score):
    """rank, score, area, matches and ignore are EQUAL for every detection of every image (the generator keeps every OKS 1e-9
    from any value it is compared with, so a last-bit difference in exp cannot move a decision). The OKS matrix itself: a
    mean of at most 17 float64 exp values, each within 1 ulp: a few 1e-16 relative; rtol 1e-12 is slack by derivation."""
    import torch
    from multiposenet_amd import pose_metrics as pm
    dets, gts, want = cases.cases()
    mode = pm.SCORE_MODES[score]
    matcher = pm.OksMatcher(cases.B, cases.MAX_BOXES, cases.MAX_GT, score=score)
    matcher.out.fill_(255)                                          # rows behind the record's total must come back zero
    matcher.oks.fill_(7.0)
    got = matcher(dets, gts, return_oks=True)
    raw, raw_oks = matcher.out.cpu().numpy().copy(), matcher.oks.cpu().numpy().copy()
    assert len(got) == cases.B
    for i, (g, w) in enumerate(zip(got, want[mode])):
        n, ng = len(dets[i]['scores']), len(gts[i]['keypoints'])
        assert g['matches'].shape == (n, 3, 10) and g['ignore'].shape == (n, 3, 10) and g['ignore'].dtype == bool
        np.testing.assert_array_equal(g['rank'], w['rank'], err_msg=f"image {i}")
        assert g['score'].tobytes() == w['score'].tobytes() and g['area'].tobytes() == w['area'].tobytes(), i
        np.testing.assert_array_equal(g['matches'], w['matches'], err_msg=f"image {i}")
        np.testing.assert_array_equal(g['ignore'], w['ignore'], err_msg=f"image {i}")
        assert g['oks'].shape == (n, cases.MAX_GT) and not g['oks'][:, ng:].any()
        np.testing.assert_allclose(g['oks'][:, :ng], w['oks'], rtol=1e-12, atol=0, err_msg=f"image {i}")
        assert g['score_mode'] == mode and g['max_dets'] == ref.MAX_DETS
    total = sum(len(d['scores']) for d in dets)
    assert total == 62 and not raw[total * pm._OUT.itemsize:].any() and not raw_oks[total:].any()
    # the same launch again: the same bytes
    again = matcher(dets, gts, return_oks=True)
    assert matcher.out.cpu().numpy().tobytes() == raw.tobytes() and matcher.oks.cpu().numpy().tobytes() == raw_oks.tobytes()
    for g, a in zip(got, again):
        assert all(np.asarray(g[k]).tobytes() == np.asarray(a[k]).tobytes() for k in g)
    # and the evaluator on top of it gives the reference's ten numbers
    ev = pm.PoseEvaluator(score=score)
    ev.update(dets, gts)
    assert ev.evaluate() == ref.summarize(*ref.accumulate(want[mode]))
    torch.cuda.synchronize()
