"""GPU: mpn_pose_nms through pose_nms.PoseSuppressor against the plain-loop reference (tests/pose_nms_ref.py) on the case
table of tests/pose_nms_cases.py: record_out and info byte for byte, the similarity matrix to rtol 1e-12.

The bound on the matrix: a similarity is a mean of at most 17 float64 exp values, each within 1 ulp of math.exp's - a few
1e-16 relative; rtol 1e-12 is slack by derivation (the bound tests/test_oks_match_gpu.py derives). The bytes can be held
to equality because tests/test_pose_nms_host.py shows that no similarity the table compares is within 1e-9 of its threshold."""
import numpy as np
import pytest

import pose_nms_cases as cases
import pose_nms_ref as ref

pytestmark = pytest.mark.gpu


def _run(suppressor, record, nms):
    """One launch over buffers pre-filled with 255: everything the launch owns must be written."""
    import torch
    suppressor.record_out.fill_(255)
    suppressor.info.fill_(255)
    suppressor.sim.view(torch.uint8).fill_(255)
    return suppressor.run(record, nms)


def _check(suppressor, record, b, max_boxes, threshold, mks, score):
    from multiposenet_amd.inference import PoseNms
    from multiposenet_amd.pose_metrics import SCORE_MODES
    nms = PoseNms(threshold, mks, score)
    want_out, want_info, want_sim = ref.run(record, b, max_boxes, nms.threshold, nms.min_keypoint_score, SCORE_MODES[score])
    out, info, sim = _run(suppressor, record, nms)
    assert out.shape == want_out.shape and info.shape == want_info.shape and sim.shape == want_sim.shape
    hw = ref.header_words(b) * 4
    np.testing.assert_array_equal(out[:hw].view(np.int32), want_out[:hw].view(np.int32), err_msg="header")
    np.testing.assert_array_equal(info[:ref.info_head_bytes(b)].view(np.int32), want_info[:ref.info_head_bytes(b)].view(np.int32))
    np.testing.assert_array_equal(info.view(np.int32), want_info.view(np.int32), err_msg="info")
    assert out.tobytes() == want_out.tobytes() and info.tobytes() == want_info.tobytes()
    assert (sim == 0).tobytes() == (want_sim == 0).tobytes()        # the diagonal and everything outside n x n
    np.testing.assert_allclose(sim, want_sim, rtol=1e-12, atol=0)
    assert np.array_equal(sim, sim.transpose(0, 2, 1))              # each unordered pair once
    # the same launch again: the same bytes
    out2, info2, sim2 = _run(suppressor, record, nms)
    assert out2.tobytes() == out.tobytes() and info2.tobytes() == info.tobytes() and sim2.tobytes() == sim.tobytes()
    return out, info, sim


@pytest.fixture(scope="module")
def table_suppressor(cuda):
    from multiposenet_amd.inference import PoseSuppressor
    return PoseSuppressor(cases.B, cases.MAX_BOXES)


@pytest.mark.parametrize("score", ["box", "box*keypoints"])
@pytest.mark.parametrize("mks", cases.MIN_KEYPOINT_SCORES)
def test_kernel_equals_the_reference(table_suppressor, score, mks):
    record = cases.table(overflow=5 if score == "box" else 0)       # a set overflow word is copied through
    out, info, _ = _check(table_suppressor, record, cases.B, cases.MAX_BOXES, cases.THRESHOLD, mks, score)
    header = out[:ref.header_words(cases.B) * 4].view(np.int32)
    assert header[0] == (76 if mks == 0.5 else 75) and header[1 + 2 * cases.B] == (5 if score == "box" else 0)
    assert info[:4 * cases.B].view(np.int32).tolist() == [0, 0, 63, 1, 0, 2 if mks == 0.5 else 3, 1, 2]


def test_threshold_one_keeps_every_row(table_suppressor):
    record = cases.table()
    out, info, _ = _check(table_suppressor, record, cases.B, cases.MAX_BOXES, 1.0, 0.0, "box")
    assert out.tobytes() == record.tobytes() and not info[:4 * cases.B].any()


def test_one_block_limit(cuda):
    """B = 64, max_boxes = 64: 4096 slots, four strides of the compaction's block; 1160 rows in, 608 out."""
    from multiposenet_amd.inference import PoseSuppressor
    out, _, _ = _check(PoseSuppressor(64, 64), cases.large(), 64, 64, cases.THRESHOLD, 0.5, "box*keypoints")
    assert out[:4].view(np.int32)[0] == 608


def test_nan_scores_and_small_shapes(cuda):
    """B = 2, max_boxes = 4 (a max_boxes below the wave size); NaN order scores sort last, in record order."""
    from multiposenet_amd.inference import PoseSuppressor
    record = cases.pack(cases.nan_scores(), 2, 4)
    out, info, _ = _check(PoseSuppressor(2, 4), record, 2, 4, cases.THRESHOLD, 0.0, "box")
    assert out[:12].view(np.int32).tolist() == [5, 4, 1] and info[:8].view(np.int32).tolist() == [0, 1]


def test_host_dicts(cuda):
    """inference.pose_nms on result dicts: the survivors of every per-person array by their source index, the three keys,
    everything else passed through."""
    from multiposenet_amd.inference import PoseNms, pose_nms
    imgs = cases.images()
    outputs = []
    for i, persons in enumerate(imgs):
        kp = np.stack([p[0] for p in persons]) if persons else np.zeros((0, 17, 3), np.float32)
        scores = np.array([p[1] for p in persons], np.float32)
        outputs.append({'scores': scores, 'keypoints': kp, 'keypoint_scores': kp[:, :, 2].copy(),
                        'boxes': np.arange(4 * len(persons), dtype=np.float32).reshape(-1, 4), 'num_boxes': np.int32(len(persons) + 1),
                        'name': f"image {i}"})
    nms = PoseNms(cases.THRESHOLD, 0.5, 'box*keypoints')
    got = pose_nms(outputs, nms)
    assert len(got) == cases.B
    for i, (o, g) in enumerate(zip(outputs, got)):
        kept, absorbed, _ = ref.survivors(o['keypoints'], o['scores'], o['keypoint_scores'], nms.threshold, 0.5, 1)
        assert set(g) == set(o) | {'pose_nms_source', 'pose_nms_absorbed', 'pose_nms_suppressed'}
        assert g['pose_nms_source'].dtype == np.int32 and g['pose_nms_absorbed'].dtype == np.int32
        assert type(g['pose_nms_suppressed']) is np.int32 and g['pose_nms_suppressed'] == len(o['scores']) - len(kept)
        assert g['pose_nms_source'].tolist() == kept and g['pose_nms_absorbed'].tolist() == [absorbed[p] for p in kept], i
        for k in ('scores', 'keypoints', 'keypoint_scores', 'boxes'):
            assert g[k].dtype == o[k].dtype and g[k].tobytes() == o[k][kept].tobytes(), (i, k)
        assert g['num_boxes'] == o['num_boxes'] and g['name'] == o['name']
    with pytest.raises(ValueError, match="pose_nms must be None or an inference.PoseNms"):
        pose_nms(outputs, 0.7)
