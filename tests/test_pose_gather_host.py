"""CPU: mpn_pose_gather's ABI surface, its refusals and record layout, and predict_batch's argument checks - no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import pose_gather_ref as ref
from multiposenet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpn_pose_gather", "mpn_pose_gather_record_bytes", "mpn_pose_gather_row_offset")


def test_pose_gather_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mpn_[a-z0-9_]+)\s*\(", text))
    l = _lib.lib()
    for n in NAMES:
        assert n in declared and n in _lib.SIGNATURES and hasattr(l, n), n
    assert l.mpn_version() == _lib.MPN_VERSION == 600          # additive: the ABI revision does not move


def test_launcher_refusals_need_no_gpu():
    P = ctypes.c_void_p(4096)
    big = 1 << 30

    def gather(boxes=P, scores=P, num=P, B=2, max_boxes=25, h=256, w=384, record=P, nbytes=big):
        _lib.call("mpn_pose_gather", boxes, scores, num, None, None, None, B, max_boxes, 0.05, h, w, record, nbytes, None)
    for kw in ({"boxes": None}, {"scores": None}, {"num": None}, {"record": None}):
        with pytest.raises(ValueError, match="BAD_ARG.*null pointer"):
            gather(**kw)
    for kw in ({"B": 0}, {"max_boxes": 0}, {"B": -3}, {"h": 0}, {"w": 0}):
        with pytest.raises(ValueError, match="BAD_SHAPE"):
            gather(**kw)
    with pytest.raises(ValueError, match="BAD_SHAPE.*single block"):
        gather(B=64, max_boxes=65)                              # 4160 rows: one more image row than the block's tables hold
    with pytest.raises(ValueError, match="BAD_ALIGN"):
        gather(record=ctypes.c_void_p(4100))
    need = _lib.lib().mpn_pose_gather_record_bytes(2, 25)
    with pytest.raises(_lib.MpnError, match="WORKSPACE"):
        gather(nbytes=need - 1)
    assert _lib.lib().mpn_pose_gather_record_bytes(64, 65) == 0 and _lib.lib().mpn_pose_gather_record_bytes(0, 25) == 0
    assert _lib.lib().mpn_pose_gather_record_bytes(64, 64) > 0   # the largest batch worth supporting (25 x 64) and beyond


@pytest.mark.parametrize("B,max_boxes", [(1, 25), (2, 25), (3, 7), (16, 25), (64, 25), (5, 1)])
def test_layout_functions_agree_with_the_numpy_record(B, max_boxes):
    l = _lib.lib()
    assert l.mpn_pose_gather_record_bytes(B, max_boxes) == ref.record_bytes(B, max_boxes)
    first = l.mpn_pose_gather_row_offset(B, max_boxes, 0)
    assert first == ref.header_words(B) * 4 and first % 16 == 0 and first >= (2 * B + 2) * 4
    n = B * max_boxes
    for r in (1, n // 2, n):
        assert l.mpn_pose_gather_row_offset(B, max_boxes, r) == first + r * ref.ROW.itemsize
    assert l.mpn_pose_gather_row_offset(B, max_boxes, n) == l.mpn_pose_gather_record_bytes(B, max_boxes)
    assert l.mpn_pose_gather_row_offset(B, max_boxes, n + 1) == 0 and l.mpn_pose_gather_row_offset(B, max_boxes, -1) == 0
    # the product's unpacking reads the record the restatement builds
    from multiposenet_amd.inference.detector import _ROW, unpack_record
    assert _ROW == ref.ROW and ref.ROW.itemsize == 432
    rs = np.random.RandomState(B * 100 + max_boxes)
    boxes, scores = rs.rand(B, max_boxes, 4).astype(np.float32), rs.rand(B, max_boxes).astype(np.float32)
    num = rs.randint(0, max_boxes + 1, B).astype(np.int32)
    ks, kp = rs.rand(n, 17).astype(np.float32), rs.rand(n, 17, 2).astype(np.float32)
    rec = ref.pose_gather(boxes, scores, num, ks, kp, 0, 0.4, 256, 384)
    outs = unpack_record(rec, B, max_boxes)
    assert len(outs) == B
    for i, o in enumerate(outs):
        keep = (np.arange(max_boxes) < num[i]) & (scores[i] > np.float32(0.4))
        np.testing.assert_array_equal(o["boxes"], boxes[i][keep])
        np.testing.assert_array_equal(o["scores"], scores[i][keep])
        assert o["num_boxes"] == num[i] and o["num_boxes"].dtype == np.int32
        np.testing.assert_array_equal(o["keypoint_scores"], ks.reshape(B, max_boxes, 17)[i][keep])
        np.testing.assert_array_equal(o["keypoint_positions"], kp.reshape(B, max_boxes, 17, 2)[i][keep])
        np.testing.assert_array_equal(o["keypoints"], ref.pixel_keypoints(o["boxes"], o["keypoint_scores"], o["keypoint_positions"], 256, 384))
    with pytest.raises(RuntimeError, match="overflowed"):
        unpack_record(ref.pose_gather(boxes, scores, num, ks, kp, 1, 0.4, 256, 384), B, max_boxes)


def test_predict_batch_argument_checks_run_before_any_device_work():
    from multiposenet_amd.inference.detector import Detector, check_batch
    ok = np.zeros((3, 128, 256, 3), np.uint8)
    assert check_batch(ok) == (3, 128, 256) and check_batch(list(ok)) == (3, 128, 256)
    with pytest.raises(ValueError, match="uint8"):
        check_batch(ok.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        check_batch([ok[0], ok[1].astype(np.int32)])
    with pytest.raises(AssertionError):
        check_batch(np.zeros((2, 100, 128, 3), np.uint8))
    with pytest.raises(AssertionError):
        check_batch([np.zeros((128, 192, 3), np.uint8)] * 2)
    with pytest.raises(ValueError, match="one size"):
        check_batch([ok[0], np.zeros((256, 256, 3), np.uint8)])
    with pytest.raises(ValueError):
        check_batch(ok[0])                                       # one image is not a batch
    with pytest.raises(ValueError, match="empty"):
        check_batch([])
    # the method itself refuses before it touches its (here absent) networks
    det = Detector.__new__(Detector)
    for bad, err in ((ok.astype(np.float32), ValueError), (np.zeros((2, 100, 128, 3), np.uint8), AssertionError),
                     ([ok[0], np.zeros((256, 256, 3), np.uint8)], ValueError)):
        with pytest.raises(err):
            det.predict_batch(bad)
