"""GPU: mpn_pose_gather against its numpy restatement (tests/pose_gather_ref.py), bit for bit on the whole record."""
import numpy as np
import pytest
import torch

import pose_gather_ref as ref
from multiposenet_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
THR = F(0.35)


def _inputs(seed, B, max_boxes, num_boxes):
    """Random padded detector / PRN outputs; every slot >= num_boxes holds NaN in all five arrays."""
    rs = np.random.RandomState(seed)
    n = B * max_boxes
    y0, x0 = rs.rand(B, max_boxes) * 0.6, rs.rand(B, max_boxes) * 0.6
    boxes = np.stack([y0, x0, y0 + rs.rand(B, max_boxes) * 0.4, x0 + rs.rand(B, max_boxes) * 0.4], axis=2).astype(F)
    scores = rs.rand(B, max_boxes).astype(F)
    ks = rs.rand(n, 17).astype(F)
    kp = (rs.randint(0, 56, (n, 17, 2)) / np.array([56.0, 36.0])).astype(F)
    num_boxes = np.asarray(num_boxes, np.int32)
    dead = (np.arange(max_boxes)[None, :] >= num_boxes[:, None])
    boxes[dead], scores[dead] = np.nan, np.nan
    ks[dead.reshape(-1)], kp[dead.reshape(-1)] = np.nan, np.nan
    return boxes, scores, num_boxes, ks, kp


def _run(boxes, scores, num_boxes, ks, kp, overflow, thr, h, w):
    dev = torch.device("cuda:0")
    B, max_boxes = scores.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = [t(boxes), t(scores), t(num_boxes), t(ks), t(kp), None if overflow is None else torch.tensor([overflow], dtype=torch.int32, device=dev)]
    nbytes = _lib.lib().mpn_pose_gather_record_bytes(B, max_boxes)
    rec = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)          # the kernel owns every byte, the zero tail included
    _lib.call("mpn_pose_gather", *[_lib.ptr(x) for x in d], B, max_boxes, float(thr), h, w, _lib.ptr(rec), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rec.cpu().numpy()


def _check(boxes, scores, num_boxes, ks, kp, overflow=0, thr=THR, h=256, w=384):
    got = _run(boxes, scores, num_boxes, ks, kp, overflow, thr, h, w)
    want = ref.pose_gather(boxes, scores, num_boxes, ks, kp, overflow, thr, h, w)
    assert got.shape == want.shape
    B = scores.shape[0]
    hw = ref.header_words(B)
    np.testing.assert_array_equal(got[:hw * 4].view(np.int32), want[:hw * 4].view(np.int32), err_msg="header")
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at byte {bad[0]} (row {(bad[0] - hw * 4) // ref.ROW.itemsize})"
    assert not np.isnan(got[hw * 4:].view(F)).any()                           # no garbage from the slots >= num_boxes
    return want[:hw * 4].view(np.int32)


# (B, max_boxes, num_boxes): one image below one wave; several images with an empty and a full one, 75 rows (above a wave, not
# a multiple of 64); 1250 rows = more than the block's 1024 threads (the scan carries across chunks); max_boxes = 1
CASES = [(1, 25, [11]), (3, 25, [0, 25, 7]), (50, 25, [(7 * i) % 26 for i in range(50)]), (7, 1, [1, 0, 1, 1, 0, 0, 1]),
         (2, 64, [64, 3])]


@pytest.mark.parametrize("B,max_boxes,num", CASES, ids=[f"{b}x{m}" for b, m, _ in CASES])
def test_record_matches_the_numpy_restatement(cuda, B, max_boxes, num):
    boxes, scores, num, ks, kp = _inputs(B * 1000 + max_boxes, B, max_boxes, num)
    header = _check(boxes, scores, num, ks, kp)
    live = int(np.minimum(num, max_boxes).sum())
    assert 0 < header[0] < live or live < 8                                   # the threshold splits the live slots
    np.testing.assert_array_equal(header[1 + B:1 + 2 * B], num)


def test_threshold_is_strict_and_all_below_gives_an_empty_record(cuda):
    boxes, scores, num, ks, kp = _inputs(5, 3, 25, [25, 9, 0])
    scores[0, 3] = THR                                                        # exactly the threshold: dropped
    scores[0, 4] = np.nextafter(THR, F(1))                                    # the next float above: kept
    scores[1, 0] = THR
    header = _check(boxes, scores, num, ks, kp)
    want_keep = (np.arange(25)[None] < num[:, None]) & (np.nan_to_num(scores) > THR)
    assert not want_keep[0, 3] and want_keep[0, 4] and not want_keep[1, 0]
    np.testing.assert_array_equal(header[1:4], want_keep.sum(axis=1))
    header = _check(boxes, scores, num, ks, kp, thr=F(1.5))                   # every score below the threshold
    assert header[0] == 0 and not header[1:4].any()
    header = _check(boxes, scores, num, ks, kp, thr=F(-1.0))                  # everything live is kept
    assert header[0] == 34


def test_null_keypoint_inputs_and_overflow_word(cuda):
    boxes, scores, num, ks, kp = _inputs(6, 3, 25, [4, 25, 13])
    _check(boxes, scores, num, None, None, overflow=None)
    _check(boxes, scores, num, ks, None)
    _check(boxes, scores, num, None, kp)
    header = _check(boxes, scores, num, ks, kp, overflow=1)
    assert header[1 + 2 * 3] == 1


def test_pixel_keypoints_are_the_documented_f32_formula(cuda):
    """x = xmin*width + pos_x * (xmax*width - xmin*width) in float32, no fused multiply-add: written out here once more, scalar
    by scalar, at a size (640 x 1152) where a contraction would change last bits."""
    boxes, scores, num, ks, kp = _inputs(9, 2, 25, [25, 25])
    h, w = 640, 1152
    rec = _run(boxes, scores, num, ks, kp, 0, F(-1.0), h, w)
    rows = rec[ref.header_words(2) * 4:].view(ref.ROW)
    for r in (0, 17, 49):
        ymin, xmin, ymax, xmax = boxes.reshape(-1, 4)[r]
        for k in (0, 8, 16):
            py, px = kp[r, k]
            x = F(xmin * F(w)) + F(px * F(F(xmax * F(w)) - F(xmin * F(w))))
            y = F(ymin * F(h)) + F(py * F(F(ymax * F(h)) - F(ymin * F(h))))
            assert rows["keypoints"][r, k].tobytes() == np.array([x, y, ks[r, k]], F).tobytes()
