"""numpy restatement of the result record of `mpn_pose_gather` (include/mpn.h), the yardstick of tests/test_pose_gather_gpu.py
and of the layout checks in tests/test_pose_gather_host.py.

The record is what the batched joint inference graph leaves for the host: the score filter of the reference's
inference/detector.py:54-59 and the live-slot gather of create_pb.py:96-104 over b images, plus the pixel keypoints of
inference/predict.ipynb (`draw_everything`). Everything below is float32 numpy (which never fuses a multiply-add) in the
documented operation order; the kernel performs the same operations in the same order, so records compare bit for bit.
"""
import numpy as np

F = np.float32
K = 17

# one row: 108 32-bit words
ROW = np.dtype([("image_index", np.int32), ("box", F, (4,)), ("score", F), ("keypoint_scores", F, (K,)),
                ("keypoint_positions", F, (K, 2)), ("keypoints", F, (K, 3))])


def header_words(B):
    """total, counts[B], num_boxes[B], overflow - padded with zero words to a multiple of 16 bytes."""
    return (2 * B + 2 + 3) // 4 * 4


def record_bytes(B, max_boxes):
    return header_words(B) * 4 + B * max_boxes * ROW.itemsize


def pixel_keypoints(boxes, keypoint_scores, keypoint_positions, height, width):
    """boxes f32 [n,4] normalised (ymin, xmin, ymax, xmax), positions f32 [n,17,2] = (y, x) normalised to the box ->
    f32 [n,17,3] = (x, y, score): x = xmin*width + pos_x * (xmax*width - xmin*width), y likewise."""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    n = len(boxes)
    out = np.zeros((n, K, 3), F)
    if keypoint_positions is not None:
        pos = np.asarray(keypoint_positions, F).reshape(n, K, 2)
        for c, (lo_i, hi_i, size, p_i) in enumerate(((1, 3, F(width), 1), (0, 2, F(height), 0))):
            lo = (boxes[:, lo_i] * size).astype(F)[:, None]
            hi = (boxes[:, hi_i] * size).astype(F)[:, None]
            span = (hi - lo).astype(F)
            out[:, :, c] = (lo + (pos[:, :, p_i] * span).astype(F)).astype(F)
    if keypoint_scores is not None:
        out[:, :, 2] = np.asarray(keypoint_scores, F).reshape(n, K)
    return out


def pose_gather(boxes, scores, num_boxes, keypoint_scores, keypoint_positions, overflow, score_threshold, height, width):
    """boxes f32 [B,max_boxes,4], scores f32 [B,max_boxes], num_boxes int32 [B], keypoint_scores f32 [B*max_boxes,17] or None,
    keypoint_positions f32 [B*max_boxes,17,2] or None, overflow int or None -> the record as a uint8 array."""
    boxes, scores = np.asarray(boxes, F), np.asarray(scores, F)
    num_boxes = np.asarray(num_boxes, np.int32)
    B, max_boxes = scores.shape
    n = B * max_boxes
    hw = header_words(B)
    rec = np.zeros(record_bytes(B, max_boxes), np.uint8)
    header = rec[:hw * 4].view(np.int32)
    rows = rec[hw * 4:].view(ROW)
    assert len(rows) == n
    slot = np.arange(max_boxes)[None, :]
    live = slot < num_boxes[:, None]
    with np.errstate(invalid="ignore"):
        keep = live & (np.where(live, scores, F(0)) > F(score_threshold))       # strict; slots >= num_boxes are never read
    header[0] = keep.sum()
    header[1:1 + B] = keep.sum(axis=1)
    header[1 + B:1 + 2 * B] = num_boxes
    header[1 + 2 * B] = 0 if overflow is None else int(overflow)
    src = np.flatnonzero(keep.reshape(-1))                                        # (image, slot) order
    t = len(src)
    rows["image_index"][:t] = src // max_boxes
    rows["box"][:t] = boxes.reshape(n, 4)[src]
    rows["score"][:t] = scores.reshape(n)[src]
    ks = None if keypoint_scores is None else np.asarray(keypoint_scores, F).reshape(n, K)[src]
    kp = None if keypoint_positions is None else np.asarray(keypoint_positions, F).reshape(n, K, 2)[src]
    if ks is not None:
        rows["keypoint_scores"][:t] = ks
    if kp is not None:
        rows["keypoint_positions"][:t] = kp
    rows["keypoints"][:t] = pixel_keypoints(rows["box"][:t], ks, kp, height, width)
    return rec
