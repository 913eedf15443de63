"""Hold-out boxes that give EVERY detector level a matched anchor: the batch of the all-levels teacher-forced gradient test
(tests/test_retinanet_gpu.py) and of the host check of the match counts (tests/test_detector_level_cases.py).

2 @ 384 x 512: levels 3..7 are 48 x 64 .. 3 x 4 pixels, the smallest non-square size at which a level-7 anchor (scale 512 or 724,
stride 128) can win a box - at 256 x 384 a whole-image box has IoU 0.375 with its best level-7 anchor and the forced match goes to
level 6. Five boxes per image, one sized for each level's anchors, in pixels (ymin, xmin, ymax, xmax)."""
import numpy as np

H, W = 384, 512
BOXES_PX = (
    ((86, 81, 116, 117), (168, 300, 238, 360), (90, 300, 210, 440), (95, 155, 345, 425), (6, 4, 380, 508)),
    ((288, 38, 312, 82), (46, 396, 134, 444), (200, 65, 300, 235), (25, 130, 355, 330), (0, 10, 384, 500)),
)
# matched anchors per level 3..7 and image, by oracle/retinanet.py (get_training_targets at the reference's thresholds)
MATCHED_PER_LEVEL = ((14, 14, 10, 23, 6), (12, 14, 14, 20, 5))


def boxes_and_num():
    """([B, 5, 4] float32 normalised by (H, W, H, W), [B] int32 = 5)"""
    boxes = np.array(BOXES_PX, np.float32) / np.array([H, W, H, W], np.float32)
    return boxes, np.full(len(BOXES_PX), len(BOXES_PX[0]), np.int32)


def matched_per_level(matches, shapes, anchors_per_location):
    """matches int32 [A] of one image (>= 0: matched) -> the count of matched anchors of every level"""
    out, at = [], 0
    for h, w in shapes:
        n = h * w * anchors_per_location
        out.append(int((matches[at:at + n] >= 0).sum()))
        at += n
    assert at == matches.shape[0]
    return tuple(out)
