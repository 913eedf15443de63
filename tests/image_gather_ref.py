"""numpy restatement of the record of `mpn_pose_gather_sized` (include/mpn.h): `mpn_pose_gather`'s record (pose_gather_ref.py)
for images that were resized onto the network canvas. Per image, extent = (box_scale_y, box_scale_x, pixel_height, pixel_width):
the record's box is box * (box_scale_y, box_scale_x, box_scale_y, box_scale_x), one float32 multiply each, and its keypoints
are pose_gather_ref.pixel_keypoints of THAT box with (pixel_height, pixel_width) - float32 numpy in the kernel's order, so
records compare bit for bit."""
import numpy as np

import pose_gather_ref as ref

F = np.float32


def source_boxes(boxes, extent):
    """boxes f32 [n,4] normalised to the canvas, extent f32 [4] -> f32 [n,4] normalised to the source image."""
    e = np.asarray(extent, F)
    return (np.asarray(boxes, F).reshape(-1, 4) * np.array([e[0], e[1], e[0], e[1]], F)).astype(F)


def map_person(person, extent):
    """A dict of `Detector.predict_batch` for a resized image -> what `Detector.predict_images` returns for its source."""
    out = dict(person)
    out["boxes"] = source_boxes(person["boxes"], extent)
    n = len(out["boxes"])
    if person["keypoint_positions"].shape[0] == n and person["keypoint_scores"].shape[0] == n:
        out["keypoints"] = ref.pixel_keypoints(out["boxes"], person["keypoint_scores"], person["keypoint_positions"],
                                               F(extent[2]), F(extent[3]))
    return out


def pose_gather_sized(boxes, scores, num_boxes, keypoint_scores, keypoint_positions, overflow, score_threshold, extent):
    """As pose_gather_ref.pose_gather, with extent f32 [B,4] in place of height, width -> the record as a uint8 array."""
    scores = np.asarray(scores, F)
    B, max_boxes = scores.shape
    extent = np.asarray(extent, F).reshape(B, 4)
    # the kept rows and their order do not depend on the extents: pack with any size, then rewrite boxes and keypoints
    rec = ref.pose_gather(boxes, scores, num_boxes, keypoint_scores, keypoint_positions, overflow, score_threshold, 1, 1)
    hw = ref.header_words(B)
    rows = rec[hw * 4:].view(ref.ROW)
    t = int(rec[:4].view(np.int32)[0])
    for j in range(t):
        e = extent[rows["image_index"][j]]
        box = source_boxes(rows["box"][j], e)
        rows["box"][j] = box[0]
        ks = None if keypoint_scores is None else rows["keypoint_scores"][j][None]
        kp = None if keypoint_positions is None else rows["keypoint_positions"][j][None]
        rows["keypoints"][j] = ref.pixel_keypoints(box, ks, kp, e[2], e[3])[0]
    return rec
