"""Per-image random decisions and geometry of the keypoint input pipeline (host, numpy float32).

Restates the host-visible maths of the reference's `augmentation` (keypoints_detector_pipeline.py:191-197) and
`resize_keeping_aspect_ratio` (:200-272): what happens to boxes and keypoints, and the numbers the per-pixel kernel
`mpn_keypoint_augment` (csrc/augment.hip) needs, packed into one descriptor per image (`DESC_DTYPE`, the layout of
`mpn_keypoint_augment_desc` in include/mpn.h). The pixels themselves never pass through here.

Randomness: TensorFlow's random streams cannot be reproduced, so every draw comes from one `np.random.Generator` with
the reference's distributions, in a fixed order per image (rotation, crop, colour, grayscale, pixel scale, flip). The
same generator state and the same images give the same descriptors, boxes and keypoints.
"""
import math

import numpy as np

from ..constants import DIVISOR, DOWNSAMPLE, NUM_KEYPOINTS, OVERLAP_THRESHOLD

F = np.float32
EPSILON = F(1e-8)                                   # detector/constants.py:16

ROTATE, COLOR, GRAYSCALE, PIXEL_SCALE, FLIP, EVAL = 1, 2, 4, 8, 16, 32   # MPN_AUGMENT_* of include/mpn.h

DESC_DTYPE = np.dtype([
    ("src_offset", "<i8"), ("mask_offset", "<i8"),
    ("src_h", "<i4"), ("src_w", "<i4"), ("mask_h", "<i4"), ("mask_w", "<i4"),
    ("crop_y", "<i4"), ("crop_x", "<i4"), ("crop_h", "<i4"), ("crop_w", "<i4"),
    ("valid_h", "<i4"), ("valid_w", "<i4"), ("valid_mh", "<i4"), ("valid_mw", "<i4"),
    ("transform", "<f4", (8,)), ("mask_transform", "<f4", (8,)), ("window", "<f4", (4,)),
    ("scale_y", "<f4"), ("scale_x", "<f4"), ("mask_scale_y", "<f4"), ("mask_scale_x", "<f4"),
    ("color", "<f4", (3,)), ("seed", "<u4"), ("flags", "<i4"), ("reserved", "<i4", (3,)),
])
assert DESC_DTYPE.itemsize == 192

# keypoints_detector_pipeline.py:441: left <-> right
FLIP_ORDER = np.array([0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15])


def mask_size(h, w):
    """create_tfrecords.py:124 / keypoints_detector_pipeline.py:150-153: masks are ceil(H/4) x ceil(W/4)."""
    return math.ceil(h / DOWNSAMPLE), math.ceil(w / DOWNSAMPLE)


def round_half_even(x):
    return np.rint(x)    # tf.round


# ---------------------------------------------------------------- box utilities (detector/utils/box_utils.py:29-60)
def _intersection(b1, b2):
    ymin1, xmin1, ymax1, xmax1 = np.split(b1, 4, axis=1)
    ymin2, xmin2, ymax2, xmax2 = np.split(b2, 4, axis=1)
    h = np.maximum(F(0), np.minimum(ymax1, ymax2.T) - np.maximum(ymin1, ymin2.T))
    w = np.maximum(F(0), np.minimum(xmax1, xmax2.T) - np.maximum(xmin1, xmin2.T))
    return h * w


def _area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def ioa(b1, b2):
    """random_crop.py:187-202: intersection over the area of boxes2, [N, M]."""
    return np.clip(_intersection(b1, b2) / (_area(b2)[None, :] + EPSILON), F(0), F(1))


def prune_non_overlapping_boxes(boxes, window, min_overlap):
    """random_crop.py:128-150: keep boxes whose IOA with the window is >= min_overlap."""
    overlap = ioa(window.reshape(1, 4).astype(F), boxes).max(axis=0) if len(boxes) else np.zeros(0, F)
    keep = np.nonzero(overlap >= F(min_overlap))[0]
    return boxes[keep], keep


def prune_completely_outside_window(boxes, window):
    """random_crop.py:99-125."""
    wy0, wx0, wy1, wx1 = window
    bad = (boxes[:, 0] >= wy1) | (boxes[:, 1] >= wx1) | (boxes[:, 2] <= wy0) | (boxes[:, 3] <= wx0)
    keep = np.nonzero(~bad)[0]
    return boxes[keep], keep


def change_coordinate_frame(boxes, window):
    """random_crop.py:153-184."""
    wh, ww = window[2] - window[0], window[3] - window[1]
    out = np.stack([(boxes[:, 0] - window[0]) / wh, (boxes[:, 1] - window[1]) / ww,
                    (boxes[:, 2] - window[0]) / wh, (boxes[:, 3] - window[1]) / ww], axis=1)
    return np.clip(out, F(0), F(1)).astype(F)


def _zero_outside(keypoints, h, w):
    """random_rotation.py:263-275 / keypoints_detector_pipeline.py:323-349: v = 0 outside [0,h) x [0,w)."""
    y, x = keypoints[:, :, 0], keypoints[:, :, 1]
    ok = (y >= 0) & (x >= 0) & (y < h) & (x < w)
    out = keypoints.copy()
    out[:, :, 2] *= ok.astype(out.dtype)
    return out


# ---------------------------------------------------------------- rotation (random_rotation.py)
def _random_rotation(rng, boxes, keypoints, h, w, max_angle=45):
    """random_rotation.py:34-77, 82-198: returns boxes, keypoints, the image transform and the mask transform."""
    ih, iw = F(h), F(w)
    center = F(0.5) * np.array([ih, iw], F)
    box = boxes[rng.integers(len(boxes))]                  # tf.random_shuffle(boxes)[0]  (:95)
    ymin, xmin, ymax, xmax = box
    bh, bw = ymax - ymin, xmax - xmin
    cy = np.clip(ymin + F(0.5) * bh, F(0.25) * ih, F(0.75) * ih)
    cx = np.clip(xmin + F(0.5) * bw, F(0.2) * iw, F(0.8) * iw)
    # get_random_rotation (:114-151)
    dist = np.abs(cx - F(0.5) * iw) / iw
    decay = max((F(0.6) - F(2.0) * dist) / F(0.6), F(0))
    max_rad = F(max_angle * (3.141592653589793 / 180.0)) * decay
    theta = F(rng.uniform(-max_rad, max_rad)) if max_rad > 0 else F(0)
    rot = np.array([[np.cos(theta), np.sin(theta)], [-np.sin(theta), np.cos(theta)]], F)
    # get_random_scaling (:154-198)
    distance = min(cx, iw - cx)
    necessary = iw / (F(2.0) * distance)
    size_ratio = iw / bw
    max_scale = size_ratio / F(3.0)
    min_scale = min(max(size_ratio / F(8.0), necessary), max_scale - F(1e-4))
    scaler = F(rng.uniform(min_scale, max_scale))
    rot = (rot * scaler).astype(F)
    translation = (center.reshape(1, 2) - np.array([[cy, cx]], F) @ rot).astype(F)
    # transform_boxes (:201-229)
    y0, x0, y1, x1 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    pts = np.concatenate([np.stack(p, 1) for p in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))], 0).astype(F)
    pts = (pts @ rot + translation).astype(F)
    p1, p2, p3, p4 = np.split(pts, 4, axis=0)
    boxes = np.stack([np.minimum(p1[:, 0], p2[:, 0]), np.minimum(p1[:, 1], p3[:, 1]),
                      np.maximum(p3[:, 0], p4[:, 0]), np.maximum(p2[:, 1], p4[:, 1])], 1).astype(F)
    # transform_keypoints (:232-251)
    pts = keypoints[:, :, :2].reshape(-1, 2).astype(F) @ rot + translation
    kp = keypoints.copy()
    kp[:, :, :2] = round_half_even(pts.astype(F)).astype(np.int32).reshape(-1, NUM_KEYPOINTS, 2)
    # correct (:254-288)
    boxes, keep = prune_non_overlapping_boxes(boxes, np.array([0, 0, ih, iw], F), OVERLAP_THRESHOLD)
    boxes = np.stack([np.clip(boxes[:, 0], 0, ih), np.clip(boxes[:, 1], 0, iw),
                      np.clip(boxes[:, 2], 0, ih), np.clip(boxes[:, 3], 0, iw)], 1).astype(F)
    kp = _zero_outside(kp[keep], int(ih), int(iw))
    # get_inverse_transform (:291-330)
    a, b, c, d = rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1]
    inv = (np.array([d, -b, -c, a], F) / (a * d - b * c)).reshape(2, 2).astype(F)
    inv_t = -(translation @ inv).astype(F)[0]
    transform = np.array([inv[0, 0], inv[0, 1], inv_t[1], inv[1, 0], inv[1, 1], inv_t[0], 0, 0], F)
    mask_transform = transform / np.array([1, 1, DOWNSAMPLE, 1, 1, DOWNSAMPLE, 1, 1], F)   # :72-73
    return boxes, kp, transform, mask_transform.astype(F)


# ---------------------------------------------------------------- crop (random_crop.py, TF 1.15 sample_distorted_bounding_box)
def sample_distorted_bounding_box(rng, height, width, boxes, min_object_covered=0.9, aspect_ratio_range=(0.95, 1.05),
                                  area_range=(0.5, 1.0), max_attempts=100):
    """A numpy restatement of TF 1.15 `sample_distorted_bounding_box` (use_image_if_no_bounding_boxes=True) with its
    100 attempts drawn at once: each attempt samples an aspect ratio, an integer height in the range the area bounds
    allow (rounded up or down once if rounding broke the area range), then an offset; the first attempt whose crop
    covers >= min_object_covered of some box (of area >= 1 pixel) wins, and the whole image if none does.
    boxes: normalised [N, 4]. Returns (y, x, h, w) integers and the normalised f32 window."""
    H, W = int(height), int(width)
    rects = [(0, 0, H, W)] if len(boxes) == 0 else [
        (int(F(b[0]) * F(H)), int(F(b[1]) * F(W)), int(F(b[2]) * F(H)), int(F(b[3]) * F(W))) for b in boxes]
    rects = np.array(rects, np.float64)
    n = max_attempts
    aspect = (rng.random(n, dtype=F) * F(aspect_ratio_range[1] - aspect_ratio_range[0]) + F(aspect_ratio_range[0])).astype(F)
    u_h, u_y, u_x = rng.random(n), rng.random(n), rng.random(n)
    min_area = F(area_range[0]) * F(W) * F(H)
    max_area = F(area_range[1]) * F(W) * F(H)
    h = np.rint(np.sqrt((min_area / aspect).astype(F))).astype(np.int64)
    max_h = np.rint(np.sqrt((max_area / aspect).astype(F))).astype(np.int64)
    over = np.rint((max_h * aspect).astype(F)) > W
    max_h = np.where(over, ((W + 0.5 - 1e-7) / aspect).astype(np.int64), max_h)
    max_h = np.minimum(max_h, H)
    h = np.minimum(h, max_h)
    h = h + np.floor(u_h * (max_h - h + 1)).astype(np.int64) * (h < max_h)
    w = np.rint((h * aspect).astype(F)).astype(np.int64)
    area = (w * h).astype(F)
    lo = area < min_area
    h = np.where(lo, h + 1, h)
    w = np.where(lo, np.rint((h * aspect).astype(F)).astype(np.int64), w)
    area = (w * h).astype(F)
    hi = area > max_area
    h = np.where(hi, h - 1, h)
    w = np.where(hi, np.rint((h * aspect).astype(F)).astype(np.int64), w)
    area = (w * h).astype(F)
    ok = (area >= min_area) & (area <= max_area) & (w <= W) & (h <= H) & (w > 0) & (h > 0)
    y = np.where(h < H, np.floor(u_y * np.maximum(H - h, 1)).astype(np.int64), 0)
    x = np.where(w < W, np.floor(u_x * np.maximum(W - w, 1)).astype(np.int64), 0)
    # SatisfiesOverlapConstraints: some box of area >= 1 covered by >= min_object_covered
    ry0, rx0, ry1, rx1 = (rects[:, i][None, :] for i in range(4))
    ih = np.maximum(0, np.minimum(y[:, None] + h[:, None], ry1) - np.maximum(y[:, None], ry0))
    iw = np.maximum(0, np.minimum(x[:, None] + w[:, None], rx1) - np.maximum(x[:, None], rx0))
    obj = (ry1 - ry0) * (rx1 - rx0)
    with np.errstate(divide="ignore", invalid="ignore"):
        covered = ((ih * iw).astype(F) / obj.astype(F)) >= F(min_object_covered)
    covered &= obj >= 1
    ok &= covered.any(axis=1) & (h * w >= 1)
    idx = np.nonzero(ok)[0]
    if idx.size:
        i = idx[0]
        cy, cx, ch, cw = int(y[i]), int(x[i]), int(h[i]), int(w[i])
    else:
        cy, cx, ch, cw = 0, 0, H, W
    window = np.array([F(cy) / F(H), F(cx) / F(W), F(cy + ch) / F(H), F(cx + cw) / F(W)], F)
    return (cy, cx, ch, cw), window


def _random_crop(rng, boxes_abs, keypoints, h, w):
    """randomly_crop_and_resize's `crop` (keypoints_detector_pipeline.py:294-327) + random_image_crop (random_crop.py:6-96).
    boxes_abs are absolute; returns normalised boxes in the crop's frame, keypoints in crop pixels, the crop and window."""
    scaler = np.array([h, w, h, w], F)
    boxes = (boxes_abs / scaler).astype(F)
    crop, window = sample_distorted_bounding_box(rng, h, w, boxes)
    boxes, inside = prune_completely_outside_window(boxes, window)
    boxes, keep = prune_non_overlapping_boxes(boxes, window, OVERLAP_THRESHOLD)
    boxes = change_coordinate_frame(boxes, window)
    kp = keypoints[inside[keep]].copy()
    wy, wx = (window * scaler)[:2]
    kp[:, :, :2] = round_half_even(kp[:, :, :2].astype(F) - np.array([wy, wx], F)).astype(np.int32)
    return boxes, kp, crop, window


def _rescale(boxes_norm, keypoints, old_hw, new_hw):
    """keypoints_detector_pipeline.py:351-384 (`rescale`)."""
    oh, ow = F(old_hw[0]), F(old_hw[1])
    nh, nw = F(new_hw[0]), F(new_hw[1])
    pts = keypoints[:, :, :2].astype(F) * np.array([nh / oh, nw / ow], F)
    boxes = (boxes_norm * np.array([nh, nw, nh, nw], F)).astype(F)
    pts = round_half_even(pts).astype(np.int32)
    kp = keypoints.copy()
    kp[:, :, 0] = np.clip(pts[:, :, 0], 0, int(nh) - 1)
    kp[:, :, 1] = np.clip(pts[:, :, 1], 0, int(nw) - 1)
    return boxes, kp


def flip_left_right(boxes, keypoints, width):
    """random_flip_left_right's `flip` (keypoints_detector_pipeline.py:405-443) on boxes and keypoints."""
    kp = keypoints.copy()
    kp[:, :, 1] = width - 1 - kp[:, :, 1]
    kp = kp[:, FLIP_ORDER]
    wf = F(width)
    b = np.stack([boxes[:, 0], wf - boxes[:, 3], boxes[:, 2], wf - boxes[:, 1]], 1).astype(F)
    return b, kp


def _identity_desc(src_h, src_w):
    d = np.zeros((), DESC_DTYPE)
    mh, mw = mask_size(src_h, src_w)
    d["src_h"], d["src_w"], d["mask_h"], d["mask_w"] = src_h, src_w, mh, mw
    d["crop_h"], d["crop_w"] = src_h, src_w
    d["window"] = np.array([0, 0, 1, 1], F)
    return d


def sample_training(rng, src_h, src_w, boxes, keypoints, image_size):
    """All random decisions of `augmentation` (keypoints_detector_pipeline.py:191-197) for one image of src_h x src_w with
    absolute boxes f32 [P,4] and keypoints int [P,17,3]; image_size = (H, W) of the output.
    Returns (descriptor without buffer offsets, boxes f32 [P',4] absolute in the output, keypoints int32 [P',17,3])."""
    H, W = int(image_size[0]), int(image_size[1])
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    kp = np.asarray(keypoints).astype(np.int32).reshape(-1, NUM_KEYPOINTS, 3)
    d = _identity_desc(src_h, src_w)
    flags = 0
    # 1. rotation, p = 0.7 (:192); an image without persons has no box to rotate around and is left as it is
    if rng.random() < 0.7 and len(boxes):
        boxes, kp, t, mt = _random_rotation(rng, boxes, kp, src_h, src_w)
        d["transform"], d["mask_transform"] = t, mt
        flags |= ROTATE
    # 2. crop, p = 0.9 (:193, :329-335)
    if rng.random() < 0.9:
        boxes_n, kp, (cy, cx, ch, cw), window = _random_crop(rng, boxes, kp, src_h, src_w)
    else:
        boxes_n = (boxes / np.array([src_h, src_w, src_h, src_w], F)).astype(F)
        cy, cx, ch, cw, window = 0, 0, src_h, src_w, np.array([0, 0, 1, 1], F)
    kp = _zero_outside(kp, ch, cw)                                   # correct_keypoints (:337-349, :387-388)
    boxes, kp = _rescale(boxes_n, kp, (ch, cw), (H, W))              # :391-400
    d["crop_y"], d["crop_x"], d["crop_h"], d["crop_w"] = cy, cx, ch, cw
    d["window"] = window
    d["scale_y"], d["scale_x"] = F(ch) / F(H), F(cw) / F(W)          # resize_images: in / out in f32
    d["valid_h"], d["valid_w"] = H, W
    d["valid_mh"], d["valid_mw"] = mask_size(H, W)
    # 3./4. colour p = 0.5, grayscale p = 0.1 (color_augmentations.py:10-44)
    if rng.random() < 0.5:
        br = F(rng.uniform(-32.0 / 255.0, 32.0 / 255.0))
        cb = F(rng.uniform(-0.1, 0.1))
        cr = F(rng.uniform(-0.1, 0.1))
        d["color"] = np.array([F(1.402) * cr + br, F(-0.344136) * cb - F(0.714136) * cr + br, F(1.772) * cb + br], F)
        flags |= COLOR
    if rng.random() < 0.1:
        flags |= GRAYSCALE
    # 5. pixel-value scale p = 0.1 in [0.9, 1.1) (:47-69): only the seed of the per-element hash is drawn here
    if rng.random() < 0.1:
        d["seed"] = np.uint32(rng.integers(0, 1 << 32))
        flags |= PIXEL_SCALE
    # 6. flip p = 0.5 (:403-450)
    if rng.random() < 0.5:
        boxes, kp = flip_left_right(boxes, kp, W)
        flags |= FLIP
    d["flags"] = flags
    return d, boxes, kp


def evaluation_size(src_h, src_w, min_dimension=512, divisor=DIVISOR):
    """resize_keeping_aspect_ratio (:200-272) sizes: (new_h, new_w, padded h, padded w)."""
    assert min_dimension % divisor == 0
    scale_factor = F(min_dimension / min(src_h, src_w))

    def scale(x):
        unpadded = int(round_half_even(F(x) * scale_factor))
        return unpadded, divisor * math.ceil(unpadded / divisor) - unpadded

    if src_h >= src_w:
        (new_h, pad_h), (new_w, pad_w) = scale(src_h), (min_dimension, 0)
    else:
        (new_h, pad_h), (new_w, pad_w) = (min_dimension, 0), scale(src_w)
    return new_h, new_w, new_h + pad_h, new_w + pad_w


def sample_evaluation(src_h, src_w, boxes, keypoints, min_dimension=512, divisor=DIVISOR):
    """resize_keeping_aspect_ratio (keypoints_detector_pipeline.py:200-272): nothing random.
    Returns (descriptor, boxes, keypoints, (h, w) output size)."""
    new_h, new_w, h, w = evaluation_size(src_h, src_w, min_dimension, divisor)
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    kp = np.asarray(keypoints).astype(np.int32).reshape(-1, NUM_KEYPOINTS, 3)
    d = _identity_desc(src_h, src_w)
    d["valid_h"], d["valid_w"] = new_h, new_w
    d["scale_y"], d["scale_x"] = F(src_h) / F(new_h), F(src_w) / F(new_w)
    d["valid_mh"], d["valid_mw"] = mask_size(new_h, new_w)
    d["mask_scale_y"] = F(d["mask_h"]) / F(d["valid_mh"])
    d["mask_scale_x"] = F(d["mask_w"]) / F(d["valid_mw"])
    d["flags"] = EVAL
    scaler = np.array([new_h / src_h, new_w / src_w], F)              # :259-260
    pts = round_half_even(kp[:, :, :2].astype(F) * scaler).astype(np.int32)
    kp = kp.copy()
    kp[:, :, 0] = np.clip(pts[:, :, 0], 0, h - 1)
    kp[:, :, 1] = np.clip(pts[:, :, 1], 0, w - 1)
    boxes = (boxes * np.concatenate([scaler, scaler])).astype(F)
    return d, boxes, kp, (h, w)


def check_descriptors(descs, src_bytes, mask_bytes, H, W):
    """The range checks the kernel leaves to its caller: every image and packed mask lies inside its buffer, and the crop
    and output regions inside the images. Raises ValueError."""
    for i, d in enumerate(np.atleast_1d(descs)):
        sh, sw, mh, mw = int(d["src_h"]), int(d["src_w"]), int(d["mask_h"]), int(d["mask_w"])
        if sh < 1 or sw < 1 or (mh, mw) != mask_size(sh, sw):
            raise ValueError(f"descriptor {i}: bad source size {sh}x{sw} / masks {mh}x{mw}")
        so, mo = int(d["src_offset"]), int(d["mask_offset"])
        if so < 0 or so + sh * sw * 3 > src_bytes:
            raise ValueError(f"descriptor {i}: image outside the source buffer")
        if mo < 0 or mo + (mh * mw * 2 + 7) // 8 > mask_bytes:
            raise ValueError(f"descriptor {i}: masks outside the mask buffer")
        cy, cx, ch, cw = int(d["crop_y"]), int(d["crop_x"]), int(d["crop_h"]), int(d["crop_w"])
        if ch < 1 or cw < 1 or cy < 0 or cx < 0 or cy + ch > sh or cx + cw > sw:
            raise ValueError(f"descriptor {i}: crop outside the image")
        if not (1 <= d["valid_h"] <= H and 1 <= d["valid_w"] <= W and 1 <= d["valid_mh"] <= H // 4
                and 1 <= d["valid_mw"] <= W // 4):
            raise ValueError(f"descriptor {i}: output region outside {H}x{W}")
