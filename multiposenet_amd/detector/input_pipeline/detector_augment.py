"""Per-image random decisions and box geometry of the person-detector input pipeline (host, numpy float32).

Restates the host-visible maths of the reference's `augmentation` (person_detector_pipeline.py:109-116) and
`resize_keeping_aspect_ratio` (:183-242): what happens to the boxes, and the numbers the per-pixel kernel
`mpn_detector_augment` (csrc/detector_augment.hip) needs, packed into one descriptor per image (`DESC_DTYPE`, the layout
of `mpn_detector_augment_desc` in include/mpn.h). The pixels themselves never pass through here.

Randomness: TensorFlow's random streams cannot be reproduced, so every draw comes from one `np.random.Generator` with
the reference's distributions, in a fixed order per image (crop, pad, colour, grayscale, pixel scale, box jitter, flip).
The same generator state and the same images give the same descriptors and boxes.
"""
import numpy as np

from ..constants import DIVISOR
from .keypoint_augment import (COLOR, EVAL, FLIP, GRAYSCALE, PIXEL_SCALE, change_coordinate_frame, evaluation_size,
                               prune_completely_outside_window, prune_non_overlapping_boxes,
                               sample_distorted_bounding_box)

F = np.float32
PAD = 64                                            # MPN_AUGMENT_PAD of include/mpn.h

# probabilities and ranges of person_detector_pipeline.py:109-116
CROP_PROBABILITY, PAD_PROBABILITY = 0.9, 0.1
COLOR_PROBABILITY, GRAYSCALE_PROBABILITY, PIXEL_SCALE_PROBABILITY, FLIP_PROBABILITY = 0.33, 0.033, 0.1, 0.5
CROP_ARGS = dict(min_object_covered=0.9, aspect_ratio_range=(0.85, 1.15), area_range=(0.75, 1.0))   # :122-128
CROP_OVERLAP_THRESHOLD = 0.3
PAD_SCALE_RANGE = (0.5, 0.9)                        # :153
PIXEL_SCALE_RANGE = (0.8, 1.2)                      # :113
JITTER_RATIO = 0.01                                 # :114

DESC_DTYPE = np.dtype([
    ("src_offset", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"),
    ("crop_y", "<i4"), ("crop_x", "<i4"), ("crop_h", "<i4"), ("crop_w", "<i4"),
    ("valid_h", "<i4"), ("valid_w", "<i4"),
    ("pad_y", "<i4"), ("pad_x", "<i4"), ("pad_h", "<i4"), ("pad_w", "<i4"),
    ("scale_y", "<f4"), ("scale_x", "<f4"), ("pad_scale_y", "<f4"), ("pad_scale_x", "<f4"),
    ("color", "<f4", (3,)), ("minval", "<f4"), ("maxval", "<f4"), ("seed", "<u4"), ("flags", "<i4"),
    ("reserved", "<i4", (3,)),
])
assert DESC_DTYPE.itemsize == 112


def _identity_desc(src_h, src_w):
    d = np.zeros((), DESC_DTYPE)
    d["src_h"], d["src_w"] = src_h, src_w
    d["crop_h"], d["crop_w"] = src_h, src_w
    return d


def normalise(boxes, src_h, src_w):
    """person_detector_pipeline.py:92-94: absolute (ymin, xmin, ymax, xmax) -> the [0, 1] range."""
    return (np.asarray(boxes, F).reshape(-1, 4) / np.array([src_h, src_w, src_h, src_w], F)).astype(F)


def random_crop(rng, boxes, src_h, src_w):
    """random_image_crop (random_crop.py:6-70) with the detector's arguments on normalised boxes. Returns the surviving
    boxes in the crop's frame, clipped, and the integer crop (y, x, h, w)."""
    crop, window = sample_distorted_bounding_box(rng, src_h, src_w, boxes, **CROP_ARGS)
    boxes, _ = prune_completely_outside_window(boxes, window)
    boxes, _ = prune_non_overlapping_boxes(boxes, window, CROP_OVERLAP_THRESHOLD)
    return change_coordinate_frame(boxes, window).reshape(-1, 4), crop


def random_pad(rng, boxes, H, W):
    """randomly_pad's `pad` (:143-176): returns boxes, scale, (off_y, off_x, scaled_h, scaled_w)."""
    scale = F(rng.random(dtype=F) * F(PAD_SCALE_RANGE[1] - PAD_SCALE_RANGE[0]) + F(PAD_SCALE_RANGE[0]))
    sh, sw = int(scale * F(H)), int(scale * F(W))                      # tf.to_int32 truncates
    oy, ox = int(rng.integers(0, H - sh)), int(rng.integers(0, W - sw))
    boxes = (boxes * scale).astype(F)                                  # the reference's `scale`, not sh / H (:170)
    translation = np.array([oy / H, ox / W, oy / H, ox / W]).astype(F)  # tf.to_float(offset / height): f64 then f32
    return (boxes + translation).astype(F), scale, (oy, ox, sh, sw)


def jitter_offsets(rng, boxes, ratio=JITTER_RATIO):
    """random_box_jitter's per-box offsets (:260-290): four draws in [-ratio, ratio) times [bh, bw, bh, bw]."""
    n = len(boxes)
    bh, bw = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    u = (rng.random((n, 4), dtype=F) * F(2 * ratio) + F(-ratio)).astype(F)
    return (np.stack([bh, bw, bh, bw], 1).astype(F) * u).astype(F)


def flip_left_right(boxes):
    """random_flip_left_right's `flip` (:247-253) on normalised boxes."""
    return np.stack([boxes[:, 0], F(1) - boxes[:, 3], boxes[:, 2], F(1) - boxes[:, 1]], 1).astype(F)


def sample_training(rng, src_h, src_w, boxes, image_size):
    """All random decisions of `augmentation` (person_detector_pipeline.py:109-116) for one image of src_h x src_w with
    absolute boxes f32 [P,4]; image_size = (H, W) of the output.
    Returns (descriptor without buffer offset, boxes f32 [P',4] normalised to the output, P' >= 0)."""
    H, W = int(image_size[0]), int(image_size[1])
    boxes = normalise(boxes, src_h, src_w)
    d = _identity_desc(src_h, src_w)
    flags = 0
    # 1. crop p = 0.9, then resize to H x W (:119-138)
    cy, cx, ch, cw = 0, 0, src_h, src_w
    if rng.random() < CROP_PROBABILITY:
        boxes, (cy, cx, ch, cw) = random_crop(rng, boxes, src_h, src_w)
    d["crop_y"], d["crop_x"], d["crop_h"], d["crop_w"] = cy, cx, ch, cw
    d["scale_y"], d["scale_x"] = F(ch) / F(H), F(cw) / F(W)             # resize_images: in / out in f32
    d["valid_h"], d["valid_w"] = H, W
    # 2. pad p = 0.1 (:141-180)
    if rng.random() < PAD_PROBABILITY:
        boxes, _, (oy, ox, sh, sw) = random_pad(rng, boxes, H, W)
        d["pad_y"], d["pad_x"], d["pad_h"], d["pad_w"] = oy, ox, sh, sw
        d["pad_scale_y"], d["pad_scale_x"] = F(H) / F(sh), F(W) / F(sw)
        flags |= PAD
    # 3./4. colour p = 0.33, grayscale p = 0.033 (color_augmentations.py:10-44)
    if rng.random() < COLOR_PROBABILITY:
        br = F(rng.uniform(-32.0 / 255.0, 32.0 / 255.0))
        cb = F(rng.uniform(-0.1, 0.1))
        cr = F(rng.uniform(-0.1, 0.1))
        d["color"] = np.array([F(1.402) * cr + br, F(-0.344136) * cb - F(0.714136) * cr + br, F(1.772) * cb + br], F)
        flags |= COLOR
    if rng.random() < GRAYSCALE_PROBABILITY:
        flags |= GRAYSCALE
    # 5. pixel-value scale p = 0.1 in [0.8, 1.2) (:113): only the seed of the per-element hash is drawn here
    if rng.random() < PIXEL_SCALE_PROBABILITY:
        d["seed"] = np.uint32(rng.integers(0, 1 << 32))
        d["minval"], d["maxval"] = PIXEL_SCALE_RANGE
        flags |= PIXEL_SCALE
    # 6. box jitter, always (:114, :260-295)
    boxes = np.clip(boxes + jitter_offsets(rng, boxes), F(0), F(1)).astype(F)
    # 7. flip p = 0.5 (:245-257)
    if rng.random() < FLIP_PROBABILITY:
        boxes = flip_left_right(boxes)
        flags |= FLIP
    d["flags"] = flags
    return d, boxes


def sample_evaluation(src_h, src_w, boxes, min_dimension=640, divisor=DIVISOR):
    """resize_keeping_aspect_ratio (person_detector_pipeline.py:183-242): nothing random.
    Returns (descriptor, boxes normalised to the padded image, (h, w) output size)."""
    new_h, new_w, h, w = evaluation_size(src_h, src_w, min_dimension, divisor)
    d = _identity_desc(src_h, src_w)
    d["valid_h"], d["valid_w"] = new_h, new_w
    d["scale_y"], d["scale_x"] = F(src_h) / F(new_h), F(src_w) / F(new_w)
    d["flags"] = EVAL
    scaler = np.array([new_h / h, new_w / w, new_h / h, new_w / w]).astype(F)     # :233-236: f64 quotients, then f32
    return d, (normalise(boxes, src_h, src_w) * scaler).astype(F), (h, w)


def check_descriptors(descs, src_bytes, H, W):
    """The range checks the kernel leaves to its caller: every image lies inside the source buffer, the crop inside its
    image, the stage-2 region and the placed rectangle inside the H x W canvas. Raises ValueError."""
    for i, d in enumerate(np.atleast_1d(descs)):
        sh, sw = int(d["src_h"]), int(d["src_w"])
        if sh < 1 or sw < 1:
            raise ValueError(f"descriptor {i}: bad source size {sh}x{sw}")
        so = int(d["src_offset"])
        if so < 0 or so + sh * sw * 3 > src_bytes:
            raise ValueError(f"descriptor {i}: image outside the source buffer")
        cy, cx, ch, cw = int(d["crop_y"]), int(d["crop_x"]), int(d["crop_h"]), int(d["crop_w"])
        if ch < 1 or cw < 1 or cy < 0 or cx < 0 or cy + ch > sh or cx + cw > sw:
            raise ValueError(f"descriptor {i}: crop outside the image")
        if not (1 <= d["valid_h"] <= H and 1 <= d["valid_w"] <= W):
            raise ValueError(f"descriptor {i}: output region outside {H}x{W}")
        if d["flags"] & PAD:
            py, px, ph, pw = int(d["pad_y"]), int(d["pad_x"]), int(d["pad_h"]), int(d["pad_w"])
            if ph < 1 or pw < 1 or py < 0 or px < 0 or py + ph > H or px + pw > W:
                raise ValueError(f"descriptor {i}: padded rectangle outside {H}x{W}")
