"""numpy restatement of `parse_and_preprocess` of the reference's detector/input_pipeline/prn_pipeline.py for one record,
the yardstick of tests/test_prn_pipeline_gpu.py and of the invariants in tests/test_prn_pipeline_host.py.

Composed from `oracle.heatmap_creation.get_heatmaps` (held to the reference by tests/golden/render_goldens.npz) and
`oracle.prn_post.crop_and_resize` (the published crop_and_resize_op.cc, float32, in its operation order); the label and
flip code below is float32 numpy (which never fuses a multiply-add), every line cited to prn_pipeline.py. The kernel
`mpn_prn_examples` performs the same float operations in the same order, so its output is compared bit for bit.
"""
import numpy as np

from oracle.heatmap_creation import get_heatmaps
from oracle.prn_post import crop_and_resize

F = np.float32
DOWNSAMPLE = 4                  # detector/constants.py:13
CROP_SIZE = (56, 36)            # prn_pipeline.py:6-7: height and width
FLIP_ORDER = np.array([0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15])   # :193


def filter_persons(keypoints, boxes, max_keypoints):
    """prn_pipeline.py:78-89: indices of the persons with at most `max_keypoints` visible keypoints (all for None)."""
    kp = np.asarray(keypoints)
    if max_keypoints is None:
        return np.arange(len(kp))
    is_visible = (kp[:, :, 2] > 0).astype(np.int32)                      # :83
    return np.flatnonzero(is_visible.sum(axis=1) <= max_keypoints)        # :84


def crops_of_image(keypoints, boxes, width, height):
    """prn_pipeline.py:91-103: get_heatmaps of the (kept) people, then crop_and_resize of every box / scaler.
    Returns f32 [P, 56, 36, 17]."""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    heatmaps = get_heatmaps(np.asarray(keypoints), boxes, int(width), int(height), DOWNSAMPLE)   # :91-95
    scaler = np.array([height, width, height, width], F)                # :65: to_float(stack(2 * [height, width]))
    box_indices = np.zeros(len(boxes), np.int32)                         # :97
    return crop_and_resize(heatmaps[None], boxes / scaler, box_indices, CROP_SIZE)   # :98-102


def label_map(keypoints, box):
    """prn_pipeline.py:105-146 (`fn`): keypoints int [17,3] of one person, box f32 [4] -> f32 [56, 36, 17]."""
    height, width = CROP_SIZE
    ymin, xmin, ymax, xmax = [F(v) for v in box]                         # :116
    kp = np.asarray(keypoints).astype(F)                                 # :149: tf.to_float(keypoints)
    y, x, v = kp[:, 0], kp[:, 1], kp[:, 2]                               # :117
    part_id = np.flatnonzero(v > 0)                                      # :120
    h, w = ymax - ymin, xmax - xmin                                      # :128
    with np.errstate(divide="ignore", invalid="ignore"):
        sy, sx = F(height) / h, F(width) / w                             # :131: [height/h, width/w], float32
        ky = np.rint((y[part_id] - ymin) * sy)                           # :133-135: -= translation, *= scaler, tf.round
        kx = np.rint((x[part_id] - xmin) * sx)                           #           (round half to even)
    # :139-140 clip_by_value(to_int32(.), 0, size - 1); clipped before the conversion, equal for every int32 value
    ky = np.clip(ky, 0, height - 1).astype(np.int64)
    kx = np.clip(kx, 0, width - 1).astype(np.int64)
    out = np.zeros((height, width, 17), F)                               # :143-146: sparse -> dense, default 0
    out[ky, kx, part_id] = F(1)
    return out


def flip(crops, labels):
    """prn_pipeline.py:175-195: flip_left_right, then gather the parts in `correct_order`."""
    return crops[:, ::-1][:, :, FLIP_ORDER], labels[:, ::-1][:, :, FLIP_ORDER]


def batch(tables):
    """(crops, labels) f32 [N,56,36,17] of one batch from the tables of `PoseResidualNetworkPipeline.sample` (or hand-made
    ones): 'keypoints' [Q,17,3], 'boxes' [Q,4], 'first_person' [R+1], 'width', 'height' [R], 'examples' with fields image,
    person (global), flip."""
    kp, bx, fp = np.asarray(tables["keypoints"]), np.asarray(tables["boxes"], F), np.asarray(tables["first_person"])
    per_image = {}
    crops, labels = [], []
    for e in tables["examples"]:
        r, q = int(e["image"]), int(e["person"])
        a, b = int(fp[r]), int(fp[r + 1])
        assert a <= q < b
        if r not in per_image:
            per_image[r] = crops_of_image(kp[a:b], bx[a:b], int(tables["width"][r]), int(tables["height"][r]))
        c, l = per_image[r][q - a], label_map(kp[q], bx[q])
        if e["flip"]:
            c, l = flip(c, l)
        crops.append(c)
        labels.append(l)
    shape = (0,) + CROP_SIZE + (17,)
    return (np.stack(crops) if crops else np.zeros(shape, F)), (np.stack(labels) if labels else np.zeros(shape, F))
