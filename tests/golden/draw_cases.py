"""The cases of tests/golden/draw_cases.npz: name -> (image uint8 [h,w,3], boxes f32 [n,4], keypoint_positions f32 [n,17,2]),
all seeded. Frames are at most 160 x 200; the images are coarse block noise (they compress) - the drawing does not read them.
make_draw_goldens.py stores them with what the reference notebook's `draw_everything` draws on them under Pillow."""
import numpy as np

F = np.float32
K = 17


def image(seed, h, w):
    rng = np.random.RandomState(seed)
    blocks = rng.randint(0, 255, ((h + 7) // 8, (w + 7) // 8, 3)).astype(np.uint8)     # (never 255: drawn ink is recognisable)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:h, :w])


def persons(seed, n, lo=0.0, hi=1.0, pos_lo=0.0, pos_hi=1.0):
    """n boxes with corners in [lo, hi] (ymin <= ymax, xmin <= xmax) and positions in [pos_lo, pos_hi]."""
    rng = np.random.RandomState(seed)
    y = np.sort(rng.uniform(lo, hi, (n, 2)), axis=1)
    x = np.sort(rng.uniform(lo, hi, (n, 2)), axis=1)
    boxes = np.stack([y[:, 0], x[:, 0], y[:, 1], x[:, 1]], axis=1).astype(F)
    return boxes, rng.uniform(pos_lo, pos_hi, (n, K, 2)).astype(F)


def _corners(n):
    """positions on the box's corners and edge midpoints, cycling."""
    pts = np.array([(0, 0), (0, 1), (1, 0), (1, 1), (0.5, 0), (0, 0.5), (1, 0.5), (0.5, 1), (0.5, 0.5)], F)
    return np.stack([pts[(np.arange(K) + i) % len(pts)] for i in range(n)]).astype(F)


def cases():
    out = {}
    out["no_persons"] = (image(1, 37, 53), np.zeros((0, 4), F), np.zeros((0, K, 2), F))
    out["one_person"] = (image(2, 96, 128),) + persons(2, 1, 0.1, 0.9)
    out["three_persons_odd_size"] = (image(3, 111, 77),) + persons(3, 3, 0.05, 0.95)
    out["crowd_25"] = (image(4, 160, 200),) + persons(4, 25)
    # boxes on the frame's border exactly, and beyond it on every side
    b = np.array([[0, 0, 1, 1], [-0.2, -0.1, 1.3, 1.2], [0.5, -0.3, 0.7, 0.4], [-0.4, 0.6, 0.3, 1.5], [0.25, 0.25, 1.0, 1.0]], F)
    out["boxes_touch_and_exceed"] = (image(5, 90, 131), b, persons(5, 5)[1])
    out["keypoints_on_box_corners"] = (image(6, 100, 100), persons(6, 4, 0.0, 1.0)[0], _corners(4))
    # positions outside their box: keypoints land outside the frame on all sides
    out["keypoints_outside_frame"] = (image(7, 80, 120),) + persons(7, 6, 0.1, 0.9, -1.5, 2.5)
    c = persons(8, 3, 0.1, 0.9)
    c[1][0, :] = c[1][0, 0]                   # person 0: all 17 keypoints coincide (zero-length lines)
    c[1][1, ::2] = c[1][1, 1]                 # person 1: half of them
    out["coincident_keypoints"] = (image(8, 64, 64),) + c
    base = np.array([0.2, 0.25, 0.8, 0.7], F)
    b = (base + np.random.RandomState(9).uniform(-0.02, 0.02, (8, 4))).astype(F)
    out["heavy_overlap"] = (image(9, 120, 97), b, persons(9, 8, pos_lo=0.3, pos_hi=0.7)[1])
    # dots at x, y < 2 (truncation toward zero changes the dot's size), some just below zero, some exactly zero
    b = np.array([[0.0, 0.0, 0.08, 0.06], [-0.01, -0.012, 0.05, 0.04], [0.0, 0.0, 0.5, 0.5]], F)
    p = persons(10, 3, pos_lo=-0.3, pos_hi=0.6)[1]
    p[2] *= F(0.01)
    p[2, :3] = 0
    p[2, 3] = F(1e-9)
    out["dots_below_two"] = (image(10, 75, 95), b, p)
    out["tiny_frame"] = (image(11, 5, 7),) + persons(11, 2, -0.5, 1.5, -0.5, 1.5)
    out["one_row_frame"] = (image(12, 1, 33),) + persons(12, 2)
    # boxes that truncate to one row / one column / one pixel
    b = np.array([[0.5, 0.1, 0.505, 0.9], [0.1, 0.3, 0.9, 0.302], [0.7, 0.7, 0.7, 0.7]], F)
    out["flat_boxes"] = (image(13, 61, 59), b, persons(13, 3)[1])
    return out
