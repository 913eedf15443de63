"""Handmade cases of `mpn_anonymize`, shared by tests/test_anonymize_host.py (the reference against Pillow, its properties) and
tests/test_anonymize_gpu.py (the kernels against the reference): frames, persons and the spec grid. The kernels' tile is
32 x 32 pixels; the frames are small so that the reference stays quick, except where a size is the point."""
import itertools

import numpy as np

F = np.float32
NAN, INF = float('nan'), float('inf')


def frame(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def person(h, w, box, face=None, spread=4.0, score=0.5, joints=5):
    """box: (y0, x0, y1, x1) in pixels -> (box f32 [4] normalised, keypoints f32 [17, 3]). face: (x, y) of the nose; the eyes
    lie spread / 2 beside and spread / 3 above it, the ears spread beside it; the first `joints` face joints score `score`,
    the others -1 (below every threshold used here). The body joints are scattered over the box and never read."""
    y0, x0, y1, x1 = box
    b = np.array([y0 / h, x0 / w, y1 / h, x1 / w], F)
    kp = np.zeros((17, 3), F)
    fx, fy = face if face is not None else ((x0 + x1) / 2, y0 + (y1 - y0) / 8)
    kp[:5, 0] = fx + np.array([0, spread / 2, -spread / 2, spread, -spread])
    kp[:5, 1] = fy + np.array([0, -spread / 3, -spread / 3, 0, 0])
    kp[:5, 2] = -1.0
    kp[:joints, 2] = score
    kp[5:, 0] = np.linspace(x0, x1, 12)
    kp[5:, 1] = np.linspace(y0, y1, 12)
    kp[5:, 2] = 0.9
    return b, kp


def _case(name, image, persons, with_keypoints=True):
    h, w, _ = image.shape
    made = [person(h, w, *p) if not isinstance(p[0], np.ndarray) else p for p in persons]
    boxes = np.stack([b for b, _ in made]).astype(F) if made else np.zeros((0, 4), F)
    kps = np.stack([k for _, k in made]).astype(F) if made else np.zeros((0, 17, 3), F)
    return name, image, boxes, kps, with_keypoints


def _broken(h, w, what):
    b, kp = person(h, w, (10, 10, 60, 50), (30, 20))
    if what == 'box_nan':
        b[2] = NAN
    elif what == 'box_inf':
        b[1] = -INF
    elif what == 'joint_nan':
        kp[1, 0] = NAN
    elif what == 'joint_inf':
        kp[3, 1] = INF
    elif what == 'score_nan':                                       # a NaN score is not in F: the others decide
        kp[0, 2] = NAN
    return b, kp


def _grid(h, w, n, seed):
    """n persons spread over an h x w frame, some partly outside."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        y0, x0 = rng.uniform(-0.1 * h, 0.8 * h), rng.uniform(-0.1 * w, 0.8 * w)
        out.append(((y0, x0, y0 + rng.uniform(8, 0.5 * h), x0 + rng.uniform(6, 0.4 * w)), None, rng.uniform(1, 6)))
    return out


def cases(full=25):
    """[(name, image, boxes, keypoints, with_keypoints)]; `full`: the persons of the full image (max_boxes)."""
    H, W = 70, 90
    return [
        _case("inside_one_tile", frame(1, H, W), [((2, 2, 30, 28), (14, 12), 3.0)]),
        _case("crossing_tiles", frame(2, H, W), [((5, 10, 68, 80), (45, 34), 12.0)]),
        _case("edges_and_corner", frame(3, H, W), [((20, -15, 50, 12), (-2, 30), 5.0), ((-12, 30, 20, 60), (45, -3), 5.0),
                                                   ((25, 75, 60, 100), (91, 35), 5.0), ((55, 30, 90, 60), (45, 71), 5.0),
                                                   ((-10, -10, 14, 14), (1, 1), 4.0), ((50, 70, 80, 100), (89, 69), 4.0)]),
        _case("entirely_outside", frame(4, H, W), [((10, 120, 40, 150), (135, 20), 4.0), ((-60, 10, -20, 40), (25, -40), 4.0)]),
        _case("no_face_joint", frame(5, H, W), [((8, 12, 64, 58), (35, 16), 4.0, 0.5, 0)]),
        _case("one_face_joint", frame(6, H, W), [((8, 12, 64, 58), (35, 18), 4.0, 0.5, 1)]),
        _case("boxes_only", frame(7, H, W), [((8, 12, 64, 58), (35, 16), 4.0), ((30, 40, 69, 88), (60, 36), 3.0)], False),
        # (rows 35 / 70 and columns 45 / 90 are exact in float32: the products are integers, floor == ceil)
        _case("zero_area_box", frame(8, H, W), [((35, 15, 35, 60), (37, 30), 5.0), ((10, 45, 50, 45), (40, 15), 0.0, 0.5, 0)]),
        _case("not_finite", frame(9, H, W), [_broken(H, W, k) for k in ('box_nan', 'box_inf', 'joint_nan', 'joint_inf', 'score_nan')]),
        _case("two_overlapping", frame(10, H, W), [((5, 5, 60, 50), (28, 22), 6.0), ((15, 25, 68, 80), (40, 30), 6.0)]),
        _case("three_overlapping", frame(11, H, W), [((5, 5, 60, 50), (30, 25), 7.0), ((10, 20, 65, 70), (42, 30), 7.0),
                                                     ((0, 30, 50, 85), (36, 20), 7.0)]),
        _case("larger_than_the_frame", frame(12, H, W), [((-40, -50, 120, 150), (45, 35), 60.0)]),
        _case("nobody", frame(13, 33, 47), []),
        _case("full", frame(14, 97, 131), _grid(97, 131, full, 15)),
        _case("frame_1x1", frame(16, 1, 1), [((0, 0, 1, 1), (0.5, 0.5), 1.0)]),
        _case("frame_5x3", frame(17, 5, 3), [((0, 0, 5, 3), (1.5, 1.0), 1.0)]),
        _case("frame_2x2047", frame(18, 2, 2047), [((0, 100, 2, 400), (250, 1), 40.0), ((0, 1990, 2, 2060), (2040, 1), 10.0)]),
        _case("frame_17x4099", frame(19, 17, 4099), [((0, 4000, 17, 4099), (4080, 8), 6.0), ((2, -20, 15, 70), (10, 8), 9.0)]),
    ]


REGIONS, MODES, SHAPES = ('head', 'box'), ('pixelate', 'blur', 'fill'), ('ellipse', 'rectangle')
GRID = list(itertools.product(MODES, SHAPES, REGIONS))              # every case runs for all 12
# the ends of the integer parameters, and the other float parameters away from their defaults
EXTRA = [dict(mode='pixelate', blocks=2), dict(mode='pixelate', blocks=32, region='box'), dict(mode='blur', radius=1),
         dict(mode='blur', radius=12, region='box', shape='rectangle'),
         dict(mode='fill', color=(255, 128, 1), scale=3.5, min_size=0.3, fallback=1.0, min_keypoint_score=0.6, shape='rectangle')]
