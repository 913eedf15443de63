"""The cases of tests/golden/pil_resize_goldens.npz: (name, seed, (src_h, src_w), (out_h, out_w)). The sources are seeded
random uint8 images (every side <= 160); make_pil_resize_goldens.py stores them with Pillow's outputs."""
import numpy as np

CASES = [
    ("down_2x", 1, (64, 96), (32, 48)),                 # integer reduction
    ("down_3_75x", 2, (150, 111), (40, 30)),            # non-integer reductions (3.75, 3.7)
    ("down_8x", 3, (160, 160), (20, 20)),               # ksize 33
    ("down_7_3x", 4, (146, 160), (20, 22)),             # non-integer, near the 8x row
    ("up", 5, (20, 30), (64, 96)),
    ("identity", 6, (48, 64), (48, 64)),                # neither pass runs
    ("one_row", 7, (1, 37), (16, 24)),
    ("one_column", 8, (29, 1), (8, 8)),
    ("horizontal_only", 9, (40, 100), (40, 32)),
    ("vertical_only", 10, (100, 40), (32, 40)),
    ("up_x_down_y", 11, (120, 20), (32, 64)),
]


def source(seed, shape):
    return np.random.RandomState(seed).randint(0, 256, tuple(shape) + (3,)).astype(np.uint8)
