"""The cases of tests/golden/plot_maps_goldens.npz: name -> (image uint8 [H,W,3], heatmaps f32 [hh,hw,17], mask f32 [hh,hw]),
all seeded and small. The images are coarse block noise (they compress). make_plot_maps_goldens.py stores them with what the
reference notebook's `plot_maps` makes of them under Pillow and matplotlib."""
import numpy as np

F = np.float32
K = 17


def image(seed, h, w, block=4):
    rng = np.random.RandomState(seed)
    blocks = rng.randint(0, 256, ((h + block - 1) // block, (w + block - 1) // block, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, block, axis=0), block, axis=1)[:h, :w])


def heatmaps(seed, hh, hw):
    """Mostly low values with a few peaks, as a trained head gives them; every channel inside [0, 1]."""
    rng = np.random.RandomState(seed)
    return (rng.uniform(0, 1, (hh, hw, K)) ** 3).astype(F)


def mask(seed, hh, hw, lo=0.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, (hh, hw)).astype(F)


def cases():
    out = {}
    out["exact_x2"] = (image(1, 128, 128), heatmaps(1, 32, 32), mask(101, 32, 32))
    out["ragged"] = (image(2, 50, 38), heatmaps(2, 13, 10), mask(102, 13, 10))
    out["tall_strip"] = (image(3, 24, 136), heatmaps(3, 6, 34), mask(103, 6, 34))
    h = np.random.RandomState(4).uniform(-0.5, 1.5, (16, 16, K)).astype(F)
    h[..., 0] = heatmaps(4, 16, 16)[..., 0]
    h[0, :4, 0] = 0.0                           # exact 0.0 and 1.0 inside a channel of [0, 1]
    h[1, :4, 0] = 1.0
    h[..., 1] = np.nan                          # what a channel with M == m is after the notebook's normalisation
    h[..., 2] = 1.0                             # opaque
    h[..., 3] = 0.0                             # transparent
    h[2, :, 4] = F(1.0) - F(2.0) ** -24         # the largest float32 below 1
    h[3, :, 4] = F(2.0) ** -9                   # x * 256 = 0.5: truncates to entry 0
    h[4, :, 4] = -F(2.0) ** -30                 # just below zero
    h[5, :4, 4] = (np.inf, -np.inf, 255.0 / 256.0, 1.0 / 256.0)
    out["values"] = (image(5, 64, 64), h, mask(105, 16, 16, -0.5, 1.5))
    yy, xx = np.mgrid[:32, :32]
    checker = np.where((yy // 4 + xx // 4) % 2 == 0, 255, 0).astype(np.uint8)          # squares of 4 pixels: edges ring
    out["saturated_frame"] = (np.ascontiguousarray(np.repeat(checker[..., None], 3, axis=2)), heatmaps(6, 8, 8), mask(106, 8, 8))
    out["short_panels"] = (image(7, 16, 40), heatmaps(7, 4, 10), mask(107, 4, 10))      # panels lower than a label: it is cut at the next panel
    return out
