"""numpy restatement of Pillow's `Image.resize` for an 8-bit RGB image (default filter: antialiased bicubic) on the tables of
`multiposenet_amd.inference.resample.resample_tables`, and of what `mpn_image_resize` leaves in its output canvas. The yardstick
of tests/test_image_resize_host.py (against Pillow's own outputs) and of the GPU tests (against the kernel, byte for byte).

A pass is clip8((sum(pixel * coeff) + 2^21) >> 22) in integers; horizontal first, rounded to uint8, then vertical; a pass whose
input and output sizes are equal is skipped."""
import numpy as np

from multiposenet_amd.inference.resample import PRECISION_BITS, resample_tables, resized_size


def _pass(a, axis, out_size):
    """One pass along `axis` (0 = vertical, 1 = horizontal) of a uint8 [h, w, 3] array."""
    in_size = a.shape[axis]
    if in_size == out_size:
        return a
    bounds, coeffs = resample_tables(in_size, out_size)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + a.shape[1:], np.uint8)
    for i in range(out_size):
        s, n = bounds[i]
        acc = np.tensordot(coeffs[i, :n].astype(np.int64), a[s:s + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                          # the kernel accumulates in int32
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(image, out_h, out_w):
    """uint8 [h, w, 3] -> uint8 [out_h, out_w, 3], equal to np.asarray(Image.fromarray(image).resize((out_w, out_h)))."""
    return np.ascontiguousarray(_pass(_pass(np.asarray(image, np.uint8), 1, out_w), 0, out_h))


def canvas(image, height, width, keep_aspect_ratio=False):
    """What mpn_image_resize writes for one source: the resized image at the top left of a zero height x width canvas."""
    new_h, new_w = resized_size(image.shape[0], image.shape[1], height, width, keep_aspect_ratio)
    out = np.zeros((height, width, 3), np.uint8)
    out[:new_h, :new_w] = resize(image, new_h, new_w)
    return out
