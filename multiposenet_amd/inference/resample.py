"""Host side of `Detector.predict_images`: Pillow's `Image.resize` (its default filter for an 8-bit RGB image: antialiased
bicubic) restated as integer coefficient tables, the letterbox geometry, and the packing of a ragged batch for
`mpn_image_resize` (include/mpn.h).

Pillow resizes an 8-bit image in two separable passes of FIXED-POINT arithmetic: once the coefficient tables exist, every pixel
is `clip8((sum(pixel * coeff) + 2^21) >> 22)` in int32, the horizontal pass first, its result rounded to uint8 before the
vertical pass, a pass whose input and output sizes are equal skipped. The tables are float64 host arithmetic and are built here;
the device does only the integer part, so its output equals Pillow's byte for byte.
"""
import functools
import math

import numpy as np

PRECISION_BITS = 22                    # fractional bits of a coefficient
MAX_KSIZE = 65                         # MPN_IMAGE_RESIZE_MAX_KSIZE: the longest tap row the kernels accept (a 16x reduction)
DESC_WORDS = 16                        # mpn_image_resize_desc in 32-bit words (64 bytes; checked against the library)


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    """Pillow's `Image.LANCZOS`: sinc(x) * sinc(x / 3), truncated to -3 <= x < 3."""
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


FILTERS = {'bicubic': (_bicubic, 2.0), 'lanczos': (_lanczos, 3.0)}     # name -> (kernel, support)


@functools.lru_cache(maxsize=512)
def resample_tables(in_size, out_size, filter='bicubic'):
    """The taps of one axis: `bounds` int32 [out_size, 2] = (first tap, tap count) and `coeffs` int32 [out_size, ksize].

    Bicubic with a = -0.5, support 2 * max(in/out, 1), ksize = ceil(support) * 2 + 1; output x has its centre at
    (x + 0.5) * in/out and taps int(centre - support + 0.5) .. int(centre + support + 0.5) clipped to [0, in_size); the weights
    are float64, normalised by their sum (added in tap order), then fixed point with 22 fractional bits rounded half away from
    zero. filter='lanczos' (Pillow's `Image.LANCZOS`, of inference/plot_maps): the same rules with sinc(x) * sinc(x / 3) on
    |x| < 3 and support 3 * max(in/out, 1). Cached per (in_size, out_size, filter): a video stream builds its tables once. The
    arrays are read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_tables: sizes must be >= 1 (got {in_size} -> {out_size})")
    if filter not in FILTERS:
        raise ValueError(f"resample_tables: filter must be one of {sorted(FILTERS)} (got {filter!r})")
    kernel, support = FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [kernel((x + xmin - center + 0.5) * ss) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[xx] = (xmin, n)
        coeffs[xx, :n] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


def check_size(size):
    """(height, width) of the network input, both positive multiples of 128 (the reference's assert, inference/detector.py:45)."""
    try:
        height, width = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (height, width) (got {size!r})")
    if height < 128 or width < 128 or height % 128 or width % 128:
        raise ValueError(f"size must be positive multiples of 128 (got {height} x {width})")
    return height, width


def check_images(images):
    """The argument checks of `Detector.predict_images`, before any device work: a non-empty list of uint8 [h, w, 3] arrays
    with h, w >= 1 (the sizes may all differ). Returns the list."""
    if isinstance(images, np.ndarray) and images.ndim == 3:
        raise ValueError("images must be a list of [height, width, 3] arrays (got one array)")
    items = list(images)
    if len(items) < 1:
        raise ValueError("empty batch")
    for im in items:
        if not isinstance(im, np.ndarray):
            raise ValueError("images must be numpy arrays")
        if im.dtype != np.uint8:
            raise ValueError("image must be uint8")
        if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError(f"an image must be [height, width, 3] with height, width >= 1 (got {tuple(im.shape)})")
    return items


def resized_size(h, w, height, width, keep_aspect_ratio):
    """(new_h, new_w) of an h x w source on a height x width canvas. Without `keep_aspect_ratio`: the canvas. With it, in
    float64: s = min(height / h, width / w), new_h = max(1, round(h * s)), new_w = max(1, round(w * s)) (Python's `round`:
    half to even), neither above the canvas."""
    if not keep_aspect_ratio:
        return height, width
    s = min(height / h, width / w)
    return min(height, max(1, round(h * s))), min(width, max(1, round(w * s)))


def extent_of(h, w, new_h, new_w, height, width):
    """f32 (box_scale_y, box_scale_x, pixel_height, pixel_width) of mpn_pose_gather_sized: a box normalised to the canvas times
    (height / new_h, width / new_w) (float64, rounded to f32) is normalised to the source; its pixels are the source's."""
    return np.array([height / new_h, width / new_w, h, w], np.float64).astype(np.float32)


def _round16(n):
    return (int(n) + 15) // 16 * 16


def capacity_for(n):
    """A buffer capacity: n rounded up to a power of two."""
    n = max(int(n), 1)
    return 1 << (n - 1).bit_length()


class Plan:
    """The packing of one ragged batch for mpn_image_resize: where every source, intermediate and table lies.

    sizes        [(h, w)] of the sources, new_sizes [(new_h, new_w)], extents f32 [b, 4]
    stage_bytes  of the packed sources (+ 4: the kernel reads a pixel as one dword, one byte past it)
    meta         int32 words: b descriptors, b extents (f32 bits), then the tables (each (in, out) pair once)
    work_bytes   of the uint8 intermediates [src_h, stride(new_w * 3 -> 16)] behind each other
    """

    def __init__(self, shapes, height, width, keep_aspect_ratio=False, align=1):
        """align: every source starts at a multiple of it (16 for sources that mpn_jpeg_decode writes)."""
        b = len(shapes)
        self.b, self.height, self.width = b, height, width
        self.sizes = [(int(h), int(w)) for h, w in shapes]
        self.new_sizes = [resized_size(h, w, height, width, keep_aspect_ratio) for h, w in self.sizes]
        self.extents = np.stack([extent_of(h, w, nh, nw, height, width) for (h, w), (nh, nw) in zip(self.sizes, self.new_sizes)])
        tables, words, table_at = [], 0, {}

        def place(in_size, out_size):
            nonlocal words
            key = (in_size, out_size)
            if key not in table_at:
                bounds, coeffs = resample_tables(in_size, out_size)
                if coeffs.shape[1] > MAX_KSIZE:
                    raise ValueError(f"a resize of {in_size} to {out_size} needs {coeffs.shape[1]} taps per output; the kernel's "
                                     f"tap loop covers {MAX_KSIZE} (a reduction of up to {(MAX_KSIZE - 1) // 4}x)")
                table_at[key] = (words, words + bounds.size, coeffs.shape[1])
                tables.extend((bounds.reshape(-1), coeffs.reshape(-1)))
                words += bounds.size + coeffs.size
            return table_at[key]

        desc = np.zeros((b, DESC_WORDS), np.int32)
        d64 = desc.view(np.int64)                                    # words 0-1 src_offset, 2-3 tmp_offset
        src_at = tmp_at = 0
        self.src_offsets = []
        for i, ((h, w), (nh, nw)) in enumerate(zip(self.sizes, self.new_sizes)):
            bx, cx, kx = place(w, nw)
            by, cy, ky = place(h, nh)
            stride = _round16(nw * 3)
            src_at = (src_at + align - 1) // align * align
            d64[i, 0], d64[i, 1] = src_at, tmp_at
            desc[i, 4:15] = (h, w, nh, nw, bx, cx, by, cy, kx, ky, stride)
            self.src_offsets.append(src_at)
            src_at += h * w * 3
            tmp_at += h * stride
        self.stage_bytes = src_at + 4
        self.work_bytes = max(tmp_at, 16)
        self.table_words = words
        self.meta = np.concatenate([desc.reshape(-1), self.extents.reshape(-1).view(np.int32)] + tables)

    @property
    def meta_words(self):
        return self.meta.size
