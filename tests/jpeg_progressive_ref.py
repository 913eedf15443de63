"""Helpers of the progressive / CMYK JPEG tests: the goldens, and the numpy restatement of the four-component colour stage
(the inverse DCT comes from jpeg_decode_ref.py). Written from Pillow's published arithmetic, in int64:

  the library passes the four samples of an Adobe CMYK file through unchanged; Pillow inverts them on load
  (C = 255 - s0, M = 255 - s1, Y = 255 - s2, K = 255 - s3) and `convert("RGB")` computes, with nk = 255 - K,
  R = clip(nk - MULDIV255(C, nk)), MULDIV255(a, b) = (t + (t >> 8)) >> 8 for t = a * b + 128; G from M and B from Y alike."""
import os

import numpy as np

import jpeg_decode_ref as R
from jpeg_progressive_cases import CASES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_progressive_goldens.npz")
_cache = {}


def goldens():
    """{name: (JPEG bytes, Pillow's pixels)} of every case; loaded once, shared, never modified."""
    if 'cases' not in _cache:
        with np.load(GOLDEN) as z:
            assert [str(n) for n in z["names"]] == [c[0] for c in CASES]
            _cache['cases'] = {c[0]: (z[f"{c[0]}/jpeg"].tobytes(), z[f"{c[0]}/pixels"]) for c in CASES}
            _cache['damaged'] = {str(n): z[f"damaged/{n}"].tobytes() for n in z["damaged"]}
            _cache['versions'] = [str(v) for v in z["versions"]]
        for _, pixels in _cache['cases'].values():
            pixels.setflags(write=False)
    return _cache['cases']


def damaged():
    goldens()
    return _cache['damaged']


def versions():
    goldens()
    return _cache['versions']


def muldiv255(a, b):
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def decode_cmyk(planes, width, height):
    """planes: [(coefs [bh, bw, 8, 8], quant [8, 8])] of four 1x1 components -> uint8 [height, width, 3]."""
    s = [R.idct_plane(*p)[:height, :width].astype(np.int64) for p in planes]
    nk = s[3]
    return np.clip(np.stack([nk - muldiv255(255 - s[i], nk) for i in range(3)], axis=2), 0, 255).astype(np.uint8)


def decode_coefficients(c):
    """A `multiposenet_amd.inference.jpeg.Coefficients` of one, three or four components -> uint8 [h, w, 3]."""
    d = c.desc[0]
    if int(d['components']) == 4:
        return decode_cmyk(c.planes(), int(d['width']), int(d['height']))
    return R.decode_coefficients(c)
