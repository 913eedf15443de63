"""Generate the JPEG-encode goldens by running PILLOW: every case of jpeg_encode_cases.py is written with
`Image.save(buf, "JPEG", quality=q, subsampling=s)` (libjpeg-turbo underneath: slow-integer forward DCT, standard Huffman
tables, no restart intervals). An RGBA case is saved from `convert("RGB")`.

`tests/golden/jpeg_encode_goldens.npz` holds, per case, the source pixels and Pillow's file bytes, and the Pillow version
that wrote them. The generator fails unless the set exercises byte stuffing, ZRL symbols and dummy blocks on each edge.

Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpeg_encode_goldens.py
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(os.path.dirname(HERE))]          # the case table; the package (its host Huffman decoder)

OUT = os.path.join(HERE, "jpeg_encode_goldens.npz")

from jpeg_encode_cases import CASES, SUBSAMPLING, source  # noqa: E402

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
SAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}


def pillow_encode(pixels, quality, subsampling):
    from PIL import Image
    image = Image.fromarray(pixels)
    if image.mode != "RGB":
        image = image.convert("RGB")
    buf = io.BytesIO()
    image.save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[subsampling])
    return buf.getvalue()


def scan_of(data):
    """The entropy-coded segment of a one-scan file, through its EOI marker."""
    at = data.index(b"\xff\xda")
    return data[at + 2 + ((data[at + 2] << 8) | data[at + 3]):]


def _has_zrl(data):
    """Some block of the file has 16 or more zeros in a row, in zig-zag order, in front of a non-zero coefficient."""
    from multiposenet_amd.inference import jpeg as J
    z = J.entropy_decode(data).coefs[:, ZIGZAG] != 0
    for row in z[z[:, 17:].any(axis=1)]:
        nz = np.flatnonzero(row)
        if (np.diff(np.concatenate([[0], nz])) > 16).any():
            return True
    return False


def check_set(files):
    """The properties the issue asks of the set; raises AssertionError otherwise."""
    assert any(scan_of(files[c[0]]).count(b"\xff\x00") >= 8 for c in CASES), "no scan with 8 stuffed bytes"
    assert any(_has_zrl(files[c[0]]) for c in CASES), "no block with a run of 16 zeros"
    right = bottom = both = False
    for name, _, (h, w), _, sub, _, _ in CASES:
        hs, vs = SAMPLING[sub]
        r = -(-w // 8) < -(-w // (8 * hs)) * hs
        b = -(-h // 8) < -(-h // (8 * vs)) * vs
        right, bottom, both = right or (r and not b), bottom or (b and not r), both or (r and b)
    assert right and bottom and both, "dummy blocks: right %s, bottom %s, both %s" % (right, bottom, both)


def main():
    import PIL
    out, names, files = {}, [], {}
    for name, seed, shape, content, sub, quality, channels in CASES:
        assert shape[0] <= 120 and shape[1] <= 160
        pixels = source(seed, shape, content, channels)
        data = pillow_encode(pixels, quality, sub)
        out[f"{name}/pixels"], out[f"{name}/jpeg"] = pixels, np.frombuffer(data, np.uint8)
        files[name] = data
        names.append(name)
    check_set(files)
    out["names"] = np.array(names)
    out["versions"] = np.array([f"Pillow {PIL.__version__}", f"numpy {np.__version__}"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
