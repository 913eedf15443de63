"""Generate the JPEG goldens by running PILLOW: every case of jpeg_cases.py is encoded with `Image.save(format="JPEG")` and
decoded again with `Image.open(...).convert("RGB")` (libjpeg-turbo underneath, its default slow-integer inverse DCT and fancy
upsampling).

Only the JPEG bytes and the pixels Pillow decoded are stored in `tests/golden/jpeg_goldens.npz`, together with the Pillow
version that made them.

Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpeg_goldens.py
"""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_goldens.npz")

from jpeg_cases import CASES, SUBSAMPLING, source  # noqa: E402


def encode(seed, shape, content, mode, quality, extra):
    from PIL import Image
    src = source(seed, shape, content)
    buf = io.BytesIO()
    if mode == 'L':
        Image.fromarray(src[:, :, 0]).save(buf, "JPEG", quality=quality, **extra)
    elif mode == 'cmyk':
        Image.fromarray(src).convert("CMYK").save(buf, "JPEG", quality=quality, **extra)
    elif mode == 'progressive':
        Image.fromarray(src).save(buf, "JPEG", quality=quality, progressive=True, **extra)
    else:
        Image.fromarray(src).save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[mode], **extra)
    return buf.getvalue()


def decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    import PIL
    out, names = {}, []
    for name, seed, shape, content, mode, quality, extra in CASES:
        data = encode(seed, shape, content, mode, quality, extra)
        pixels = decode(data)
        assert pixels.shape == shape + (3,) and pixels.dtype == np.uint8
        out[f"{name}/jpeg"], out[f"{name}/pixels"] = np.frombuffer(data, np.uint8), pixels
        names.append(name)
    out["names"] = np.array(names)
    out["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
