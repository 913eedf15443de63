"""Generate the progressive / CMYK JPEG goldens by running PILLOW: every case of jpeg_progressive_cases.py is encoded with
`Image.save(format="JPEG")` and decoded again with `Image.open(...).convert("RGB")`; the damaged files are cut from, or
edited in, the bytes of one case and carry no pixels.

Only the JPEG bytes and the pixels Pillow decoded are stored in `tests/golden/jpeg_progressive_goldens.npz`, together with
the Pillow and numpy versions that made them.

Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpeg_progressive_goldens.py
"""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_progressive_goldens.npz")

from jpeg_progressive_cases import CASES, DAMAGED, SUBSAMPLING, damage, scans, source  # noqa: E402


def encode(seed, shape, content, mode, quality, extra):
    from PIL import Image
    src = source(seed, shape, content)
    buf = io.BytesIO()
    if mode == 'pL':
        Image.fromarray(src[:, :, 0]).save(buf, "JPEG", quality=quality, progressive=True, **extra)
    elif mode in ('cmyk', 'pcmyk'):
        Image.fromarray(src).convert("CMYK").save(buf, "JPEG", quality=quality, progressive=mode == 'pcmyk', **extra)
    else:
        Image.fromarray(src).save(buf, "JPEG", quality=quality, progressive=True, subsampling=SUBSAMPLING[mode], **extra)
    return buf.getvalue()


def decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    import PIL
    out, names, files = {}, [], {}
    for name, seed, shape, content, mode, quality, extra in CASES:
        data = files[name] = encode(seed, shape, content, mode, quality, extra)
        pixels = decode(data)
        assert pixels.shape == shape + (3,) and pixels.dtype == np.uint8
        out[f"{name}/jpeg"], out[f"{name}/pixels"] = np.frombuffer(data, np.uint8), pixels
        names.append(name)
    assert len(scans(files[DAMAGED[0][1]])) == sum(d[2] == 'cut' for d in DAMAGED), "one cut per scan of the file"
    for name, base, kind, which in DAMAGED:
        out[f"damaged/{name}"] = np.frombuffer(damage(files[base], kind, which), np.uint8)
    out["names"] = np.array(names)
    out["damaged"] = np.array([d[0] for d in DAMAGED])
    out["versions"] = np.array([f"Pillow {PIL.__version__}", f"numpy {np.__version__}"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "cases", len(DAMAGED), "damaged files", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
