"""Generate golden vectors for the image resize by running PILLOW (`Image.resize` with its default filter, what the
reference's inference/predict.ipynb cell 6 calls before the detector).

Only the seeded inputs and the outputs Pillow produced are stored in `tests/golden/pil_resize_goldens.npz`, together with the
Pillow version that made them.

Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pil_resize_goldens.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pil_resize_goldens.npz")

from pil_resize_cases import CASES, source  # noqa: E402


def main():
    import PIL
    from PIL import Image
    out, names = {}, []
    for name, seed, shape, (oh, ow) in CASES:
        src = source(seed, shape)
        res = np.asarray(Image.fromarray(src).resize((ow, oh)))
        assert res.shape == (oh, ow, 3) and res.dtype == np.uint8
        out[f"{name}/source"], out[f"{name}/resized"] = src, res
        names.append(name)
    out["names"] = np.array(names)
    out["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
