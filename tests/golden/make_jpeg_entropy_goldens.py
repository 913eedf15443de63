"""Generate the goldens of the device's JPEG entropy stage by running PILLOW: four 240x320 4:2:0 quality-90 files whose scans
are longer than one 32 KB group or close to it (smooth, noise, noise with optimised tables, a saturated checkerboard whose
periodic scan never self-synchronises). Only the JPEG bytes are stored, in `tests/golden/jpeg_entropy_goldens.npz`, with the
Pillow version that made them; the pixels they decode to are whatever the host path gives.

Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpeg_entropy_goldens.py
"""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_entropy_goldens.npz")

from jpeg_cases import source  # noqa: E402

CASES = [("240x320_smooth", 31, 'smooth', {}), ("240x320_noise", 32, 'noise', {}), ("240x320_noise_opt", 33, 'noise', {'optimize': True}),
         ("240x320_checker", 34, 'checker', {})]


def main():
    import PIL
    from PIL import Image
    out = {}
    for name, seed, content, extra in CASES:
        buf = io.BytesIO()
        Image.fromarray(source(seed, (240, 320), content)).save(buf, "JPEG", quality=90, subsampling=2, **extra)
        out[f"{name}/jpeg"] = np.frombuffer(buf.getvalue(), np.uint8)
        print(name, len(buf.getvalue()), "bytes")
    out["names"] = np.array([c[0] for c in CASES])
    out["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
