"""Generate golden frames for the detection drawing by running the REFERENCE notebook's own `draw_everything`
(inference/predict.ipynb, cells 10 and 12: `EDGES` and the function) under Pillow.

The notebook is read as JSON at generation time and the two cells are executed as they stand; none of their text is kept.
Only the seeded inputs (draw_cases.py) and the RGBA frames Pillow produced are stored in `tests/golden/draw_cases.npz`,
together with the Pillow and numpy versions that made them.

Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_draw_goldens.py      (MPN_REFERENCE: the reference checkout)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "draw_cases.npz")
CELLS = (10, 12)
REF = os.environ.get("MPN_REFERENCE", "/root/reference")

from draw_cases import cases  # noqa: E402


def notebook_draw():
    import PIL
    from PIL import Image, ImageDraw
    with open(os.path.join(REF, "inference", "predict.ipynb")) as f:
        nb = json.load(f)
    scope = {"np": np, "Image": Image, "ImageDraw": ImageDraw}
    for c in CELLS:
        exec("".join(nb["cells"][c]["source"]), scope)
    return scope["draw_everything"], Image, PIL.__version__


def main():
    draw, Image, version = notebook_draw()
    out, names = {}, []
    for name, (img, boxes, pos) in cases().items():
        res = np.asarray(draw(Image.fromarray(img), {"boxes": boxes, "keypoint_positions": pos}))
        assert res.shape == img.shape[:2] + (4,) and res.dtype == np.uint8
        out[f"{name}/image"], out[f"{name}/boxes"], out[f"{name}/keypoint_positions"] = img, boxes, pos
        out[f"{name}/annotated"] = res
        names.append(name)
    out["names"] = np.array(names)
    out["pillow_version"], out["numpy_version"] = np.array(version), np.array(np.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
