"""Generate golden frames for the heatmap and mask overlays by running the REFERENCE notebook's own `plot_maps`
(inference/predict.ipynb: the cell that builds the colormap and the cell that defines `ORDER` and the function) under Pillow
and matplotlib.

The notebook is read as JSON at generation time and the two cells, found by their content, are executed as they stand; none
of their text is kept. Only the seeded inputs (plot_maps_cases.py), the RGBA frames Pillow produced, the colormap's 256 RGBA
bytes and the label names are stored in `tests/golden/plot_maps_goldens.npz`, together with the Pillow, matplotlib and numpy
versions that made them. The frames depend on the installed Pillow's default font (the labels).

Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_plot_maps_goldens.py      (MPN_REFERENCE: the reference checkout)
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plot_maps_goldens.npz")
REF = os.environ.get("MPN_REFERENCE", "/root/reference")

from plot_maps_cases import cases  # noqa: E402


def notebook_plot_maps():
    import matplotlib
    matplotlib.use("Agg")
    import PIL
    from PIL import Image, ImageDraw
    with open(os.path.join(REF, "inference", "predict.ipynb")) as f:
        nb = json.load(f)
    sources = ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]
    cmap_cell, = [s for s in sources if "ListedColormap(" in s and "def " not in s]
    plot_cell, = [s for s in sources if "def plot_maps(" in s]
    scope = {"np": np, "Image": Image, "ImageDraw": ImageDraw}
    exec(cmap_cell, scope)
    exec(plot_cell, scope)
    return scope, Image, PIL.__version__, matplotlib.__version__


def _save(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same file, byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    scope, Image, pillow, mpl = notebook_plot_maps()
    plot_maps, cmap, order = scope["plot_maps"], scope["cmap"], scope["ORDER"]
    out, names = {}, []
    for name, (img, heat, mask) in cases().items():
        with np.errstate(invalid="ignore"):
            res = np.asarray(plot_maps(img, heat, mask))
        h, w = img.shape[0] // 2, img.shape[1] // 2
        assert res.shape == (18 * h, w, 4) and res.dtype == np.uint8
        out[f"{name}/image"], out[f"{name}/heatmaps"], out[f"{name}/mask"], out[f"{name}/maps"] = img, heat, mask, res
        names.append(name)
    out["names"] = np.array(names)
    out["colour_table"] = (255 * cmap(np.arange(cmap.N))).astype("uint8")
    out["labels"] = np.array([order[j] for j in range(17)] + ["segmentation mask"])
    out["pillow_version"], out["matplotlib_version"], out["numpy_version"] = np.array(pillow), np.array(mpl), np.array(np.__version__)
    _save(OUT, out)
    print("wrote", OUT, len(names), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
