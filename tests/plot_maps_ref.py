"""numpy restatement of the reference notebook's `plot_maps` (inference/predict.ipynb) as Pillow and matplotlib compute it,
stage by stage in integers: the colormap lookup, the RGBA resize (premultiply, two Lanczos passes through an 8-bit
intermediate, un-premultiply), `Image.alpha_composite`, the paste and the label blend. The yardstick of
tests/test_plot_maps_host.py (against the goldens Pillow made) and of the GPU tests (against the kernels, byte for byte).

Only the Lanczos tables and the label stamps come from the product (multiposenet_amd.inference: resample_tables, label_stamps);
the host tests pin both against Pillow."""
import numpy as np

from multiposenet_amd.inference.maps import label_stamps
from multiposenet_amd.inference.resample import PRECISION_BITS, resample_tables

I = np.int64


def colour_table():
    """matplotlib's 'autumn' with the notebook's alpha, as bytes: rows (1, g, 0, sqrt(g)) * 255 truncated."""
    g = np.linspace(0, 1, 256)
    return (255 * np.stack([np.ones(256), g, np.zeros(256), np.sqrt(g)], axis=1)).astype(np.uint8)


def colourise(x):
    """`(255 * cmap(x)).astype('uint8')` for a float32 array -> uint8 [..., 4]."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * np.float32(256)
        idx = np.where(np.isfinite(t), t, 0).astype(I)              # truncation toward zero
        idx = np.where(t < 0, 0, np.where(t >= 256, 255, idx))      # under -> first entry, x == 1 and over -> last entry
    out = colour_table()[np.clip(idx, 0, 255)]
    out[np.isnan(t)] = 0                                            # bad -> (0, 0, 0, 0)
    return out


def _div255(t):
    t = t + 128
    return ((t >> 8) + t) >> 8


def _pass(a, axis, out_size):
    """One Lanczos pass along `axis` of a uint8 [h, w, c] array (Pillow skips a pass between equal sizes)."""
    in_size = a.shape[axis]
    if in_size == out_size:
        return a
    bounds, coeffs = resample_tables(in_size, out_size, "lanczos")
    a = np.moveaxis(a, axis, 0).astype(I)
    out = np.empty((out_size,) + a.shape[1:], np.uint8)
    for i in range(out_size):
        s, n = bounds[i]
        acc = np.tensordot(coeffs[i, :n].astype(I), a[s:s + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                          # Pillow and the kernels accumulate in int32
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def lanczos(a, out_h, out_w):
    """uint8 [h, w] or [h, w, c] -> Pillow's `resize((out_w, out_h), Image.LANCZOS)` of an L / RGB image (no alpha handling)."""
    a = np.asarray(a, np.uint8)
    b = a[..., None] if a.ndim == 2 else a
    b = _pass(_pass(b, 1, out_w), 0, out_h)
    return np.ascontiguousarray(b[..., 0] if a.ndim == 2 else b)


def lanczos_rgba(a, out_h, out_w):
    """Pillow's resize of an RGBA image: to premultiplied 'RGBa' (MULDIV255), the passes, back (alpha 0 or 255 copies the
    pixel, else clip8(255 * c / a))."""
    a = np.asarray(a, np.uint8).astype(I)
    pm = a.copy()
    pm[..., :3] = _div255(a[..., :3] * a[..., 3:])
    r = lanczos(pm.astype(np.uint8), out_h, out_w).astype(I)
    alpha = r[..., 3:]
    safe = np.where(alpha == 0, 1, alpha)
    rgb = np.where((alpha == 0) | (alpha == 255), r[..., :3], np.minimum(255 * r[..., :3] // safe, 255))
    return np.concatenate([rgb, alpha], axis=-1).astype(np.uint8)


def alpha_composite(dst, src):
    """Pillow's `Image.alpha_composite(dst, src)` (AlphaComposite.c) on uint8 [h, w, 4] arrays."""
    d, s = dst.astype(I), src.astype(I)
    da, sa = d[..., 3:], s[..., 3:]
    blend = da * (255 - sa)
    outa255 = sa * 255 + blend
    coef1 = sa * 255 * 255 * 128 // np.where(outa255 == 0, 1, outa255)
    coef2 = 255 * 128 - coef1
    t = s[..., :3] * coef1 + d[..., :3] * coef2 + (0x80 << 7)
    rgb = (((t >> 8) + t) >> 8) >> 7
    a = outa255 + 0x80
    a = ((a >> 8) + a) >> 8
    out = np.concatenate([rgb, a], axis=-1)
    return np.where(sa == 0, d, out).astype(np.uint8)


def blend_stamp(frame, mask, x0, y0, ink=(255, 0, 0, 255)):
    """`ImageDraw.Draw(im, 'RGBA').text` on an opaque RGBA frame, in place: BLEND8 of the ink on all four bands, clipped."""
    h, w = frame.shape[:2]
    sh, sw = mask.shape
    ya, yb, xa, xb = max(y0, 0), min(y0 + sh, h), max(x0, 0), min(x0 + sw, w)
    if ya >= yb or xa >= xb:
        return
    m = mask[ya - y0:yb - y0, xa - x0:xb - x0].astype(I)[..., None]
    frame[ya:yb, xa:xb] = _div255(frame[ya:yb, xa:xb].astype(I) * (255 - m) + np.array(ink, I) * m)


def normalise(heatmaps):
    """Notebook cell 20: (h - m) / (M - m) per channel, in float32; a channel with M == m becomes NaN."""
    h = np.asarray(heatmaps, np.float32)
    m, M = h.min(0).min(0), h.max(0).max(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (h - m) / (M - m)


def plot_maps(image, heatmaps, segmentation_mask):
    """uint8 [H, W, 3], float32 [hh, hw, 17], float32 [hh, hw] -> uint8 [18 * (H // 2), W // 2, 4], in the notebook's order of
    operations: every panel is pasted, then labelled on the whole picture (a label that leaves its panel is overwritten by
    the next paste or clipped by the picture)."""
    H, W, _ = image.shape
    h, w = H // 2, W // 2
    stamps = label_stamps()
    out = np.full((18 * h, w, 4), 255, np.uint8)
    frame = np.concatenate([lanczos(image, h, w), np.full((h, w, 1), 255, np.uint8)], axis=-1)
    heat = colourise(heatmaps)                                       # [hh, hw, 17, 4]
    for j in range(18):
        if j < 17:
            over = lanczos_rgba(heat[:, :, j], h, w)
        else:
            m = (255 * np.clip(np.asarray(segmentation_mask, np.float32), 0.0, 1.0)).astype(np.uint8)
            band = lanczos(m, h, w)
            over = np.repeat(band[..., None], 4, axis=-1)
        out[j * h:(j + 1) * h] = alpha_composite(frame, over)
        mask, (ox, oy) = stamps[j]
        blend_stamp(out, mask, ox, j * h + oy)
    return out
