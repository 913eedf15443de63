"""numpy restatement of `mpn_keypoint_augment` (csrc/augment.hip), the yardstick of tests/test_keypoint_augment_gpu.py.

Each step is the TF 1.15 operation the reference's keypoint pipeline runs per image, written with the same float32
operations in the same order (numpy never fuses a multiply-add), so the kernel's output is compared bit for bit:
  convert_image_dtype        u8 * float32(1/255)
  ImageProjectiveTransform   BILINEAR (corners floor / floor+1, 0 outside) for images, NEAREST (round half away from
                             zero, 0 outside) for masks      - tensorflow/contrib/image/kernels/image_ops.h
  resize_images (legacy)     in = out * f32(in/out), lo = floor, hi = min(lo+1, in-1), top + (bottom-top)*lerp
  crop_and_resize nearest    in = y1*(h-1) + y*((y2-y1)*(h-1)/(crop-1)), roundf, 0 outside
  resize_nearest_neighbor    min(floor(out * scale), in-1)
  colour / grayscale / pixel scale / flip as described in include/mpn.h.
"""
import numpy as np

F = np.float32
ROTATE, COLOR, GRAYSCALE, PIXEL_SCALE, FLIP, EVAL = 1, 2, 4, 8, 16, 32


def roundf(x):
    """C roundf: half away from zero (x - trunc(x) is exact)."""
    t = np.trunc(x)
    return (t + np.sign(x) * (np.abs(x - t) >= F(0.5))).astype(F)


def fmix32(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h = (h * np.uint32(0x85EBCA6B)).astype(np.uint32)
    h ^= h >> np.uint32(13)
    h = (h * np.uint32(0xC2B2AE35)).astype(np.uint32)
    h ^= h >> np.uint32(16)
    return h


def hash_uniform(seed, idx):
    """u in [0, 1): (fmix32(seed ^ (idx * 0x9E3779B1)) >> 8) * 2^-24 (uint32 arithmetic)."""
    with np.errstate(over="ignore"):
        h = fmix32(np.uint32(seed) ^ (idx.astype(np.uint32) * np.uint32(0x9E3779B1)).astype(np.uint32))
    return (h >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def _read(img, y, x):
    """img f32 [h,w,C]; y, x float arrays; 0 outside (also for NaN)."""
    h, w = img.shape[:2]
    ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    yi = np.where(ok, y, 0).astype(np.int64)
    xi = np.where(ok, x, 0).astype(np.int64)
    return img[yi, xi] * ok[..., None].astype(F)


def _project(t, ox, oy):
    t = t.astype(F)
    proj = t[6] * ox + t[7] * oy + F(1)
    x = (t[0] * ox + t[1] * oy + t[2]) / proj
    y = (t[3] * ox + t[4] * oy + t[5]) / proj
    return y.astype(F), x.astype(F), proj != 0


def _rotated(img, d, ry, rx):
    if not d["flags"] & ROTATE:
        return _read(img, ry.astype(F), rx.astype(F))
    with np.errstate(divide="ignore", invalid="ignore"):
        y, x, ok = _project(d["transform"], rx.astype(F), ry.astype(F))
    yf, xf = np.floor(y), np.floor(x)
    yc, xc = yf + F(1), xf + F(1)
    a, b, c, e = _read(img, yf, xf), _read(img, yf, xc), _read(img, yc, xf), _read(img, yc, xc)
    top = (xc - x)[..., None] * a + (x - xf)[..., None] * b
    bot = (xc - x)[..., None] * c + (x - xf)[..., None] * e
    v = (yc - y)[..., None] * top + (y - yf)[..., None] * bot
    return v * ok[..., None].astype(F)


def augment_image(src_u8, d, H, W):
    """One image: src uint8 [h,w,3], d a DESC_DTYPE record -> f32 [H,W,3]."""
    img = src_u8.astype(F) * F(1.0 / 255.0)
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px = W - 1 - ox if d["flags"] & FLIP else ox
    valid = (oy < d["valid_h"]) & (px < d["valid_w"])
    iny, inx = oy.astype(F) * F(d["scale_y"]), px.astype(F) * F(d["scale_x"])
    fy, fx = np.floor(iny), np.floor(inx)
    y0, x0 = np.maximum(fy.astype(np.int64), 0), np.maximum(fx.astype(np.int64), 0)
    y1, x1 = np.minimum(y0 + 1, d["crop_h"] - 1), np.minimum(x0 + 1, d["crop_w"] - 1)
    ly, lx = (iny - fy)[..., None], (inx - fx)[..., None]
    cy, cx = int(d["crop_y"]), int(d["crop_x"])
    tl, tr = _rotated(img, d, cy + y0, cx + x0), _rotated(img, d, cy + y0, cx + x1)
    bl, br = _rotated(img, d, cy + y1, cx + x0), _rotated(img, d, cy + y1, cx + x1)
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    v = (top + (bot - top) * ly).astype(F)
    if d["flags"] & COLOR:
        v = np.minimum(np.maximum(v + d["color"].astype(F), F(0)), F(1))
    if d["flags"] & GRAYSCALE:
        g = F(0.2989) * v[..., 0] + F(0.5870) * v[..., 1] + F(0.1140) * v[..., 2]
        v = np.repeat(g[..., None], 3, axis=2)
    if d["flags"] & PIXEL_SCALE:
        idx = ((oy.astype(np.uint64) * W + px.astype(np.uint64)) * 3)[..., None] + np.arange(3, dtype=np.uint64)
        u = hash_uniform(d["seed"], (idx & 0xFFFFFFFF).astype(np.uint32))
        coef = u * (F(1.1) - F(0.9)) + F(0.9)
        v = np.minimum(np.maximum(v * coef, F(0)), F(1))
    return np.where(valid[..., None], v, F(0)).astype(F)


def augment_masks(packed, d, H, W):
    """One image's packed masks -> (loss, segmentation) f32 [H/4, W/4]."""
    mh_in, mw_in = int(d["mask_h"]), int(d["mask_w"])
    m = np.unpackbits(np.asarray(packed, np.uint8), count=mh_in * mw_in * 2).reshape(mh_in, mw_in, 2).astype(F)
    mh, mw = H // 4, W // 4
    oy, ox = np.meshgrid(np.arange(mh), np.arange(mw), indexing="ij")
    px = mw - 1 - ox if d["flags"] & FLIP else ox
    if d["flags"] & EVAL:
        ok = (oy < d["valid_mh"]) & (px < d["valid_mw"])
        sy = np.minimum(np.floor(oy.astype(F) * F(d["mask_scale_y"])).astype(np.int64), mh_in - 1)
        sx = np.minimum(np.floor(px.astype(F) * F(d["mask_scale_x"])).astype(np.int64), mw_in - 1)
    else:
        y1, x1, y2, x2 = (F(v) for v in d["window"])
        ih1, iw1 = F(mh_in - 1), F(mw_in - 1)
        if mh > 1:
            iny = y1 * ih1 + oy.astype(F) * ((y2 - y1) * ih1 / F(mh - 1))
        else:
            iny = np.full(oy.shape, F(0.5 * float(y1 + y2) * float(ih1)))
        if mw > 1:
            inx = x1 * iw1 + px.astype(F) * ((x2 - x1) * iw1 / F(mw - 1))
        else:
            inx = np.full(px.shape, F(0.5 * float(x1 + x2) * float(iw1)))
        ok = (iny >= 0) & (iny <= ih1) & (inx >= 0) & (inx <= iw1)
        sy, sx = roundf(np.where(ok, iny, 0)), roundf(np.where(ok, inx, 0))
        if d["flags"] & ROTATE:
            with np.errstate(divide="ignore", invalid="ignore"):
                y, x, pok = _project(d["mask_transform"], sx, sy)
            ry, rx = roundf(np.where(pok, y, -1)), roundf(np.where(pok, x, -1))
            ok &= pok & (ry >= 0) & (ry < mh_in) & (rx >= 0) & (rx < mw_in)
            sy, sx = np.where(ok, ry, 0), np.where(ok, rx, 0)
        sy, sx = sy.astype(np.int64), sx.astype(np.int64)
    ok &= (sy >= 0) & (sy < mh_in) & (sx >= 0) & (sx < mw_in)
    sy, sx = np.where(ok, sy, 0), np.where(ok, sx, 0)
    out = m[sy, sx] * ok[..., None].astype(F)
    return out[..., 0], out[..., 1]


def augment_batch(sources, masks, descs, H, W):
    """sources / masks: the concatenated uint8 buffers the kernel reads; descs: DESC_DTYPE [B].
    Returns images [B,H,W,3], loss_masks, segmentation_masks [B,H/4,W/4] (f32)."""
    B = len(descs)
    imgs = np.zeros((B, H, W, 3), F)
    loss = np.zeros((B, H // 4, W // 4), F)
    seg = np.zeros((B, H // 4, W // 4), F)
    for b, d in enumerate(descs):
        so, sh, sw = int(d["src_offset"]), int(d["src_h"]), int(d["src_w"])
        src = np.asarray(sources[so:so + sh * sw * 3], np.uint8).reshape(sh, sw, 3)
        mo = int(d["mask_offset"])
        nb = (int(d["mask_h"]) * int(d["mask_w"]) * 2 + 7) // 8
        imgs[b] = augment_image(src, d, H, W)
        loss[b], seg[b] = augment_masks(masks[mo:mo + nb], d, H, W)
    return imgs, loss, seg
