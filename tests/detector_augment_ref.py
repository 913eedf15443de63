"""numpy restatement of `mpn_detector_augment` (csrc/detector_augment.hip), the yardstick of
tests/test_detector_pipeline_gpu.py.

Each step is the TF 1.15 operation the reference's detector pipeline runs per image, on whole materialised images and in the
reference's order, with the same float32 operations (numpy never fuses a multiply-add), so the kernel - which composes the
two resamples per pixel and stores no intermediate image - is compared bit for bit:
  convert_image_dtype        u8 * float32(1/255)
  slice                      the crop window
  resize_images (legacy)     in = out * f32(in/out), lo = floor, hi = min(lo+1, in-1), top + (bottom-top)*lerp
  pad_to_bounding_box        zeros around (evaluation: bottom / right; randomly_pad: anywhere)
  colour / grayscale / pixel scale over the whole canvas, then flip_left_right.
Nothing of the product is imported except the flag values (compared in the tests).
"""
import numpy as np

from keypoint_augment_ref import hash_uniform

F = np.float32
COLOR, GRAYSCALE, PIXEL_SCALE, FLIP, EVAL, PAD = 2, 4, 8, 16, 32, 64


def resize_bilinear(img, out_h, out_w, scale_y, scale_x):
    """Legacy tf.image.resize_images BILINEAR (align_corners=False) of f32 [h,w,3] with the given f32 in/out scales."""
    h, w = img.shape[:2]
    iny = np.arange(out_h, dtype=F) * F(scale_y)
    inx = np.arange(out_w, dtype=F) * F(scale_x)
    fy, fx = np.floor(iny), np.floor(inx)
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    ly, lx = (iny - fy)[:, None, None], (inx - fx)[None, :, None]
    tl, tr = img[y0][:, x0], img[y0][:, x1]
    bl, br = img[y1][:, x0], img[y1][:, x1]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    return (top + (bot - top) * ly).astype(F)


def place(img, y, x, H, W):
    """tf.image.pad_to_bounding_box."""
    out = np.zeros((H, W, 3), F)
    out[y:y + img.shape[0], x:x + img.shape[1]] = img
    return out


def augment_image(src_u8, d, H, W):
    """One image: src uint8 [h,w,3], d a descriptor record -> f32 [H,W,3]."""
    flags = int(d["flags"])
    img = src_u8.astype(F) * F(1.0 / 255.0)
    cy, cx, ch, cw = (int(d[k]) for k in ("crop_y", "crop_x", "crop_h", "crop_w"))
    img = img[cy:cy + ch, cx:cx + cw]
    vh, vw = int(d["valid_h"]), int(d["valid_w"])
    v = place(resize_bilinear(img, vh, vw, d["scale_y"], d["scale_x"]), 0, 0, H, W)          # stage 2
    if flags & PAD:                                                                            # stage 3
        ph, pw = int(d["pad_h"]), int(d["pad_w"])
        v = place(resize_bilinear(v, ph, pw, d["pad_scale_y"], d["pad_scale_x"]), int(d["pad_y"]), int(d["pad_x"]), H, W)
    if flags & COLOR:
        v = np.minimum(np.maximum(v + d["color"].astype(F), F(0)), F(1))
    if flags & GRAYSCALE:
        g = F(0.2989) * v[..., 0] + F(0.5870) * v[..., 1] + F(0.1140) * v[..., 2]
        v = np.repeat(g[..., None], 3, axis=2)
    if flags & PIXEL_SCALE:
        u = hash_uniform(d["seed"], np.arange(H * W * 3, dtype=np.uint32).reshape(H, W, 3))
        coef = u * (F(d["maxval"]) - F(d["minval"])) + F(d["minval"])
        v = np.minimum(np.maximum(v * coef, F(0)), F(1))
    if flags & FLIP:
        v = v[:, ::-1]
    return np.ascontiguousarray(v, F)


def augment_batch(sources, descs, H, W):
    """sources: the concatenated uint8 buffer the kernel reads; descs: descriptor records [B] -> images f32 [B,H,W,3]."""
    out = np.zeros((len(descs), H, W, 3), F)
    for b, d in enumerate(descs):
        so, sh, sw = int(d["src_offset"]), int(d["src_h"]), int(d["src_w"])
        out[b] = augment_image(np.asarray(sources[so:so + sh * sw * 3], np.uint8).reshape(sh, sw, 3), d, H, W)
    return out
