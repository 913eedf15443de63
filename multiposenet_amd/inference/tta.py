"""Host side of the Detector's test-time augmentation (flip=, scales=): the launches of mpn_mirror_images and mpn_tta_merge
(include/mpn.h) and the persistent buffers of one graph entry - the inputs of the extra scales with the fixed
mpn_image_resize descriptors that fill them from the base input, and the merged maps everything downstream reads."""
import ctypes

import torch

from .. import _lib
from . import resample

MAX_SOURCES = 8                        # MPN_TTA_MAX_SOURCES
MAX_SCALES = 3                         # extra scales beside the base: with flip, 2 * (1 + 3) sources


class Source(ctypes.Structure):
    """mpn_tta_source."""
    _fields_ = [('heat', ctypes.c_void_p), ('seg', ctypes.c_void_p), ('h', ctypes.c_int32), ('w', ctypes.c_int32),
                ('mirrored', ctypes.c_int32), ('reserved', ctypes.c_int32)]


def mirror_images(src, dst):
    """dst[i, y, x, :] = src[i, y, w-1-x, :] for uint8 [n, h, w, 3] device tensors (contiguous, different memory)."""
    n, h, w, _ = src.shape
    if dst.shape != src.shape or src.dtype != torch.uint8 or dst.dtype != torch.uint8 or src.shape[3] != 3:
        raise ValueError("mirror_images: src and dst must be uint8 [n, h, w, 3] of one shape")
    if not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("mirror_images: src and dst must be contiguous")
    _lib.call("mpn_mirror_images", _lib.ptr(src), n, h, w, _lib.ptr(dst), _lib.stream_ptr())


def merge(sources, heat_out, seg_out):
    """sources: [(heat f32 [b, h_k, w_k, 17], seg f32 [b, h_k, w_k], mirrored)] in the order they are summed -> heat_out f32
    [b, h0, w0, 17], seg_out f32 [b, h0, w0]. One launch; the sources travel by value in its arguments."""
    if not 1 <= len(sources) <= MAX_SOURCES:
        raise ValueError(f"tta merge: {len(sources)} sources, 1 .. {MAX_SOURCES} are taken")
    b, h0, w0, k = heat_out.shape
    table = (Source * len(sources))()
    for i, (heat, seg, mirrored) in enumerate(sources):
        row = table[i]
        if (heat.dtype != torch.float32 or seg.dtype != torch.float32 or heat.shape[0] != b or heat.shape[3] != k
                or tuple(seg.shape) != tuple(heat.shape[:3]) or not (heat.is_contiguous() and seg.is_contiguous())):
            raise ValueError("tta merge: a source is f32 heat [b, h, w, 17] and seg [b, h, w], contiguous")
        row.heat, row.seg, row.h, row.w, row.mirrored = heat.data_ptr(), seg.data_ptr(), heat.shape[1], heat.shape[2], int(mirrored)
    if k != 17 or tuple(seg_out.shape) != (b, h0, w0) or not (heat_out.is_contiguous() and seg_out.is_contiguous()):
        raise ValueError("tta merge: the outputs are f32 heat [b, h0, w0, 17] and seg [b, h0, w0], contiguous")
    _lib.call("mpn_tta_merge", ctypes.cast(table, ctypes.c_void_p), len(sources), b, h0, w0, _lib.ptr(heat_out),
              _lib.ptr(seg_out), _lib.stream_ptr())


def network_input(n, h, w, device):
    """uint8 [n, h, w, 3] with slack behind it: mpn_image_resize reads a source pixel as one dword, a byte past its end."""
    flat = torch.empty(n * h * w * 3 + 16, dtype=torch.uint8, device=device)
    return flat[:n * h * w * 3].view(n, h, w, 3)


class Buffers:
    """The persistent state of one graph entry with flip or scales: `x`, the base network input [passes * b, h, w, 3] (the
    second half is the mirror of the first); per extra scale its input [passes * b, H_k, W_k, 3] and the descriptors, tables
    and intermediates of the mpn_image_resize that fills its first half from x[:b] - fixed per entry, placed once here; the
    merged maps."""

    def __init__(self, flip, scales, b, h, w, device):
        self.flip, self.b = bool(flip), b
        passes = 2 if flip else 1
        self.x = network_input(passes * b, h, w, device)
        self.scales = []
        for wk, hk in scales:
            plan = resample.Plan([(h, w)] * b, hk, wk)
            self.scales.append((network_input(passes * b, hk, wk, device), torch.from_numpy(plan.meta.copy()).to(device),
                                torch.empty(plan.work_bytes, dtype=torch.uint8, device=device)))
        self.heat = torch.empty((b, h // 4, w // 4, 17), dtype=torch.float32, device=device)
        self.seg = torch.empty((b, h // 4, w // 4), dtype=torch.float32, device=device)

    def fill(self, x, xk, meta, work):
        """The input of one extra scale from the base input: Pillow's bicubic of x[:b], then its mirror."""
        b = self.b
        _, hk, wk, _ = xk.shape
        _lib.call("mpn_image_resize", _lib.ptr(x), _lib.ptr(meta[b * (resample.DESC_WORDS + 4):]), _lib.ptr(meta), b, hk, wk,
                  _lib.ptr(xk), _lib.ptr(work), work.numel(), _lib.stream_ptr())
        if self.flip:
            mirror_images(xk[:b], xk[b:])
