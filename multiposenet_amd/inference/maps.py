"""Host side of the heatmap and mask overlays (`mpn_plot_maps`, include/mpn.h): the reference notebook's `plot_maps`
(inference/predict.ipynb, the cells under "Show heatmaps") made on the device - the frame at half size with each of the 17
keypoint heatmaps and the segmentation mask laid over it, 18 labelled panels stacked vertically, byte for byte what Pillow and
matplotlib make there. Here: what stays on the host - the Lanczos coefficient tables (resample.resample_tables), the
colormap's 256 RGBA bytes, the label stamps (rendered once per process with Pillow's default font) - packed into one int32
buffer with the descriptor that says where each part lies; the device buffers of one (B, H, W, hh, hw); the launch."""
import functools

import numpy as np

from .. import _lib
from .resample import MAX_KSIZE, resample_tables

PANELS = 18
NUM_KEYPOINTS = 17
DESC_WORDS = 16                        # mpn_plot_maps_desc in 32-bit words (64 bytes; checked against the library)
STAMP_WORDS = 8                        # one label's descriptor in the tables
# the notebook's ORDER (the COCO keypoint order) and its last panel
LABELS = ('nose', 'left eye', 'right eye', 'left ear', 'right ear', 'left shoulder', 'right shoulder', 'left elbow',
          'right elbow', 'left wrist', 'right wrist', 'left hip', 'right hip', 'left knee', 'right knee', 'left ankle',
          'right ankle', 'segmentation mask')


def muldiv255(a, b):
    """Pillow's MULDIV255 on integer arrays: a * b / 255 rounded."""
    t = np.asarray(a, np.int64) * b + 128
    return ((t >> 8) + t) >> 8


@functools.lru_cache(maxsize=1)
def colour_table():
    """uint8 [256, 4]: matplotlib's 'autumn' with alpha sqrt(g), as `(255 * cmap(...)).astype('uint8')` gives its entries:
    the float rows are (1, g, 0, sqrt(g)), g = linspace(0, 1, 256). Read-only."""
    g = np.linspace(0, 1, 256)
    rows = np.stack([np.ones_like(g), g, np.zeros_like(g), np.sqrt(g)], axis=1)
    table = (255 * rows).astype('uint8')
    table.setflags(write=False)
    return table


def premultiplied_table():
    """The colour table as Pillow's RGBA -> RGBa conversion leaves it (every band MULDIV255 by alpha): what the resize reads."""
    table = colour_table().astype(np.int64)
    out = table.copy()
    out[:, :3] = muldiv255(table[:, :3], table[:, 3:])
    return out.astype(np.uint8)


@functools.lru_cache(maxsize=1)
def label_stamps():
    """[(mask uint8 [sh, sw], (ox, oy))] of LABELS: what `ImageDraw.text` blends for each string in Pillow's default font, and
    where (the offset `font.getmask2` reports, added to the text's position). Rendered once per process."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default()
    stamps = []
    for text in LABELS:
        core, (ox, oy) = font.getmask2(text, 'L')
        sw, sh = core.size
        mask = np.zeros((max(sh, 0), max(sw, 0)), np.uint8)
        if sw > 0 and sh > 0:
            im = Image.new('L', (sw, sh), 0)
            ImageDraw.Draw(im).text((-ox, -oy), text, fill=255, font=font)      # the mask itself: BLEND8(m, 0, 255) = m
            mask = np.asarray(im).copy()
        mask.setflags(write=False)
        stamps.append((mask, (int(ox), int(oy))))
    return stamps


def check_arrays(image, heatmaps, segmentation_mask):
    """The argument checks of `plot_maps`: uint8 [H, W, 3] (H, W >= 2), float32 [hh, hw, 17], float32 [hh, hw]."""
    for name, a, dtype in (('image', image, np.uint8), ('heatmaps', heatmaps, np.float32),
                           ('segmentation_mask', segmentation_mask, np.float32)):
        if not isinstance(a, np.ndarray):
            raise ValueError(f"{name} must be a numpy array")
        if a.dtype != dtype:
            raise ValueError(f"{name} must be {np.dtype(dtype).name} (got {a.dtype})")
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 2 or image.shape[1] < 2:
        raise ValueError(f"image must be [height, width, 3] with height, width >= 2 (got {tuple(image.shape)})")
    if heatmaps.ndim != 3 or heatmaps.shape[2] != NUM_KEYPOINTS or heatmaps.shape[0] < 1 or heatmaps.shape[1] < 1:
        raise ValueError(f"heatmaps must be [h, w, {NUM_KEYPOINTS}] (got {tuple(heatmaps.shape)})")
    if tuple(segmentation_mask.shape) != tuple(heatmaps.shape[:2]):
        raise ValueError(f"segmentation_mask must be {tuple(heatmaps.shape[:2])}, the heatmaps' size (got {tuple(segmentation_mask.shape)})")


def tables_for(H, W, hh, hw):
    """(tables int32 [n], desc int32 [DESC_WORDS]) for frames [H, W] and maps [hh, hw]: the four Lanczos axes (W -> w, H -> h,
    hw -> w, hh -> h; w = W // 2, h = H // 2), the premultiplied colour table (one RGBA pixel per word), the 18 stamp
    descriptors (byte offset, sw, sh, ox, oy) and the stamps' packed L8 pixels. The descriptor holds word offsets."""
    H, W, hh, hw = int(H), int(W), int(hh), int(hw)
    if H < 2 or W < 2 or hh < 1 or hw < 1:
        raise ValueError(f"plot_maps: frames must be at least 2 x 2 and maps 1 x 1 (got {H} x {W}, {hh} x {hw})")
    h, w = H // 2, W // 2
    parts, words = [], 0
    desc = np.zeros(DESC_WORDS, np.int32)

    def put(a):
        nonlocal words
        at = words
        a = np.ascontiguousarray(a).reshape(-1)
        pad = (-a.size) % 4                                           # every part starts at a multiple of 16 bytes
        parts.extend((a, np.zeros(pad, np.int32)))
        words += a.size + pad
        return at

    for i, (n_in, n_out) in enumerate(((W, w), (H, h), (hw, w), (hh, h))):
        bounds, coeffs = resample_tables(n_in, n_out, 'lanczos')
        if coeffs.shape[1] > MAX_KSIZE:
            raise ValueError(f"plot_maps: a resize of {n_in} to {n_out} needs {coeffs.shape[1]} taps per output; the kernels' "
                             f"tap loops cover {MAX_KSIZE}")
        desc[3 * i:3 * i + 3] = (put(bounds), put(coeffs), coeffs.shape[1])
    desc[12] = put(np.ascontiguousarray(premultiplied_table()).view(np.int32))     # R in the low byte
    stamps = label_stamps()
    sdesc, pixels, at = np.zeros((PANELS, STAMP_WORDS), np.int32), [], 0
    for j, (mask, (ox, oy)) in enumerate(stamps):
        sdesc[j, :5] = (at, mask.shape[1], mask.shape[0], ox, oy)
        pixels.append(mask.reshape(-1))
        at += mask.size
    packed = np.concatenate(pixels + [np.zeros((-at) % 4, np.uint8)])
    desc[13] = put(sdesc)
    desc[14] = put(packed.view(np.int32))
    desc[15] = at
    return np.concatenate(parts).astype(np.int32), desc


class MapPlotter:
    """`plot_maps` for batches of B frames [H, W, 3] with maps [hh, hw]: holds the tables and stamps on the device, the
    workspace of the horizontal pass, the min / max keys and the output [B, 18 * (H // 2), W // 2, 4]. `launch` queues the
    kernels on the current stream over device tensors (grids depend on the shape alone: it can be captured); `__call__`
    takes host arrays."""

    def __init__(self, b, H, W, hh, hw, device=None):
        import torch
        lib = _lib.lib()
        if lib.mpn_plot_maps_desc_bytes() != DESC_WORDS * 4:
            raise _lib.MpnError("mpn_plot_maps: the descriptor's layout is not the one this binding was written against")
        self.device = torch.device(device) if device is not None else _lib.current_device()
        self.shape = (int(b), int(H), int(W), int(hh), int(hw))
        b, H, W, hh, hw = self.shape
        tables, desc = tables_for(H, W, hh, hw)
        work = lib.mpn_plot_maps_workspace_bytes(b, H, W, hh, hw)
        if work == 0:
            raise ValueError(f"plot_maps: a batch of {b} frames {H} x {W} with maps {hh} x {hw} is more than mpn_plot_maps "
                             "takes in one launch")
        self.desc = np.ascontiguousarray(desc)                          # HOST: read by the launcher, not by the kernels
        self.tables = torch.from_numpy(tables).to(self.device)
        self.work = torch.empty(work, dtype=torch.uint8, device=self.device)
        self.keys = torch.empty(b * NUM_KEYPOINTS * 2, dtype=torch.int32, device=self.device)
        self.out = torch.empty((b, PANELS * (H // 2), W // 2, 4), dtype=torch.uint8, device=self.device)

    def launch(self, frames, heatmaps, mask, normalise=False):
        """frames uint8 [B, H, W, 3], heatmaps float32 [B, hh, hw, 17], mask float32 [B, hh, hw] or None, contiguous device
        tensors -> the output tensor (this object's own: the next launch overwrites it). normalise: (x - m) / (M - m) per
        frame and channel first, as the notebook does before it calls `plot_maps`."""
        import torch
        b, H, W, hh, hw = self.shape
        for name, t, shape, dtype in (('frames', frames, (b, H, W, 3), torch.uint8),
                                      ('heatmaps', heatmaps, (b, hh, hw, NUM_KEYPOINTS), torch.float32),
                                      ('mask', mask, (b, hh, hw), torch.float32)):
            if t is None and name == 'mask':
                continue
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"plot_maps: {name} must be a contiguous {dtype} device tensor {shape} (got {tuple(t.shape)}, {t.dtype})")
        keys = None
        if normalise:
            _lib.call("mpn_heatmap_minmax", _lib.ptr(heatmaps), b, hh, hw, NUM_KEYPOINTS, _lib.ptr(self.keys), _lib.stream_ptr())
            keys = self.keys
        _lib.call("mpn_plot_maps", _lib.ptr(frames), _lib.ptr(heatmaps), _lib.ptr(mask), _lib.ptr(keys), _lib.ptr(self.tables),
                  self.tables.numel(), self.desc.ctypes.data, b, H, W, hh, hw, _lib.ptr(self.out), _lib.ptr(self.work),
                  self.work.numel(), _lib.stream_ptr())
        return self.out

    def __call__(self, images, heatmaps, masks, normalise=False):
        """Host arrays uint8 [B, H, W, 3], float32 [B, hh, hw, 17], float32 [B, hh, hw] -> uint8 [B, 18 * (H // 2), W // 2, 4]."""
        import torch
        with torch.cuda.device(self.device):
            dev = [torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (images, heatmaps, masks)]
            out = self.launch(*dev, normalise=normalise).cpu().numpy()
        return out


_plotters = {}


def plot_maps(image, heatmaps, segmentation_mask):
    """The notebook's `plot_maps` for one frame, on the device.

    Arguments:
        image: a numpy uint8 array [H, W, 3].
        heatmaps: a numpy float32 array [hh, hw, 17], used as given (the notebook normalises them before the call).
        segmentation_mask: a numpy float32 array [hh, hw].
    Returns a numpy uint8 array [18 * (H // 2), W // 2, 4]: the RGBA image the notebook shows, byte for byte.
    """
    check_arrays(image, heatmaps, segmentation_mask)
    key = (1,) + tuple(image.shape[:2]) + tuple(heatmaps.shape[:2]) + (str(_lib.current_device()),)
    plotter = _plotters.get(key)
    if plotter is None:
        if len(_plotters) >= 8:                                        # a few shapes stay resident, not every one ever seen
            _plotters.pop(next(iter(_plotters)))
        plotter = _plotters[key] = MapPlotter(*key[:5])
    return plotter(image[None], heatmaps[None], segmentation_mask[None])[0]
