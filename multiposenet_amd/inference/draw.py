"""Host side of the annotated frames (`mpn_draw_detections`, include/mpn.h): the reference notebook's `draw_everything`
(inference/predict.ipynb, cells 10 and 12) drawn on the device - the frame as RGBA, every kept person's box in red, skeleton in
white, keypoints as red dots, byte for byte what Pillow draws there. Here: where every frame of a ragged batch lies in the
packed output, the descriptors, the device buffers of one batch shape and the launch."""
import numpy as np

from .. import _lib
from .resample import _round16

DESC_WORDS = 8                         # mpn_draw_desc in 32-bit words (32 bytes; checked against the library)
MAX_BOXES = 128                        # MPN_DRAW_MAX_BOXES


def out_capacity(source_bytes, b):
    """Bytes of packed RGBA output that hold ANY b frames whose packed RGB sources fit source_bytes (each frame's h*w*4 is
    rounded up to 16 bytes)."""
    return _round16(int(source_bytes) // 3 * 4 + 16 * b)


def layout(shapes, src_offsets):
    """[(h, w)] and the byte offsets of the frames in the packed sources -> (descriptors int32 [b, DESC_WORDS],
    frames [(out_offset, h, w)], out_bytes)."""
    desc = np.zeros((len(shapes), DESC_WORDS), np.int32)
    d64 = desc.view(np.int64)                                    # words 0-1 src_offset, 2-3 out_offset
    frames, at = [], 0
    for i, ((h, w), src) in enumerate(zip(shapes, src_offsets)):
        d64[i, 0], d64[i, 1] = src, at
        desc[i, 4:6] = (h, w)
        frames.append((at, int(h), int(w)))
        at += _round16(h * w * 4)
    return desc, frames, at


class Buffers:
    """The device side of the drawing for b frames of at most `source_bytes` packed RGB bytes: descriptors (with their pinned
    staging), the packed output, the primitive workspace, and an empty record for a graph without a person detector."""

    def __init__(self, b, max_boxes, source_bytes, device):
        import torch
        lib = _lib.lib()
        if lib.mpn_draw_desc_bytes() != DESC_WORDS * 4:
            raise _lib.MpnError("mpn_draw_detections: the descriptor's layout is not the one this binding was written against")
        work = lib.mpn_draw_detections_workspace_bytes(b, max_boxes)
        if work == 0:
            raise ValueError(f"annotate: {b} x {max_boxes} slots are more than mpn_draw_detections draws in one launch "
                             f"(max_boxes <= {MAX_BOXES}, b * max_boxes <= 4096)")
        self.b, self.max_boxes = b, max_boxes
        self.desc_stage = torch.zeros((b, DESC_WORDS), dtype=torch.int32).pin_memory()
        self.desc = torch.zeros((b, DESC_WORDS), dtype=torch.int32, device=device)
        self.out = torch.empty(out_capacity(source_bytes, b), dtype=torch.uint8, device=device)
        self.work = torch.empty(work, dtype=torch.uint8, device=device)
        self.no_record = torch.zeros(lib.mpn_pose_gather_record_bytes(b, max_boxes), dtype=torch.uint8, device=device)
        self.frames, self.out_bytes = [], 0

    def place(self, shapes, src_offsets):
        """This call's frames: the descriptors go to the device (one small copy, ordered before the launch on the stream)."""
        desc, self.frames, self.out_bytes = layout(shapes, src_offsets)
        if self.out_bytes > self.out.numel():
            raise ValueError("annotate: the frames exceed the output buffer")     # (out_capacity rules it out)
        self.desc_stage.numpy()[...] = desc
        self.desc.copy_(self.desc_stage, non_blocking=True)

    def launch(self, sources, record, with_keypoints):
        """sources: flat uint8 device tensor; record: mpn_pose_gather's (None: no persons) -> the packed RGBA output."""
        record = self.no_record if record is None else record
        _lib.call("mpn_draw_detections", _lib.ptr(sources), sources.numel(), _lib.ptr(self.desc), _lib.ptr(record), record.numel(),
                  self.b, self.max_boxes, int(bool(with_keypoints)), _lib.ptr(self.out), self.out.numel(), _lib.ptr(self.work),
                  self.work.numel(), _lib.stream_ptr())
        return self.out

    def unpack(self, host):
        """A host copy of the packed output -> the frames as uint8 [h, w, 4] arrays of their own."""
        return [host[at:at + h * w * 4].reshape(h, w, 4).copy() for at, h, w in self.frames]
