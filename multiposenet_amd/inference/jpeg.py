"""JPEG decode split between host and device (include/mpn.h, "JPEG decode"): `jpeg_info` and `entropy_decode` are the host
stage (marker scan and Huffman decode in C++, the GIL released: a thread pool runs them in parallel), `JpegBatchDecoder` ships
the coefficients of a batch and launches `mpn_jpeg_decode`, which writes uint8 RGB into a packed source buffer - the bytes Pillow
returns for the same file. Streams outside the supported set (progressive, CMYK, ...) are decoded by Pillow per image and
copied as pixels, inside the same batch."""
import ctypes
import io

import numpy as np

from .. import _lib

DESC_BYTES = 512                        # MPN_JPEG_DESC_BYTES (checked against the library)
REASONS = ('supported', 'malformed', 'progressive', 'arithmetic', 'frame_type', 'precision', 'components', 'colorspace',
           'sampling', 'multiscan', 'dqt16', 'too_large')


class _Header(ctypes.Structure):        # mpn_jpeg_header
    _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32), ('components', ctypes.c_int32),
                ('h_samp', ctypes.c_int32), ('v_samp', ctypes.c_int32), ('restart_interval', ctypes.c_int32),
                ('supported', ctypes.c_int32), ('reason', ctypes.c_int32),
                ('blocks_w', ctypes.c_int32 * 3), ('blocks_h', ctypes.c_int32 * 3),
                ('total_blocks', ctypes.c_int32), ('reserved', ctypes.c_int32), ('coef_bytes', ctypes.c_int64)]


# mpn_jpeg_desc as a numpy record (its three offsets are the caller's)
DESC = np.dtype([('src_offset', np.int64), ('coef_offset', np.int64), ('work_offset', np.int64),
                 ('width', np.int32), ('height', np.int32), ('components', np.int32), ('h_samp', np.int32), ('v_samp', np.int32),
                 ('total_blocks', np.int32), ('blocks_w', np.int32, (3,)), ('blocks_h', np.int32, (3,)),
                 ('reserved', np.int32, (14,)), ('quant', np.uint16, (3, 64))])
assert DESC.itemsize == DESC_BYTES


def _as_bytes(data):
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError("a JPEG must be bytes")
    return bytes(data)


def jpeg_info(data):
    """The header of a JPEG as a dict: 'width', 'height', 'components', 'sampling' (h, v) of the first component,
    'restart_interval', 'supported' (bool), 'reason' (one of REASONS), 'blocks' [(blocks_h, blocks_w)] per component,
    'total_blocks', 'coef_bytes'. A stream whose headers are damaged raises ValueError."""
    data = _as_bytes(data)
    h = _Header()
    _lib.check(_lib.lib().mpn_jpeg_info(data, len(data), ctypes.byref(h)))
    return {'width': h.width, 'height': h.height, 'components': h.components, 'sampling': (h.h_samp, h.v_samp),
            'restart_interval': h.restart_interval, 'supported': bool(h.supported), 'reason': REASONS[h.reason],
            'blocks': [(h.blocks_h[c], h.blocks_w[c]) for c in range(min(h.components, 3))] if h.supported else [],
            'total_blocks': h.total_blocks, 'coef_bytes': h.coef_bytes}


class Coefficients:
    """A JPEG after the host stage: `.shape` (h, w, 3) of the image it decodes to, `.coefs` int16 [total_blocks, 64] (raw
    coefficients, natural order, one plane of blocks per component) and `.desc`, a one-element DESC record."""
    __slots__ = ('shape', 'coefs', 'desc')

    def __init__(self, shape, coefs, desc):
        self.shape, self.coefs, self.desc = shape, coefs, desc

    def planes(self):
        """[(coefficients [blocks_h, blocks_w, 8, 8], quantisation table [8, 8])] per component."""
        d, out, at = self.desc[0], [], 0
        for c in range(int(d['components'])):
            bh, bw = int(d['blocks_h'][c]), int(d['blocks_w'][c])
            out.append((self.coefs[at:at + bh * bw].reshape(bh, bw, 8, 8), d['quant'][c].reshape(8, 8)))
            at += bh * bw
        return out


def entropy_decode(data):
    """The host stage on one SUPPORTED JPEG -> Coefficients. Raises ValueError for a stream that is damaged, truncated or
    outside the supported set (`jpeg_info(data)['supported']`)."""
    data = _as_bytes(data)
    lib = _lib.lib()
    h = _Header()
    _lib.check(lib.mpn_jpeg_info(data, len(data), ctypes.byref(h)))
    if not h.supported:
        raise ValueError(f"entropy_decode: stream not supported ({REASONS[h.reason]})")
    coefs = np.empty((h.total_blocks, 64), np.int16)
    desc = np.zeros(1, DESC)
    _lib.check(lib.mpn_jpeg_entropy_decode(data, len(data), coefs.ctypes.data_as(ctypes.c_void_p), coefs.nbytes,
                                           desc.ctypes.data_as(ctypes.c_void_p)))
    return Coefficients((h.height, h.width, 3), coefs, desc)


def pillow_decode(data):
    """What the device path must equal, and the per-image fallback: Pillow's decode to uint8 [h, w, 3]."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def prepare(item):
    """One entry of a batch, ready for `JpegBatchDecoder`: JPEG bytes -> Coefficients when the stream is supported, else the
    pixels Pillow decodes; a uint8 [h, w, 3] array or a Coefficients passes through. Thread-safe (the pipelines' decode pool)."""
    if isinstance(item, (Coefficients, np.ndarray)):
        return item
    data = _as_bytes(item)
    h = _Header()
    rc = _lib.lib().mpn_jpeg_info(data, len(data), ctypes.byref(h))
    if rc == 0 and h.supported:
        return entropy_decode(data)
    return pillow_decode(data)


def _round16(n):
    return (int(n) + 15) // 16 * 16


def _capacity(n):
    n = max(int(n), 16)
    return 1 << (n - 1).bit_length()


class JpegBatchDecoder:
    """Fills a packed uint8 source buffer on the device from a batch of prepared entries.

        decoder = JpegBatchDecoder(device)
        decoder.decode(entries, sources, offsets, stream)

    entries: Coefficients (decoded on the device by mpn_jpeg_decode) or uint8 [h, w, 3] arrays (copied as pixels: streams
    the device path does not support, records that are not JPEGs). sources: a uint8 device tensor; image i lands at byte
    offsets[i], a multiple of 16. Coefficients, descriptors and fallback pixels go through ONE pinned staging buffer and ONE
    host-to-device copy on `stream`; staging and device buffers grow to the largest batch seen. A decoder is bound to one
    consumer: the next `decode` waits for the previous one's copy before it reuses the staging."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if _lib.lib().mpn_jpeg_desc_bytes() != DESC_BYTES:
            raise _lib.MpnError("mpn_jpeg_decode: the descriptor's layout is not the one this binding was written against")
        self._stage = self._dev = self._work = None
        self._done = None

    def _ensure(self, stage_bytes, work_bytes):
        import torch
        grow_stage = self._stage is None or self._stage.numel() < stage_bytes
        grow_work = self._work is None or self._work.numel() < work_bytes
        if (grow_stage and self._stage is not None) or (grow_work and self._work is not None):
            torch.cuda.synchronize(self.device)     # (rare) growth: no queued copy or launch still uses the old buffers
        if grow_stage:
            n = _capacity(stage_bytes)
            self._stage = torch.empty(n, dtype=torch.uint8).pin_memory()
            self._dev = torch.empty(n, dtype=torch.uint8, device=self.device)
        if grow_work:
            self._work = torch.empty(_capacity(work_bytes), dtype=torch.uint8, device=self.device)

    @staticmethod
    def plan(entries, offsets):
        """Host arithmetic of one batch: (jpeg indices, pixel indices, staging layout). The staging holds the descriptors of
        the JPEG entries, their coefficients, then the pixels of the other entries, each part 16-byte aligned."""
        jp = [i for i, e in enumerate(entries) if isinstance(e, Coefficients)]
        px = [i for i, e in enumerate(entries) if not isinstance(e, Coefficients)]
        for i in px:
            e = entries[i]
            if not isinstance(e, np.ndarray) or e.dtype != np.uint8 or e.ndim != 3 or e.shape[2] != 3:
                raise ValueError("a batch entry must be Coefficients or a uint8 [height, width, 3] array")
        for i in jp:
            if offsets[i] % 16:
                raise ValueError(f"the offset of a device-decoded image must be a multiple of 16 (got {offsets[i]})")
        at = len(jp) * DESC_BYTES
        coef_at, work_at = [], []
        coef_base, work = at, 0
        for i in jp:
            coef_at.append(at - coef_base)
            work_at.append(work)
            at += entries[i].coefs.nbytes                    # (128 per block: stays 16-byte aligned)
            work += entries[i].coefs.shape[0] * 64
        coef_bytes = at - coef_base
        pix_at = []
        for i in px:
            pix_at.append(at)
            at += _round16(entries[i].size)
        return jp, px, {'coef_base': coef_base, 'coef_bytes': coef_bytes, 'coef_at': coef_at, 'work_at': work_at,
                        'work_bytes': work, 'pix_at': pix_at, 'stage_bytes': at}

    def decode(self, entries, sources, offsets, stream=None):
        import torch
        if len(entries) != len(offsets) or not len(entries):
            raise ValueError("decode: one offset per entry, at least one entry")
        if sources.dtype != torch.uint8 or not sources.is_contiguous() or sources.device != self.device:
            raise ValueError("decode: sources must be a contiguous uint8 tensor on the decoder's device")
        total = sources.numel()
        for e, off in zip(entries, offsets):
            shape = e.shape
            if off < 0 or off + shape[0] * shape[1] * 3 > total:
                raise ValueError(f"decode: an image of {shape} at byte {off} does not fit a buffer of {total} bytes")
        jp, px, lay = self.plan(entries, offsets)
        if self._done is not None:
            self._done.synchronize()                            # the previous batch's copy has left the staging
        self._ensure(lay['stage_bytes'], max(lay['work_bytes'], 64))
        stage = self._stage.numpy()
        if jp:
            descs = stage[:len(jp) * DESC_BYTES].view(DESC)
            for k, i in enumerate(jp):
                e = entries[i]
                descs[k] = e.desc[0]
                descs[k]['src_offset'], descs[k]['coef_offset'], descs[k]['work_offset'] = offsets[i], lay['coef_at'][k], lay['work_at'][k]
                at = lay['coef_base'] + lay['coef_at'][k]
                stage[at:at + e.coefs.nbytes] = e.coefs.reshape(-1).view(np.uint8)
        for k, i in enumerate(px):
            e = entries[i]
            stage[lay['pix_at'][k]:lay['pix_at'][k] + e.size] = e.reshape(-1)
        stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        n = lay['stage_bytes']
        with torch.cuda.stream(stream):
            self._dev[:n].copy_(self._stage[:n], non_blocking=True)
            if jp:
                base = self._dev.data_ptr()
                _lib.call("mpn_jpeg_decode", ctypes.c_void_p(base + lay['coef_base']), lay['coef_bytes'], ctypes.c_void_p(base),
                          len(jp), _lib.ptr(sources), total, _lib.ptr(self._work), self._work.numel(),
                          ctypes.c_void_p(stream.cuda_stream))
            for k, i in enumerate(px):
                at, size = lay['pix_at'][k], entries[i].size
                sources[offsets[i]:offsets[i] + size].copy_(self._dev[at:at + size], non_blocking=True)
            self._done = torch.cuda.Event()
            self._done.record(stream)
