"""JPEG decode split between host and device (include/mpn.h, "JPEG decode"): `jpeg_info` and `entropy_decode` are the host
stage (marker scan and Huffman decode in C++, the GIL released: a thread pool runs them in parallel), `JpegBatchDecoder` ships
the coefficients of a batch and launches `mpn_jpeg_decode`, which writes uint8 RGB into a packed source buffer - the bytes Pillow
returns for the same file. Progressive files and Adobe CMYK files take a second host stage, `scans_decode` (every scan of the
file -> the same coefficients; four planes for CMYK, which the device converts as Pillow does); `jpeg_support` says which route
a file takes. Streams outside both sets (YCCK, arithmetic coding, 12 bits, ...) are decoded by Pillow per image and copied as
pixels, inside the same batch.

JPEG encode is the second half of the file: `quality_tables`, `jpeg_headers`, `JpegBatchEncoder`, `encode_jpegs`."""
import ctypes
import io

import numpy as np

from .. import _lib
from ..model_state import resolve_device
from .resample import _round16, capacity_for

DESC_BYTES = 512                        # MPN_JPEG_DESC_BYTES (checked against the library)
REASONS = ('supported', 'malformed', 'progressive', 'arithmetic', 'frame_type', 'precision', 'components', 'colorspace',
           'sampling', 'multiscan', 'dqt16', 'too_large')


class _Header(ctypes.Structure):        # mpn_jpeg_header
    _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32), ('components', ctypes.c_int32),
                ('h_samp', ctypes.c_int32), ('v_samp', ctypes.c_int32), ('restart_interval', ctypes.c_int32),
                ('supported', ctypes.c_int32), ('reason', ctypes.c_int32),
                ('blocks_w', ctypes.c_int32 * 3), ('blocks_h', ctypes.c_int32 * 3),
                ('total_blocks', ctypes.c_int32), ('reserved', ctypes.c_int32), ('coef_bytes', ctypes.c_int64)]
    INFO = "mpn_jpeg_info"
    decodes = property(lambda h: bool(h.supported))     # mpn_jpeg_entropy_decode takes the stream


class _ScansHeader(ctypes.Structure):   # mpn_jpeg_scans_header
    _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32), ('components', ctypes.c_int32),
                ('h_samp', ctypes.c_int32), ('v_samp', ctypes.c_int32), ('progressive', ctypes.c_int32),
                ('route', ctypes.c_int32), ('reason', ctypes.c_int32),
                ('blocks_w', ctypes.c_int32 * 4), ('blocks_h', ctypes.c_int32 * 4),
                ('total_blocks', ctypes.c_int32), ('reserved', ctypes.c_int32), ('coef_bytes', ctypes.c_int64)]
    INFO = "mpn_jpeg_scans_info"
    decodes = property(lambda h: h.route != 2)          # mpn_jpeg_scans_decode takes the stream


ROUTES = ('device', 'host-entropy', 'pillow')       # MPN_JPEG_ROUTE_*

# mpn_jpeg_desc as a numpy record (its three offsets are the caller's). With four components the fourth's grid is
# (blocks_h3, blocks_w3) and its quantisation table is quant[quant3]
DESC = np.dtype([('src_offset', np.int64), ('coef_offset', np.int64), ('work_offset', np.int64),
                 ('width', np.int32), ('height', np.int32), ('components', np.int32), ('h_samp', np.int32), ('v_samp', np.int32),
                 ('total_blocks', np.int32), ('blocks_w', np.int32, (3,)), ('blocks_h', np.int32, (3,)),
                 ('blocks_w3', np.int32), ('blocks_h3', np.int32), ('quant3', np.int32),
                 ('reserved', np.int32, (11,)), ('quant', np.uint16, (3, 64))])
assert DESC.itemsize == DESC_BYTES


# mpn_jpeg_scan_desc: what the device's entropy stage reads (its four offsets are the caller's)
SCAN_DESC_BYTES = 2704                  # MPN_JPEG_SCAN_DESC_BYTES (checked against the library)
ENTROPY_RECORD_BYTES = 16
ENT_OK, ENT_NOT_CONVERGED, ENT_BAD_DATA, ENT_SKIPPED = 0, 1, 2, 3
ENTROPY_MODES = ('host', 'device')
MAX_PASSES = 4                          # launches that carry a 32 KB group's exit into the next group (mpn.h)
SCAN_DESC = np.dtype([('file_offset', np.int64), ('coef_offset', np.int64), ('src_offset', np.int64), ('work_offset', np.int64),
                      ('nbytes', np.int64), ('scan_offset', np.int64),
                      ('width', np.int32), ('height', np.int32), ('components', np.int32), ('h_samp', np.int32), ('v_samp', np.int32),
                      ('restart_interval', np.int32), ('total_blocks', np.int32), ('blocks_w', np.int32, (3,)),
                      ('blocks_h', np.int32, (3,)), ('dc_table', np.int32, (3,)), ('ac_table', np.int32, (3,)),
                      ('supported', np.int32), ('reason', np.int32), ('reserved', np.int32, (3,)),
                      ('quant', np.uint16, (3, 64)), ('huff_bits', np.uint8, (2, 4, 16)), ('huff_vals', np.uint8, (2, 4, 256))])
ENTROPY_RECORD = np.dtype([('status', np.int32), ('passes', np.int32), ('blocks', np.int32), ('reserved', np.int32)])
assert SCAN_DESC.itemsize == SCAN_DESC_BYTES and ENTROPY_RECORD.itemsize == ENTROPY_RECORD_BYTES


def check_entropy_mode(entropy):
    if entropy not in ENTROPY_MODES:
        raise ValueError(f"entropy must be one of {ENTROPY_MODES} (got {entropy!r})")
    return entropy


def _as_bytes(data):
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError("a JPEG must be bytes")
    return bytes(data)


def _header(h, data):
    """The info call of the header struct `h` into it; damaged headers raise ValueError."""
    _lib.check(getattr(_lib.lib(), h.INFO)(data, len(data), ctypes.byref(h)))
    return h


def _header_dict(h, **own):
    """What both header structs hold, and the fields `own` of one of them."""
    return {'width': h.width, 'height': h.height, 'components': h.components, 'sampling': (h.h_samp, h.v_samp), **own,
            'reason': REASONS[h.reason],
            'blocks': [(h.blocks_h[c], h.blocks_w[c]) for c in range(min(h.components, len(h.blocks_w)))] if h.decodes else [],
            'total_blocks': h.total_blocks, 'coef_bytes': h.coef_bytes}


def jpeg_info(data):
    """The header of a JPEG as a dict: 'width', 'height', 'components', 'sampling' (h, v) of the first component,
    'restart_interval', 'supported' (bool), 'reason' (one of REASONS), 'blocks' [(blocks_h, blocks_w)] per component,
    'total_blocks', 'coef_bytes'. A stream whose headers are damaged raises ValueError."""
    h = _header(_Header(), _as_bytes(data))
    return _header_dict(h, restart_interval=h.restart_interval, supported=bool(h.supported))


class Coefficients:
    """A JPEG after a host stage: `.shape` (h, w, 3) of the image it decodes to, `.coefs` int16 [total_blocks, 64] (raw
    coefficients, natural order, one plane of blocks per component: 1, 3 or - CMYK - 4) and `.desc`, a one-element DESC record."""
    __slots__ = ('shape', 'coefs', 'desc')

    def __init__(self, shape, coefs, desc):
        self.shape, self.coefs, self.desc = shape, coefs, desc

    def planes(self):
        """[(coefficients [blocks_h, blocks_w, 8, 8], quantisation table [8, 8])] per component."""
        d, out, at = self.desc[0], [], 0
        for c in range(int(d['components'])):
            bh, bw = (int(d['blocks_h'][c]), int(d['blocks_w'][c])) if c < 3 else (int(d['blocks_h3']), int(d['blocks_w3']))
            out.append((self.coefs[at:at + bh * bw].reshape(bh, bw, 8, 8), d['quant'][c if c < 3 else int(d['quant3'])].reshape(8, 8)))
            at += bh * bw
        return out


def _host_stage(name, h, data):
    """The info call of `h`, then mpn_jpeg_<name> into a buffer of the size the header reports -> Coefficients."""
    data = _as_bytes(data)
    _header(h, data)
    if not h.decodes:
        raise ValueError(f"{name}: stream not supported ({REASONS[h.reason]})")
    coefs = np.empty((h.total_blocks, 64), np.int16)
    desc = np.zeros(1, DESC)
    _lib.check(getattr(_lib.lib(), "mpn_jpeg_" + name)(data, len(data), coefs.ctypes.data_as(ctypes.c_void_p), coefs.nbytes,
                                                       desc.ctypes.data_as(ctypes.c_void_p)))
    return Coefficients((h.height, h.width, 3), coefs, desc)


def entropy_decode(data):
    """The host stage on one SUPPORTED JPEG -> Coefficients. Raises ValueError for a stream that is damaged, truncated or
    outside the supported set (`jpeg_info(data)['supported']`)."""
    return _host_stage("entropy_decode", _Header(), data)


def scans_info(data):
    """The header of a JPEG as the multi-scan host stage sees it: 'width', 'height', 'components', 'sampling', 'progressive'
    (bool), 'route' (one of ROUTES), 'reason' (one of REASONS: why the route is 'pillow', else 'supported'), 'blocks'
    [(blocks_h, blocks_w)] of up to four components, 'total_blocks', 'coef_bytes'. Damaged headers raise ValueError."""
    h = _header(_ScansHeader(), _as_bytes(data))
    return _header_dict(h, progressive=bool(h.progressive), route=ROUTES[h.route])


def jpeg_support(data):
    """The route a JPEG takes through `prepare(..., extended=True)`: 'device' (baseline gray / YCbCr: one scan, whose Huffman
    stage may run on the host or on the device), 'host-entropy' (progressive, Adobe CMYK: every scan decoded on the host by
    `scans_decode`, the rest on the device) or 'pillow' (decoded by Pillow, copied as pixels). Damaged headers raise ValueError."""
    return scans_info(data)['route']


def scans_decode(data):
    """The multi-scan host stage on one JPEG whose route is 'host-entropy' or 'device' -> Coefficients (four planes for CMYK).
    Raises ValueError for a file that is damaged, truncated, incomplete or on the 'pillow' route."""
    return _host_stage("scans_decode", _ScansHeader(), data)


class Scan:
    """A SUPPORTED JPEG whose Huffman stage is left to the device: `.data` (the file's bytes), `.shape` (h, w, 3) and `.desc`,
    a one-element SCAN_DESC record (headers only; the scan's bytes were not touched)."""
    __slots__ = ('data', 'shape', 'desc')

    def __init__(self, data, shape, desc):
        self.data, self.shape, self.desc = data, shape, desc

    @property
    def total_blocks(self):
        return int(self.desc[0]['total_blocks'])


def _scan(data):
    """mpn_jpeg_scan_prepare -> (return code, reason, the Scan of a SUPPORTED stream or None)."""
    desc = np.zeros(1, SCAN_DESC)
    rc = _lib.lib().mpn_jpeg_scan_prepare(data, len(data), desc.ctypes.data_as(ctypes.c_void_p))
    d = desc[0]
    return rc, REASONS[int(d['reason'])], Scan(data, (int(d['height']), int(d['width']), 3), desc) if rc == 0 and d['supported'] else None


def scan_prepare(data):
    """The header stage on one SUPPORTED JPEG -> Scan. Raises ValueError for a stream whose headers are damaged or that is
    outside the supported set."""
    rc, reason, scan = _scan(_as_bytes(data))
    _lib.check(rc)
    if scan is None:
        raise ValueError(f"scan_prepare: stream not supported ({reason})")
    return scan


def pillow_decode(data):
    """What the device path must equal, and the per-image fallback: Pillow's decode to uint8 [h, w, 3]."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _extended(data):
    """Coefficients of a file on the 'host-entropy' route, else Pillow's pixels (which raises for a damaged file)."""
    h = _ScansHeader()
    if _lib.lib().mpn_jpeg_scans_info(data, len(data), ctypes.byref(h)) == 0 and h.route == 1:
        try:
            return scans_decode(data)
        except ValueError:
            pass                # damaged, or a script the stage refuses: the library decides what the file is worth
    return pillow_decode(data)


def prepare(item, entropy='host', extended=False):
    """One entry of a batch, ready for `JpegBatchDecoder`: JPEG bytes -> Coefficients when the stream is supported (a Scan
    with entropy='device': headers only, the Huffman stage runs on the device), else the pixels Pillow decodes; a uint8
    [h, w, 3] array, a Coefficients or a Scan passes through. extended=True (what the pipelines and `Detector.predict_jpegs`
    pass) also returns Coefficients for progressive and Adobe CMYK files (`jpeg_support(data) == 'host-entropy'`): their
    scans are decoded here, on the host, with either `entropy` - a file of several scans has no single scan to hand to the
    device. The default keeps Pillow's pixels for them. Thread-safe (the pipelines' decode pool)."""
    check_entropy_mode(entropy)
    if isinstance(item, (Coefficients, Scan, np.ndarray)):
        return item
    data = _as_bytes(item)
    if entropy == 'device':
        entry = _scan(data)[2]
    else:
        h = _Header()
        entry = entropy_decode(data) if _lib.lib().mpn_jpeg_info(data, len(data), ctypes.byref(h)) == 0 and h.supported else None
    if entry is not None:
        return entry
    return _extended(data) if extended else pillow_decode(data)


def _capacity(n):
    return capacity_for(max(n, 16))


class JpegBatchDecoder:
    """Fills a packed uint8 source buffer on the device from a batch of prepared entries.

        decoder = JpegBatchDecoder(device)
        decoder.decode(entries, sources, offsets, stream)

    entries: Coefficients (decoded on the device by mpn_jpeg_decode), Scan (Huffman-decoded on the device first, by
    mpn_jpeg_entropy_decode_device: the file's bytes and a header descriptor are staged instead of coefficients; the [B]
    records come back with one small copy and one event wait, and every image that is not OK takes the host `entropy_decode` -
    which raises ValueError for a damaged stream - and a second mpn_jpeg_decode; `.fallbacks` counts them) or uint8 [h, w, 3]
    arrays (copied as pixels: streams the device path does not support, records that are not JPEGs). A Coefficients entry may
    hold one, three or four planes (CMYK), in any mix. `.staged_bytes`: what
    the last `decode` uploaded. sources: a uint8 device tensor; image i lands at byte
    offsets[i], a multiple of 16. Coefficients, descriptors and fallback pixels go through ONE pinned staging buffer and ONE
    host-to-device copy on `stream`; staging and device buffers grow to the largest batch seen. A decoder is bound to one
    consumer: the next `decode` waits for the previous one's copy before it reuses the staging."""

    def __init__(self, device, max_passes=MAX_PASSES):
        self.device = resolve_device(device)
        if _lib.lib().mpn_jpeg_desc_bytes() != DESC_BYTES or _lib.lib().mpn_jpeg_scan_desc_bytes() != SCAN_DESC_BYTES:
            raise _lib.MpnError("mpn_jpeg_decode: the descriptor's layout is not the one this binding was written against")
        self.max_passes = int(max_passes)
        self.fallbacks = 0                  # Scan entries of the last `decode` that took the host entropy stage
        self.staged_bytes = 0               # bytes the last `decode` uploaded
        self.records = None                 # ENTROPY_RECORD per Scan entry of the last `decode`
        self._buf = {}                      # grow-only buffers, by name
        self.scan_layout = None
        self._done = None

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

    def _buffer(self, name, nbytes, pinned=False):
        """A uint8 buffer of at least nbytes that grows to the largest batch seen."""
        import torch
        have = self._buf.get(name)
        if have is None or have.numel() < nbytes:
            if have is not None:
                torch.cuda.synchronize(self.device)             # (rare) growth: no queued copy or launch still uses the old buffer
            n = _capacity(nbytes)
            have = torch.empty(n, dtype=torch.uint8).pin_memory() if pinned else torch.empty(n, dtype=torch.uint8, device=self.device)
            self._buf[name] = have
        return have

    def _staging(self, name, nbytes):
        """The pinned staging buffer `name`, free to be written: the previous batch's copy has left it."""
        if self._done is not None:
            self._done.synchronize()
        return self._buffer(name, nbytes, pinned=True)

    def _ship(self, stage, dev, n, kind, items, decode_args, sources, stream, entropy=False):
        """Writes `items` - (descriptor record of dtype `kind`, the caller's offsets {field: value}, payload as uint8, its
        position) - into the staging, queues the copy of its first n bytes to `dev` and behind it (the device's entropy stage
        and) mpn_jpeg_decode over the items: decode_args = (coefs, coef_bytes, descs, work buffer)."""
        import torch
        host = stage.numpy()
        descs = host[:len(items) * kind.itemsize].view(kind)
        for k, (record, own, payload, at) in enumerate(items):
            descs[k] = record
            for field, value in own.items():
                descs[k][field] = value
            host[at:at + payload.size] = payload
        with torch.cuda.stream(stream):
            dev[:n].copy_(stage[:n], non_blocking=True)
            if entropy:
                self.entropy_launch(stream)
            if items:
                coefs, coef_bytes, dev_descs, work = decode_args
                _lib.call("mpn_jpeg_decode", coefs, coef_bytes, dev_descs, len(items), _lib.ptr(sources), sources.numel(),
                          _lib.ptr(work), work.numel(), ctypes.c_void_p(stream.cuda_stream))

    @staticmethod
    def plan_scans(scans, offsets, file_order=None):
        """Host arithmetic of the Scan entries of a batch: the staging holds their descriptors, then their files, each at a
        multiple of 16; coefficients and inverse-DCT planes follow each other on the device. file_order: the order in which
        the files lie in the staging (a permutation of the entries' indices; default: the entries' own order) - the device
        call does not care."""
        order = list(range(len(scans))) if file_order is None else [int(k) for k in file_order]
        if sorted(order) != list(range(len(scans))):
            raise ValueError("file_order must be a permutation of the entries' indices")
        at = len(scans) * SCAN_DESC_BYTES
        file_base = at
        file_at = [0] * len(scans)
        for k in order:
            file_at[k] = at - file_base
            at += _round16(len(scans[k].data))
        coef_at, work_at, coef, work = [], [], 0, 0
        for e, off in zip(scans, offsets):
            if off % 16:
                raise ValueError(f"the offset of a device-decoded image must be a multiple of 16 (got {off})")
            coef_at.append(coef)
            work_at.append(work)
            coef += e.total_blocks * 128
            work += e.total_blocks * 64
        return {'file_base': file_base, 'files_bytes': at - file_base, 'file_at': file_at, 'coef_at': coef_at, 'work_at': work_at,
                'coef_bytes': coef, 'work_bytes': work, 'stage_bytes': at}

    def entropy_launch(self, stream=None):
        """mpn_jpeg_entropy_decode_device over the Scan entries `decode_scans` staged last, on `stream` (default: the current
        one). No host synchronisation: what `decode_scans` queues, and what a benchmark times."""
        lay, buf = self.scan_layout, self._buf
        base = buf['scan_dev'].data_ptr()
        st = _lib.stream_ptr() if stream is None else ctypes.c_void_p(stream.cuda_stream)
        _lib.call("mpn_jpeg_entropy_decode_device", ctypes.c_void_p(base + lay['file_base']), lay['files_bytes'], ctypes.c_void_p(base),
                  len(lay['file_at']), _lib.ptr(buf['scan_coefs']), buf['scan_coefs'].numel(), _lib.ptr(buf['scan_descs']),
                  _lib.ptr(buf['records']), _lib.ptr(buf['entropy_work']), buf['entropy_work'].numel(), self.max_passes, st)

    def decode_scans(self, scans, sources, offsets, stream, file_order=None):
        """Entropy stage and inverse DCT of the Scan entries on the device, then the wait for their records (`.records`);
        returns the indices (into `scans`) of the images whose record is not OK. `decode` calls this and handles them.
        mpn_jpeg_decode runs over every image of the batch, so until the fallback has run (or when it raises) the pixels
        of an image that is not OK are undefined inside its own [offset, offset + h * w * 3) of `sources`."""
        import torch
        lay = self.scan_layout = self.plan_scans(scans, offsets, file_order)
        b, n = len(scans), lay['stage_bytes']
        ent_work = _lib.lib().mpn_jpeg_entropy_decode_device_workspace_bytes(b, lay['files_bytes'])
        if ent_work == 0:
            raise ValueError(f"decode: a batch of {b} files in {lay['files_bytes']} bytes is outside what mpn_jpeg_entropy_decode_device takes")
        stage, dev = self._staging('scan_stage', n), self._buffer('scan_dev', n)
        coefs, planes = self._buffer('scan_coefs', lay['coef_bytes']), self._buffer('scan_planes', max(lay['work_bytes'], 64))
        descs_out, records = self._buffer('scan_descs', b * DESC_BYTES), self._buffer('records', b * ENTROPY_RECORD_BYTES)
        record_host = self._buffer('record_host', b * ENTROPY_RECORD_BYTES, pinned=True)
        self._buffer('entropy_work', ent_work)
        items = [(e.desc[0], {'file_offset': lay['file_at'][k], 'coef_offset': lay['coef_at'][k], 'src_offset': off, 'work_offset': lay['work_at'][k]},
                  np.frombuffer(e.data, np.uint8), lay['file_base'] + lay['file_at'][k]) for k, (e, off) in enumerate(zip(scans, offsets))]
        self._ship(stage, dev, n, SCAN_DESC, items, (_lib.ptr(coefs), coefs.numel(), _lib.ptr(descs_out), planes), sources, stream, entropy=True)
        with torch.cuda.stream(stream):
            record_host[:b * ENTROPY_RECORD_BYTES].copy_(records[:b * ENTROPY_RECORD_BYTES], non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
        done.synchronize()
        self.records = record_host.numpy()[:b * ENTROPY_RECORD_BYTES].view(ENTROPY_RECORD).copy()
        self.staged_bytes += n
        skipped = [k for k in range(b) if self.records[k]['status'] == ENT_SKIPPED]
        if skipped:
            raise _lib.MpnError(f"mpn_jpeg_entropy_decode_device skipped image {skipped[0]}: its descriptor is out of range")
        return [k for k in range(b) if self.records[k]['status'] != ENT_OK]

    def scan_coefficients(self, k):
        """The device's coefficients of Scan entry k of the last batch, int16 [total_blocks, 64] on the host (tests, tools)."""
        lay = self.scan_layout
        end = lay['coef_at'][k + 1] if k + 1 < len(lay['coef_at']) else lay['coef_bytes']
        return self._buf['scan_coefs'][lay['coef_at'][k]:end].cpu().numpy().view(np.int16).reshape(-1, 64)

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
        self.fallbacks = self.staged_bytes = 0
        self.records = None
        stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        sc = [i for i, e in enumerate(entries) if isinstance(e, Scan)]
        if sc:
            bad = self.decode_scans([entries[i] for i in sc], sources, [offsets[i] for i in sc], stream)
            self.fallbacks = len(bad)
            redo = {sc[k]: entropy_decode(entries[sc[k]].data) for k in bad}     # (raises ValueError for a damaged stream)
            keep = [i for i, e in enumerate(entries) if not isinstance(e, Scan) or i in redo]
            if not keep:
                return
            entries, offsets = [redo.get(i, entries[i]) for i in keep], [offsets[i] for i in keep]
        jp, px, lay = self.plan(entries, offsets)
        n = lay['stage_bytes']
        stage, dev, work = self._staging('stage', n), self._buffer('dev', n), self._buffer('work', max(lay['work_bytes'], 64))
        for k, i in enumerate(px):
            stage.numpy()[lay['pix_at'][k]:lay['pix_at'][k] + entries[i].size] = entries[i].reshape(-1)
        items = [(entries[i].desc[0], {'src_offset': offsets[i], 'coef_offset': lay['coef_at'][k], 'work_offset': lay['work_at'][k]},
                  entries[i].coefs.reshape(-1).view(np.uint8), lay['coef_base'] + lay['coef_at'][k]) for k, i in enumerate(jp)]
        self.staged_bytes += n
        base = dev.data_ptr()
        self._ship(stage, dev, n, DESC, items, (ctypes.c_void_p(base + lay['coef_base']), lay['coef_bytes'], ctypes.c_void_p(base), work),
                   sources, stream)
        with torch.cuda.stream(stream):
            for k, i in enumerate(px):
                at, size = lay['pix_at'][k], entries[i].size
                sources[offsets[i]:offsets[i] + size].copy_(dev[at:at + size], non_blocking=True)
            self._done = torch.cuda.Event()
            self._done.record(stream)


# ------------------------------------------------------------------------------------------------ encode
# All of it on the device (include/mpn.h, "JPEG encode"): `mpn_jpeg_forward` turns packed RGB / RGBA frames into quantised
# coefficients, `mpn_jpeg_entropy_encode` into the finished scan; the host adds the headers, which depend on nothing but the
# geometry and the tables. The files equal Pillow's `save(buf, "JPEG", quality=q, subsampling=s)` byte for byte.

ENC_DESC_BYTES = 512                    # MPN_JPEG_ENC_DESC_BYTES (checked against the library)
RECORD_BYTES = 32                       # mpn_jpeg_stream_record
ENC_OK, ENC_NO_FIT, ENC_NO_FIT_RAW, ENC_SKIPPED = 0, 1, 2, 3
SAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}
BYTES_PER_SAMPLE = 2                    # an image's capacity: blocks * 64 * this + 256 (a stream beyond it takes the fallback)

ENC_DESC = np.dtype([('src_offset', np.int64), ('coef_offset', np.int64), ('out_offset', np.int64), ('capacity', np.int64),
                     ('work_offset', np.int64), ('width', np.int32), ('height', np.int32), ('channels', np.int32),
                     ('h_samp', np.int32), ('v_samp', np.int32), ('reserved', np.int32, (17,)), ('quant', np.uint16, (3, 64))])
RECORD = np.dtype([('offset', np.int64), ('size', np.int64), ('status', np.int32), ('reserved', np.int32, (3,))])
assert ENC_DESC.itemsize == ENC_DESC_BYTES and RECORD.itemsize == RECORD_BYTES

# Annex K.1 / K.2 (natural order) and K.3 - K.6 as Pillow's DHT segments hold them: (class, id, 16 counts, symbols)
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
              80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
              95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                99, 99, 99) + (99,) * 32
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
           42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_DHT = tuple(bytes.fromhex(s) for s in (
    "00" "00010501010101010100000000000000" "000102030405060708090a0b",
    "10" "0002010303020403050504040000017d" "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a"
    "25262728292a3435363738393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999a"
    "a2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa",
    "01" "00030101010101010101010000000000" "000102030405060708090a0b",
    "11" "00020102040403040705040400010277" "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f1"
    "1718191a262728292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a9293949596"
    "9798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def quality_tables(quality):
    """The two 8-bit quantisation tables (luma, chroma; uint16 [64], natural order) libjpeg derives from the Annex K tables
    for `quality` in 1..100: scale = 5000 / q below 50, else 200 - 2q; entry = (base * scale + 50) / 100 clamped to 1..255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be in 1..100 (got {quality})")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(base, np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16) for base in (_BASE_LUMA, _BASE_CHROMA))


def _sampling(subsampling):
    try:
        return SAMPLING[subsampling]
    except (KeyError, TypeError):
        raise ValueError(f"subsampling must be one of {sorted(SAMPLING)} (got {subsampling!r})")


def _segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, 'big') + payload


def jpeg_headers(width, height, sampling, tables):
    """The bytes from SOI through the SOS header as Pillow writes them for an RGB image with no extra `info`: APP0 (JFIF 1.1,
    no density), two DQT, SOF0, four DHT (the standard tables), SOS. sampling: '4:4:4', '4:2:2' or '4:2:0'; tables: the two
    8-bit tables of `quality_tables` (natural order)."""
    hs, vs = _sampling(sampling)
    if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
        raise ValueError(f"a JPEG is 1..65535 pixels per side (got {height} x {width})")
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate(tables):
        t = np.asarray(t).reshape(64)
        out += _segment(0xDB, bytes((i,)) + bytes(int(t[n]) for n in _ZIGZAG))
    out += _segment(0xC0, b"\x08" + int(height).to_bytes(2, 'big') + int(width).to_bytes(2, 'big') + b"\x03"
                    + bytes((1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for table in _DHT:
        out += _segment(0xC4, table)
    return out + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def pillow_encode(pixels, quality=75, subsampling='4:2:0'):
    """What the device path must equal, and the per-image fallback: Pillow's file for a uint8 [h, w, 3 or 4] array."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(pixels[..., :3])).save(buf, "JPEG", quality=int(quality),
                                                                subsampling={'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}[subsampling])
    return buf.getvalue()


def total_blocks(height, width, sampling):
    hs, vs = _sampling(sampling)
    return -(-int(width) // (8 * hs)) * -(-int(height) // (8 * vs)) * (hs * vs + 2)


class EncodePlan:
    """Host arithmetic of one batch: `.descs` (ENC_DESC [b]), where every image's coefficients, scan and workspace lie (each
    at a multiple of 16), the three buffer sizes `.need` = (coef_bytes, out_bytes, work_bytes), and the headers."""

    def __init__(self, shapes, offsets, channels, quality=75, subsampling='4:2:0', capacities=None):
        hs, vs = _sampling(subsampling)
        tables = quality_tables(quality)
        if len(shapes) != len(offsets) or not len(shapes):
            raise ValueError("encode: one offset per image, at least one image")
        if channels not in (3, 4):
            raise ValueError(f"encode: channels must be 3 (RGB) or 4 (RGBA) (got {channels})")
        lib = _lib.lib()
        b = len(shapes)
        self.quality, self.subsampling, self.channels = int(quality), subsampling, channels
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        self.offsets = [int(o) for o in offsets]
        self.descs = np.zeros(b, ENC_DESC)
        self.headers = []
        coef = out = work = 0
        for i, ((h, w), off) in enumerate(zip(self.shapes, self.offsets)):
            if off % 16:
                raise ValueError(f"encode: the offset of an image must be a multiple of 16 (got {off})")
            blocks = total_blocks(h, w, subsampling)
            cap = _round16(blocks * 64 * BYTES_PER_SAMPLE + 256) if capacities is None else int(capacities[i])
            share = lib.mpn_jpeg_entropy_encode_workspace_bytes(blocks, cap)
            if share == 0:
                raise ValueError(f"encode: an image of {h} x {w} with a capacity of {cap} bytes is outside what mpn_jpeg_entropy_encode takes")
            d = self.descs[i]
            d['src_offset'], d['coef_offset'], d['out_offset'], d['capacity'], d['work_offset'] = off, coef, out, cap, work
            d['width'], d['height'], d['channels'], d['h_samp'], d['v_samp'] = w, h, channels, hs, vs
            d['quant'][0], d['quant'][1], d['quant'][2] = tables[0], tables[1], tables[1]
            self.headers.append(jpeg_headers(w, h, subsampling, tables))
            coef += blocks * 128
            out += _round16(cap)
            work += _round16(share)
        self.need = (coef, out, work)


class JpegBatchEncoder:
    """Encodes a batch of frames that lie in a packed uint8 buffer on the device.

        encoder = JpegBatchEncoder(device)
        files = encoder.encode(sources, offsets, shapes, channels, quality=75, subsampling='4:2:0')

    sources: a uint8 device tensor; image i is [h_i, w_i, channels] at byte offsets[i], a multiple of 16; channels 3 (RGB) or
    4 (RGBA as mpn_draw_detections writes it; alpha is ignored). One descriptor upload, the two device calls, one small copy
    of the records, then one copy per image of exactly the bytes its stream used, packed into one pinned buffer behind a
    single synchronise; buffers grow to the largest batch seen. An image whose stream does not fit
    its capacity (blocks * 64 * BYTES_PER_SAMPLE + 256 bytes) is fetched as pixels and encoded by Pillow: the same bytes.
    The steps are also there one by one (`reserve`, `upload`, `launch`, `collect`) for a caller that captures `launch` in a
    graph: the Detector."""

    def __init__(self, device):
        self.device = resolve_device(device)
        if _lib.lib().mpn_jpeg_enc_desc_bytes() != ENC_DESC_BYTES:
            raise _lib.MpnError("mpn_jpeg_forward: the descriptor's layout is not the one this binding was written against")
        self.b = self.n = 0                                     # descriptors allocated; images of the batch in place
        self.capacity = (0, 0, 0)
        self.fallbacks = 0                                      # images the last `collect` left to Pillow
        self.copied_bytes = 0                                   # bytes its record and stream copies brought to the host
        self._coefs = self._out = self._work = self._descs = self._desc_stage = self._records = self._record_host = None
        self._out_host = None

    def reserve(self, b, coef_bytes, out_bytes, work_bytes):
        """Buffers for batches of up to b images within the three sizes; True when anything was (re)allocated."""
        import torch
        need = (coef_bytes, out_bytes, work_bytes)
        grow = any(n > c for n, c in zip(need, self.capacity))
        if not grow and b <= self.b:
            return False
        if self._coefs is not None:
            torch.cuda.synchronize(self.device)                 # (rare) growth: no queued launch still uses the old buffers
        dev = self.device
        if grow:
            self.capacity = tuple(max(_capacity(n), c) for n, c in zip(need, self.capacity))
            self._coefs = torch.empty(self.capacity[0], dtype=torch.uint8, device=dev)
            self._out = torch.empty(self.capacity[1], dtype=torch.uint8, device=dev)
            self._work = torch.empty(self.capacity[2], dtype=torch.uint8, device=dev)
            self._out_host = torch.empty(self.capacity[1], dtype=torch.uint8).pin_memory()
        if b > self.b:
            self.b = b
            self._desc_stage = torch.zeros(b * ENC_DESC_BYTES, dtype=torch.uint8).pin_memory()
            self._descs = torch.zeros(b * ENC_DESC_BYTES, dtype=torch.uint8, device=dev)
            self._records = torch.zeros(b * RECORD_BYTES, dtype=torch.uint8, device=dev)
            self._record_host = torch.zeros(b * RECORD_BYTES, dtype=torch.uint8).pin_memory()
        return True

    def upload(self, plan):
        """This call's descriptors to the device: one small copy on the current stream, ordered before the launch."""
        n = len(plan.descs)
        if n > self.b or any(need > c for need, c in zip(plan.need, self.capacity)):
            raise ValueError("encode: the batch exceeds the reserved buffers")
        self.n = n
        self._desc_stage.numpy()[:n * ENC_DESC_BYTES] = plan.descs.view(np.uint8)
        self._descs[:n * ENC_DESC_BYTES].copy_(self._desc_stage[:n * ENC_DESC_BYTES], non_blocking=True)

    def launch(self, sources):
        """The two device calls on the current stream (no host synchronisation: capturable)."""
        st = _lib.stream_ptr()
        _lib.call("mpn_jpeg_forward", _lib.ptr(sources), sources.numel(), _lib.ptr(self._descs), self.n, _lib.ptr(self._coefs),
                  self._coefs.numel(), st)
        _lib.call("mpn_jpeg_entropy_encode", _lib.ptr(self._coefs), self._coefs.numel(), _lib.ptr(self._descs), self.n,
                  _lib.ptr(self._out), self._out.numel(), _lib.ptr(self._records), _lib.ptr(self._work), self._work.numel(), st)

    def collect(self, plan, sources, count=None):
        """The records, then the bytes used -> the files. Only [offset, offset + size) of every written stream is copied: one
        asynchronous copy per image into a PACKED pinned buffer, then one synchronise (`.copied_bytes`: records + streams). An
        image that did not fit is fetched as pixels and left to Pillow. count: collect the first `count` images of the plan
        only (a caller whose later images are unused slots); None: all of them."""
        import torch
        stream = torch.cuda.current_stream(self.device)
        n = len(plan.descs)
        if count is not None:
            if not 0 <= int(count) <= n:
                raise ValueError(f"encode: count must be in 0..{n} (got {count})")
            n = int(count)
        self._record_host[:n * RECORD_BYTES].copy_(self._records[:n * RECORD_BYTES], non_blocking=True)
        stream.synchronize()
        records = self._record_host.numpy().view(RECORD)[:n].copy()
        packed, at = [], 0
        for r in records:
            packed.append(at)
            if r['status'] == ENC_OK:                            # (size <= capacity, and the capacities fit the buffer)
                off, size = int(r['offset']), int(r['size'])
                self._out_host[at:at + size].copy_(self._out[off:off + size], non_blocking=True)
                at += size
        if at:
            stream.synchronize()
        self.copied_bytes = n * RECORD_BYTES + at
        host = self._out_host.numpy()
        files, self.fallbacks = [], 0
        for i, r in enumerate(records):
            if r['status'] == ENC_OK:
                files.append(plan.headers[i] + host[packed[i]:packed[i] + int(r['size'])].tobytes())
                continue
            if r['status'] == ENC_SKIPPED:
                raise _lib.MpnError(f"mpn_jpeg_entropy_encode skipped image {i}: its descriptor is out of range")
            (h, w), off = plan.shapes[i], plan.offsets[i]
            pixels = sources[off:off + h * w * plan.channels].cpu().numpy().reshape(h, w, plan.channels)
            files.append(pillow_encode(pixels, plan.quality, plan.subsampling))
            self.fallbacks += 1
        return files

    def encode(self, sources, offsets, shapes, channels, quality=75, subsampling='4:2:0', stream=None, capacities=None):
        import torch
        if sources.dtype != torch.uint8 or not sources.is_contiguous() or sources.device != self.device:
            raise ValueError("encode: sources must be a contiguous uint8 tensor on the encoder's device")
        plan = EncodePlan(shapes, offsets, channels, quality, subsampling, capacities)
        total = sources.numel()
        for (h, w), off in zip(plan.shapes, plan.offsets):
            if off < 0 or off + h * w * channels > total:
                raise ValueError(f"encode: an image of {(h, w, channels)} at byte {off} does not fit a buffer of {total} bytes")
        stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            self.reserve(len(plan.descs), *plan.need)
            self.upload(plan)
            self.launch(sources)
            return self.collect(plan, sources)


def encode_jpegs(images, quality=75, subsampling='4:2:0', device=None):
    """A list of uint8 [h, w, 3] arrays -> a list of `bytes`: the files Pillow writes for them with `save(buf, "JPEG",
    quality=quality, subsampling=subsampling)`, encoded on the device (one upload of the pixels, `JpegBatchEncoder.encode`)."""
    import torch
    items = list(images)
    if not items:
        raise ValueError("empty batch")
    for im in items:
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("an image must be a uint8 [height, width, 3] array")
    _sampling(subsampling)
    quality_tables(quality)
    device = _lib.current_device() if device is None else torch.device(device)
    offsets, at = [], 0
    for im in items:
        offsets.append(at)
        at += _round16(im.size)
    stage = torch.zeros(at, dtype=torch.uint8).pin_memory()
    host = stage.numpy()
    for im, off in zip(items, offsets):
        host[off:off + im.size] = im.reshape(-1)
    sources = stage.to(device, non_blocking=True)
    return JpegBatchEncoder(device).encode(sources, offsets, [im.shape[:2] for im in items], 3, quality, subsampling)
