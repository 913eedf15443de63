"""Numpy restatement of the baseline JPEG encoder as libjpeg(-turbo) - and so Pillow's `save(buf, "JPEG", quality=q,
subsampling=s)` - runs it: pixels -> quantised coefficients -> the entropy-coded scan -> the whole file. Written from the rules
in DESIGN.md ("JPEG encode"), with no code shared with multiposenet_amd: it is the yardstick the device kernels are held to,
and is itself held to Pillow's files byte for byte (tests/test_jpeg_encode_host.py)."""
import numpy as np

SAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}

# Annex K.1 / K.2, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

# zigzag position -> natural position
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                    21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                    60, 61, 54, 47, 55, 62, 63])

# Annex K.3 - K.6 as a DHT segment holds them: 16 counts, then the symbols. (class, id): DC luma, AC luma, DC chroma, AC chroma
_AC_TAIL = ("16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 "
            "69 6a 73 74 75 76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 "
            "b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 "
            "f8 f9 fa")
HUFFMAN = [
    (0, 0, bytes.fromhex("00 01 05 01 01 01 01 01 01 00 00 00 00 00 00 00"), bytes(range(12))),
    (1, 0, bytes.fromhex("00 02 01 03 03 02 04 03 05 05 04 04 00 00 01 7d"),
     bytes.fromhex("01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 82 09 0a"
                   + _AC_TAIL)),
    (0, 1, bytes.fromhex("00 03 01 01 01 01 01 01 01 01 01 00 00 00 00 00"), bytes(range(12))),
    (1, 1, bytes.fromhex("00 02 01 02 04 04 03 04 07 05 04 04 00 01 02 77"),
     bytes.fromhex("00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 0a 16 24 "
                   "34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 "
                   "66 67 68 69 6a 73 74 75 76 77 78 79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 "
                   "a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 e8 e9 ea "
                   "f2 f3 f4 f5 f6 f7 f8 f9 fa")),
]


def quality_tables(quality):
    """The two 8-bit tables (natural order, int64 [64]) libjpeg derives from Annex K for `quality` in 1..100."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((base * scale + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA)]


def _codes(bits, vals):
    """symbol -> (code, length) of a DHT table (Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


# ------------------------------------------------------------------------------------------------ pixels -> component planes
def _fix(x):
    return int(x * 65536 + 0.5)


def ycbcr(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(0.299) * r + _fix(0.587) * g + _fix(0.114) * b + 32768) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_right(p, width):
    return np.concatenate([p, np.repeat(p[:, -1:], width - p.shape[1], axis=1)], axis=1) if width > p.shape[1] else p


def _pad_bottom(p, height):
    return np.concatenate([p, np.repeat(p[-1:], height - p.shape[0], axis=0)], axis=0) if height > p.shape[0] else p


def component_planes(rgb, hs, vs):
    """[Y, Cb, Cr] as int64 planes on their padded block grids, with libjpeg's edge rules."""
    h, w = rgb.shape[:2]
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    y, cb, cr = ycbcr(rgb[..., :3])
    planes = [_pad_bottom(_pad_right(y, mx * hs * 8), my * vs * 8)]
    for c in (cb, cr):
        c = _pad_bottom(_pad_right(c, mx * hs * 8), -(-h // vs) * vs)      # the source only up to a multiple of v_samp
        if (hs, vs) == (2, 2):
            bias = 1 + (np.arange(c.shape[1] // 2) & 1)
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        elif (hs, vs) == (2, 1):
            bias = np.arange(c.shape[1] // 2) & 1
            c = (c[:, 0::2] + c[:, 1::2] + bias) >> 1
        planes.append(_pad_bottom(c, my * 8))                              # then the last DOWNSAMPLED row
    return planes


# ------------------------------------------------------------------------------------------------ forward DCT, quantisation
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """One pass of the slow-integer forward DCT over the last axis (jfdctint.c)."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2], out[6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def _blocks_of(plane):
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    return plane.reshape(bh, 8, bw, 8).swapaxes(1, 2)                     # [bh, bw, 8 rows, 8 columns]


def forward(rgb, tables, hs, vs):
    """Pixels -> int16 [total_blocks, 64]: the layout of `entropy_decode(...).coefs`."""
    h, w = rgb.shape[:2]
    out = []
    for c, plane in enumerate(component_planes(rgb, hs, vs)):
        x = _blocks_of(plane) - 128
        x = _fdct_1d(x, True)                                             # rows
        x = np.swapaxes(_fdct_1d(np.swapaxes(x, 2, 3), False), 2, 3)      # columns
        q8 = 8 * np.asarray(tables[min(c, 1)], np.int64).reshape(8, 8)
        x = np.sign(x) * ((np.abs(x) + (q8 >> 1)) // q8)
        if c == 0:                                                        # dummy blocks beyond the component's own grid
            rbw, rbh = -(-w // 8), -(-h // 8)
            bh, bw = x.shape[:2]
            for by in range(bh):
                for bx in range(bw):
                    if by < rbh and bx < rbw:
                        continue
                    sy, sx = (by - 1, bx | (hs - 1)) if by >= rbh else (by, bx)
                    if sx >= rbw:
                        sx -= 1
                    dc = x[sy, sx, 0, 0]
                    x[by, bx] = 0
                    x[by, bx, 0, 0] = dc
        out.append(x.reshape(-1, 64))
    return np.concatenate(out).astype(np.int16)


# ------------------------------------------------------------------------------------------------ coefficients -> scan
class _BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, code, length):
        self.bits.append((int(code), int(length)))

    def finish(self):
        acc, n, out = 0, 0, bytearray()
        for code, length in self.bits:
            acc = (acc << length) | code
            n += length
            while n >= 8:
                n -= 8
                byte = (acc >> n) & 255
                out.append(byte)
                if byte == 255:
                    out.append(0)
            acc &= (1 << n) - 1
        if n:
            byte = ((acc << (8 - n)) | ((1 << (8 - n)) - 1)) & 255
            out.append(byte)
            if byte == 255:
                out.append(0)
        return bytes(out)


def _size(v):
    return int(abs(int(v))).bit_length()


def scan(coefs, width, height, hs, vs):
    """int16 [total_blocks, 64] -> the entropy-coded segment through the EOI marker."""
    tables = {(cls, tid): _codes(bits, vals) for cls, tid, bits, vals in HUFFMAN}
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    bw = [mx * hs, mx, mx]
    base = [0, mx * hs * my * vs, mx * hs * my * vs + mx * my]
    w = _BitWriter()
    pred = [0, 0, 0]
    for m_y in range(my):
        for m_x in range(mx):
            for c in range(3):
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                dc, ac = tables[(0, min(c, 1))], tables[(1, min(c, 1))]
                for v in range(cv):
                    for hh in range(ch):
                        blk = coefs[base[c] + (m_y * cv + v) * bw[c] + m_x * ch + hh].astype(np.int64)
                        diff = int(blk[0]) - pred[c]
                        pred[c] = int(blk[0])
                        s = _size(diff)
                        w.put(*dc[s])
                        if s:
                            w.put((diff if diff > 0 else diff - 1) & ((1 << s) - 1), s)
                        run = 0
                        for k in range(1, 64):
                            val = int(blk[NATURAL[k]])
                            if val == 0:
                                run += 1
                                continue
                            while run > 15:
                                w.put(*ac[0xF0])
                                run -= 16
                            s = _size(val)
                            w.put(*ac[(run << 4) | s])
                            w.put((val if val > 0 else val - 1) & ((1 << s) - 1), s)
                            run = 0
                        if run:
                            w.put(*ac[0])
    return w.finish() + b"\xff\xd9"


# ------------------------------------------------------------------------------------------------ the file
def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def headers(width, height, hs, vs, tables):
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate(tables):
        out += _segment(0xDB, bytes([i]) + bytes(int(t[n]) for n in NATURAL))
    out += _segment(0xC0, b"\x08" + height.to_bytes(2, 'big') + width.to_bytes(2, 'big') + b"\x03"
                    + bytes([1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, tid, bits, vals in HUFFMAN:
        out += _segment(0xC4, bytes([(cls << 4) | tid]) + bits + vals)
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(rgb, quality, subsampling):
    """uint8 [h, w, 3 or 4] -> (coefficients, scan bytes, whole file)."""
    hs, vs = SAMPLING[subsampling]
    h, w = rgb.shape[:2]
    tables = quality_tables(quality)
    coefs = forward(rgb, tables, hs, vs)
    s = scan(coefs, w, h, hs, vs)
    return coefs, s, headers(w, h, hs, vs, tables) + s
