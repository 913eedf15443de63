"""A numpy / Python restatement of the device's JPEG entropy stage (include/mpn.h, "JPEG entropy decode on the device") on the
RAW bytes of a file: subsequences of S bits anchored at the file's first byte, a decoder state (raw bit position, block in the
MCU, zigzag index), f_i with byte stuffing, RSTn and the end marker, the fixed point of entry[i + 1] = f_i(entry[i]), the
exclusive prefix sum of the block counts, the write pass (DC as the difference) and the DC pass. `decode(data)` returns the
coefficients in the layout of `entropy_decode(data).coefs`.

Two ways to the same fixed point: `sweep=True` is the plain sweep of the scheme (every entry but the first starts as a guess,
all subsequences are re-decoded until nothing changes); `sweep=False` walks the chain once from the known entry, which is what
the sweeps converge to, and is what the long phase sweeps of the tests use."""
import numpy as np

S = 1024
TERMINAL = 0xFFFFFFFF
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def parse(data):
    """Headers of a baseline stream with one interleaved scan: geometry, restart interval, Huffman tables, scan offset."""
    assert data[:2] == b"\xff\xd8"
    pos, h = 2, {'restart': 0, 'huff': {}}
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        length = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + length]
        if m in (0xC0, 0xC1):
            h['height'], h['width'], n = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            h['ncomp'] = n
            h['hs'], h['vs'] = (seg[7] >> 4, seg[7] & 15) if n == 3 else (1, 1)
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                counts = list(seg[i + 1:i + 17])
                total = sum(counts)
                h['huff'][(seg[i] >> 4, seg[i] & 15)] = (counts, list(seg[i + 17:i + 17 + total]))
                i += 17 + total
        elif m == 0xDD:
            h['restart'] = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            n = seg[0]
            h['tables'] = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(n)]
            h['sos_at'], h['scan_offset'] = pos, pos + 2 + length
            return h
        pos += 2 + length


def lookup16(counts, symbols):
    """code in the top bits of 16 -> (length << 8) | symbol; 0 = no code starts these bits."""
    table = np.zeros(1 << 16, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            first = code << (16 - length)
            table[first:first + (1 << (16 - length))] = (length << 8) | symbols[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table.tolist()


class Scan:
    def __init__(self, data):
        self.data = data
        self.h = h = parse(data)
        self.nbytes = len(data)
        self.nsub = -(-self.nbytes * 8 // S)
        self.first = min(h['scan_offset'] * 8 // S, self.nsub - 1)
        hs, vs, n = h['hs'], h['vs'], h['ncomp']
        self.hv = hs * vs
        self.bpm = self.hv + 2 if n == 3 else 1
        self.mcus_x, self.mcus_y = -(-h['width'] // (8 * hs)), -(-h['height'] // (8 * vs))
        self.total = self.mcus_x * self.mcus_y * self.bpm
        self.dc = [lookup16(*h['huff'][(0, td)]) for td, _ in h['tables']]
        self.ac = [lookup16(*h['huff'][(1, ta)]) for _, ta in h['tables']]
        # the entropy-coded segments between markers: (clean bytes, raw index of each clean byte (+ the marker's), kind, after)
        raw = np.frombuffer(data, np.uint8)
        self.segments, self.segment_of = [], np.full(self.nbytes + 1, -1, np.int64)
        self.clean_of = np.zeros(self.nbytes + 1, np.int64)
        at = h['scan_offset']
        while at <= self.nbytes:
            k = at
            while True:                                     # the next FF that is not followed by 00
                if k >= self.nbytes:
                    kind, after = 'eof', self.nbytes
                    break
                if raw[k] == 0xFF:
                    if k + 1 < self.nbytes and raw[k + 1] == 0:
                        k += 2
                        continue
                    j = k + 1
                    while j < self.nbytes and raw[j] == 0xFF:
                        j += 1
                    if j >= self.nbytes:
                        kind, after = 'eof', self.nbytes
                    elif 0xD0 <= raw[j] <= 0xD7:
                        kind, after = 'rst', j + 1
                    else:
                        kind, after = 'end', self.nbytes
                    break
                k += 1
            idx = np.arange(at, k)
            stuffed = np.zeros(len(idx), bool)
            if len(idx) > 1:
                stuffed[1:] = (raw[idx[1:]] == 0) & (raw[idx[:-1]] == 0xFF)
            keep = idx[~stuffed]
            self.segment_of[at:k] = len(self.segments)
            self.clean_of[at:k] = np.cumsum(~stuffed) - 1 + stuffed          # a stuffed 00 maps to the byte behind it
            self.segments.append((bytes(raw[keep]) + b"\0" * 8, np.append(keep, k), kind, after))
            if kind != 'rst':
                break
            at = after

    def component(self, b):
        return 0 if b < self.hv else 1 + b - self.hv

    def f(self, i, entry, blk0=0, rst0=0, out=None):
        """Decodes whole symbols from `entry` = (raw bit position, b, z) until the position leaves subsequence i. Returns
        (exit state, blocks completed, restart markers passed). With `out` (true entries only) coefficients are stored as
        out[block of the decode order, zigzag -> natural] and every error raises ValueError."""
        pos, b, z = entry
        end = (i + 1) * S
        blocks = restarts = 0
        if pos >= end:
            return entry, 0, 0
        seg = self.segment_of[pos >> 3] if (pos >> 3) <= self.nbytes else -1
        if seg < 0:                                         # (a guess inside a marker, or behind the scan)
            return (TERMINAL, 0, 0), 0, 0
        final = out is not None
        while True:
            clean, raw_of, kind, after = self.segments[seg]
            nbits = (len(clean) - 8) * 8
            q = int(self.clean_of[pos >> 3]) * 8 + (pos & 7)
            while True:
                rem = nbits - q
                if rem < 8 and (rem <= 0 or clean[q >> 3] & ((1 << rem) - 1) == (1 << rem) - 1):
                    break                                   # only the padding of the last byte is left: 1-bits (no code is all ones)
                pos = int(raw_of[q >> 3]) * 8 + (q & 7)
                if pos >= end:
                    return (pos, b, z), blocks, restarts
                k = q >> 3
                w = (int.from_bytes(clean[k:k + 5], 'big') >> (8 - (q & 7))) & 0xFFFFFFFF
                e = (self.dc if z == 0 else self.ac)[self.component(b)][w >> 16]
                if e == 0:
                    if final:
                        raise ValueError("invalid code")
                    q += 1
                    continue
                length, sym = e >> 8, e & 255
                if z == 0:
                    if final and sym > 11:
                        raise ValueError("DC category above 11")
                    s, run = sym & 15, 0
                else:
                    s, run = sym & 15, sym >> 4
                v = (w >> (32 - length - s)) & ((1 << s) - 1) if s else 0
                if s and v < (1 << (s - 1)):
                    v -= (1 << s) - 1
                q += length + s
                if q > nbits:
                    if final:
                        raise ValueError("the scan ends inside a symbol")
                    return (TERMINAL, 0, 0), blocks, restarts
                if z == 0:
                    if final:
                        if blk0 + blocks >= self.total:
                            raise ValueError("more blocks than the image has")
                        out[blk0 + blocks, 0] = v
                    z = 1
                elif s:
                    z += run
                    if z > 63:
                        if final:
                            raise ValueError("a run past 63")
                        z = 63
                    if final:
                        out[blk0 + blocks, ZIGZAG[z]] = v
                    z += 1
                else:
                    z = z + 16 if run == 15 else 64
                if z >= 64:
                    z, b, blocks = 0, (b + 1) % self.bpm, blocks + 1
            if kind != 'rst':
                if final and (kind == 'eof' or b or z):
                    raise ValueError("the scan ends without a marker" if kind == 'eof' else "the scan ends inside a block")
                return (TERMINAL, 0, 0), blocks, restarts
            if final and (b or z or not self.h['restart'] or blk0 + blocks != (rst0 + restarts + 1) * self.h['restart'] * self.bpm):
                raise ValueError("block count disagrees at a restart marker")
            restarts, b, z, pos = restarts + 1, 0, 0, after * 8
            if pos >= end:
                return (pos, 0, 0), blocks, restarts
            seg += 1

    def entries(self, sweep):
        """The fixed point: (entries [first..nsub], counts, sweeps used)."""
        n, first = self.nsub, self.first
        known = (self.h['scan_offset'] * 8, 0, 0)
        if not sweep:
            entry, counts = {first: known}, {}
            for i in range(first, n):
                entry[i + 1], blocks, restarts = self.f(i, entry[i])
                counts[i] = (blocks, restarts)
            return entry, counts, 1
        entry = {i: (i * S, 0, 0) for i in range(first, n + 1)}
        entry[first] = known
        used, result = {}, {}
        for sweeps in range(1, n - first + 3):
            new = dict(entry)
            changed = False
            for i in range(first, n):
                if used.get(i) != entry[i]:
                    result[i] = self.f(i, entry[i])
                    used[i] = entry[i]
                    changed = True
                new[i + 1] = result[i][0]
            entry = new
            if not changed:
                break
        return entry, {i: result[i][1:] for i in range(first, n)}, sweeps - 1

    def decode(self, sweep=True):
        entry, counts, self.sweeps = self.entries(sweep)
        order = np.zeros((self.total, 64), np.int64)
        blk = rst = 0
        for i in range(self.first, self.nsub):              # exclusive prefix sums, then the write pass
            self.f(i, entry[i], blk, rst, order)
            blk, rst = blk + counts[i][0], rst + counts[i][1]
        want_rst = (self.total // self.bpm - 1) // self.h['restart'] if self.h['restart'] else 0
        if blk != self.total or rst != want_rst:
            raise ValueError("block count disagrees at the end")
        # DC pass: per-component running sum in decode order, reset every restart interval
        comp = np.array([self.component(b) for b in range(self.bpm)])[np.arange(self.total) % self.bpm]
        mcu = np.arange(self.total) // self.bpm
        interval = mcu // self.h['restart'] if self.h['restart'] else np.zeros(self.total, np.int64)
        for c in range(self.h['ncomp']):
            for k in np.unique(interval):
                sel = (comp == c) & (interval == k)
                order[sel, 0] = np.cumsum(order[sel, 0])
        # decode order -> planes per component, raster order over the padded block grid
        hs, vs = self.h['hs'], self.h['vs']
        bi = np.arange(self.total) % self.bpm
        my, mx = mcu // self.mcus_x, mcu % self.mcus_x
        luma = (my * vs + bi // hs) * (self.mcus_x * hs) + mx * hs + bi % hs
        base1 = self.mcus_x * self.mcus_y * self.hv
        chroma = base1 + (comp - 1) * self.mcus_x * self.mcus_y + my * self.mcus_x + mx
        planes = np.zeros((self.total, 64), np.int16)
        planes[np.where(comp == 0, luma, chroma)] = order.astype(np.int16)
        return planes


def decode(data, sweep=True):
    return Scan(data).decode(sweep)


def with_comment(data, length):
    """The file with a COM segment of `length` >= 2 bytes (its length field: the two length bytes and length - 2 of payload)
    in front of its SOS: the scan moves by length + 2 bytes."""
    at = parse(data)['sos_at']
    return data[:at] + b"\xff\xfe" + length.to_bytes(2, 'big') + bytes((i * 37 + 11) % 251 for i in range(length - 2)) + data[at:]
