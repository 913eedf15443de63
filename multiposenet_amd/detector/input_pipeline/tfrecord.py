"""TFRecord files and `tf.train.Example` records in pure Python (no TensorFlow, no protobuf package).

The files the reference's `data/create_tfrecords.py` writes (:89-94) and `KeypointPipeline.parse` reads
(keypoints_detector_pipeline.py:113-168):

    image        bytes   JPEG
    num_persons  int64
    boxes        float   [P*4]   absolute (ymin, xmin, ymax, xmax)
    keypoints    int64   [P*17*3] (y, x, visibility)
    masks        bytes   np.packbits of uint8 [ceil(H/4), ceil(W/4), 2] (0: loss mask, 1: segmentation mask)

Framing of one record: u64 length, u32 masked_crc32c(length), data, u32 masked_crc32c(data), little endian;
mask(c) = ((c >> 15) | (c << 17)) + 0xa282ead8 mod 2^32. The length CRC is always checked; the data CRC only with
`verify_data_crc=True` (table-driven CRC32C in Python costs tens of ms over a JPEG - far too slow for training).
"""
import struct

import numpy as np

__all__ = ["crc32c", "masked_crc32c", "read_records", "parse_example", "encode_example", "frame_record",
           "decode_keypoint_example", "unpack_masks", "decode_jpeg", "jpeg_shape"]


def _crc_table():
    poly = 0x82F63B78   # CRC-32C (Castagnoli), reflected
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ poly if c & 1 else c >> 1
        table.append(c)
    return table


_TABLE = _crc_table()


def crc32c(data, crc=0):
    """CRC-32C of `data` (bytes-like)."""
    c = crc ^ 0xFFFFFFFF
    t = _TABLE
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc32c(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def frame_record(data):
    """One framed TFRecord of the payload `data`."""
    n = struct.pack("<Q", len(data))
    return n + struct.pack("<I", masked_crc32c(n)) + bytes(data) + struct.pack("<I", masked_crc32c(data))


def read_records(path, verify_data_crc=False):
    """Yields the payload of every record of the TFRecord file `path` (uncompressed)."""
    with open(path, "rb") as f:
        offset = 0
        while True:
            head = f.read(12)
            if not head:
                return
            if len(head) < 12:
                raise IOError(f"{path}: truncated record header at byte offset {offset}")
            (length,) = struct.unpack("<Q", head[:8])
            (crc,) = struct.unpack("<I", head[8:])
            if masked_crc32c(head[:8]) != crc:
                raise IOError(f"{path}: corrupted record length at byte offset {offset}")
            data = f.read(length)
            tail = f.read(4)
            if len(data) < length or len(tail) < 4:
                raise IOError(f"{path}: truncated record at byte offset {offset} ({length} data bytes expected)")
            if verify_data_crc and masked_crc32c(data) != struct.unpack("<I", tail)[0]:
                raise IOError(f"{path}: corrupted record data at byte offset {offset}")
            yield data
            offset += 16 + length


# ---------------------------------------------------------------- protobuf wire format
def _varint(buf, pos):
    result = shift = 0
    while True:
        if pos >= len(buf):
            raise ValueError("truncated varint")
        b = buf[pos]
        pos += 1
        result |= (b & 0x7F) << shift
        if not b & 0x80:
            return result, pos
        shift += 7
        if shift >= 70:
            raise ValueError("varint too long")


def _fields(buf):
    """(field number, wire type, value) of a message: value is an int (varint), bytes (length-delimited) or raw bytes
    of a fixed32 / fixed64."""
    pos, n = 0, len(buf)
    while pos < n:
        key, pos = _varint(buf, pos)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(buf, pos)
        elif wt == 2:
            ln, pos = _varint(buf, pos)
            if pos + ln > n:
                raise ValueError("truncated length-delimited field")
            v, pos = buf[pos:pos + ln], pos + ln
        elif wt == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        elif wt == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        else:
            raise ValueError(f"unsupported wire type {wt}")
        yield num, wt, v


def _int64(u):
    return u - (1 << 64) if u >= (1 << 63) else u   # two's complement of a ten-byte varint


def _parse_feature(buf):
    # Feature { oneof { BytesList bytes_list = 1; FloatList float_list = 2; Int64List int64_list = 3; } }
    for num, wt, v in _fields(buf):
        if wt != 2:
            continue
        if num == 1:       # BytesList { repeated bytes value = 1; }
            return [bytes(x) for n, w, x in _fields(v) if n == 1 and w == 2]
        if num == 2:       # FloatList { repeated float value = 1 [packed]; }
            # packed (one length-delimited run) or unpacked (one fixed32 per value): little-endian floats either way
            out = [np.frombuffer(bytes(x), dtype="<f4") for n, w, x in _fields(v) if n == 1 and w in (2, 5)]
            return np.concatenate(out).astype(np.float32) if out else np.zeros(0, np.float32)
        if num == 3:       # Int64List { repeated int64 value = 1 [packed]; }
            out = []
            for n, w, x in _fields(v):
                if n != 1:
                    continue
                if w == 2:
                    p = 0
                    while p < len(x):
                        u, p = _varint(x, p)
                        out.append(_int64(u))
                elif w == 0:
                    out.append(_int64(x))
            return np.array(out, dtype=np.int64)
    return None   # an empty Feature


def parse_example(data):
    """Example { Features features = 1; }, Features { map<string, Feature> feature = 1; } -> {name: value}: a list of bytes,
    a float32 array or an int64 array."""
    out = {}
    buf = memoryview(data)
    for num, wt, v in _fields(buf):
        if num != 1 or wt != 2:
            continue
        for n, w, entry in _fields(v):
            if n != 1 or w != 2:
                continue
            key, val = None, None
            for en, ew, ev in _fields(entry):
                if en == 1 and ew == 2:
                    key = bytes(ev).decode("utf-8")
                elif en == 2 and ew == 2:
                    val = _parse_feature(ev)
            if key is not None:
                out[key] = val
    return out


def _enc_varint(u):
    out = bytearray()
    while True:
        b = u & 0x7F
        u >>= 7
        if u:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _enc_ld(num, payload):
    return _enc_varint((num << 3) | 2) + _enc_varint(len(payload)) + payload


def encode_example(features):
    """The inverse of parse_example for {name: bytes | list of bytes | float array | int array} (packed lists)."""
    entries = b""
    for key, val in features.items():
        if isinstance(val, (bytes, bytearray)):
            val = [bytes(val)]
        if isinstance(val, list) and (not val or isinstance(val[0], (bytes, bytearray))):
            feat = _enc_ld(1, b"".join(_enc_ld(1, bytes(x)) for x in val))
        else:
            a = np.asarray(val).reshape(-1)
            if np.issubdtype(a.dtype, np.floating):
                feat = _enc_ld(2, _enc_ld(1, a.astype("<f4").tobytes()))
            else:
                feat = _enc_ld(3, _enc_ld(1, b"".join(_enc_varint(int(x) & 0xFFFFFFFFFFFFFFFF) for x in a)))
        entry = _enc_ld(1, key.encode("utf-8")) + _enc_ld(2, feat)
        entries += _enc_ld(1, entry)
    return _enc_ld(1, entries)


# ---------------------------------------------------------------- the keypoint record contract
def unpack_masks(packed, mask_h, mask_w):
    """keypoints_detector_pipeline.py:155-166: the first mask_h * mask_w * 2 bits (MSB first) as uint8 [mh, mw, 2]."""
    n = mask_h * mask_w * 2
    bits = np.unpackbits(np.frombuffer(bytes(packed), np.uint8), count=n)
    if bits.size < n:
        raise ValueError(f"masks hold {bits.size} bits, {n} needed for [{mask_h}, {mask_w}, 2]")
    return bits.reshape(mask_h, mask_w, 2)


def decode_jpeg(data):
    """JPEG bytes -> uint8 [H, W, 3] RGB (tf.image.decode_jpeg(channels=3)) through PIL, imported on first use."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("decoding JPEG records needs PIL (Pillow), which is not installed; pass already decoded "
                          "examples (an in-memory source) instead") from e
    import io
    with Image.open(io.BytesIO(bytes(data))) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def jpeg_shape(data):
    """(height, width) of a JPEG stream without decoding it (tf.image.extract_jpeg_shape, prn_pipeline.py:63): the frame
    header SOF0..SOF15 (markers 0xC0-0xCF except DHT 0xC4, JPG 0xC8 and DAC 0xCC) holds precision u8, height u16, width u16,
    big endian. Raises ValueError on a stream without one."""
    buf = memoryview(data).cast("B") if not isinstance(data, (bytes, bytearray)) else data
    n = len(buf)
    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        raise ValueError("not a JPEG stream (no SOI marker)")
    pos = 2
    while pos + 4 <= n:
        if buf[pos] != 0xFF:
            raise ValueError(f"JPEG: marker expected at byte {pos}")
        m = buf[pos + 1]
        if m == 0xFF:                                   # fill byte
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:              # TEM, RSTn, SOI: no length
            pos += 2
            continue
        if m == 0xD9 or m == 0xDA:                      # EOI, or the scan began before any frame header
            break
        length = (buf[pos + 2] << 8) | buf[pos + 3]
        if length < 2:
            raise ValueError(f"JPEG: bad segment length at byte {pos}")
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if length < 7 or pos + 9 > n:
                raise ValueError("JPEG: truncated frame header")
            return (buf[pos + 5] << 8) | buf[pos + 6], (buf[pos + 7] << 8) | buf[pos + 8]
        pos += 2 + length
    raise ValueError("JPEG: no frame header (SOF) found")


def decode_keypoint_example(data, decode_image=True):
    """One serialized record of the contract above -> {'image': uint8 [H,W,3] (or the JPEG bytes with decode_image=False),
    'boxes': f32 [P,4], 'keypoints': int32 [P,17,3], 'masks': packed uint8 bytes}."""
    f = parse_example(data)
    for k in ("image", "num_persons", "masks"):
        if f.get(k) is None:
            raise ValueError(f"record has no '{k}' feature")
    p = int(f["num_persons"][0])
    boxes = f.get("boxes")
    kps = f.get("keypoints")
    boxes = np.zeros(0, np.float32) if boxes is None else boxes
    kps = np.zeros(0, np.int64) if kps is None else kps
    if boxes.size != p * 4 or kps.size != p * 17 * 3:
        raise ValueError(f"record: num_persons={p} but {boxes.size} box values and {kps.size} keypoint values")
    image = f["image"][0]
    return {"image": decode_jpeg(image) if decode_image else image,
            "boxes": boxes.reshape(p, 4).astype(np.float32),
            "keypoints": kps.reshape(p, 17, 3).astype(np.int32),
            "masks": np.frombuffer(f["masks"][0], np.uint8)}
