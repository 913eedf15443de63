"""numpy restatement of the DEVICE stage of the JPEG decode (mpn_jpeg_decode): raw coefficients and quantisation tables ->
uint8 RGB, in libjpeg's integer arithmetic (jidctint.c "slow integer" inverse DCT, jdsample.c fancy upsampling, jdcolor.c
YCbCr -> RGB). Written from the library's published algorithm, in int64, with none of the kernels' structure."""
import numpy as np

CONST_BITS, PASS1_BITS = 13, 2
F = {n: v for n, v in (("0_298", 2446), ("0_390", 3196), ("0_541", 4433), ("0_765", 6270), ("0_899", 7373), ("1_175", 9633),
                       ("1_501", 12299), ("1_847", 15137), ("1_961", 16069), ("2_053", 16819), ("2_562", 20995), ("3_072", 25172))}


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(v, shift):
    """v: int64 [..., 8] along the last axis -> the 8 outputs of one pass, descaled by `shift`."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k] for k in range(8))
    z1 = (i2 + i6) * F["0_541"]
    tmp2 = z1 - i6 * F["1_847"]
    tmp3 = z1 + i2 * F["0_765"]
    tmp0 = (i0 + i4) << CONST_BITS
    tmp1 = (i0 - i4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F["1_175"]
    t0, t1, t2, t3 = t0 * F["0_298"], t1 * F["2_053"], t2 * F["3_072"], t3 * F["1_501"]
    z1, z2 = -z1 * F["0_899"], -z2 * F["2_562"]
    z3, z4 = -z3 * F["1_961"] + z5, -z4 * F["0_390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([_descale(o, shift) for o in out], axis=-1)


def idct_plane(coefs, quant):
    """coefs int16 [bh, bw, 8, 8] (natural order), quant [8, 8] -> uint8 [bh*8, bw*8]."""
    x = coefs.astype(np.int64) * quant.astype(np.int64)
    # pass 1 works on COLUMNS (along axis 2), pass 2 on rows
    ws = np.swapaxes(_idct_1d(np.swapaxes(x, 2, 3), CONST_BITS - PASS1_BITS), 2, 3)
    px = _idct_1d(ws, CONST_BITS + PASS1_BITS + 3)
    idx = px & 1023                                             # the library's range-limit table, 10-bit index
    signed = np.where(idx >= 512, idx - 1024, idx)
    out = np.clip(signed + 128, 0, 255).astype(np.uint8)
    bh, bw = coefs.shape[:2]
    return out.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1_fancy(p):
    """[h, cw] -> [h, 2*cw]: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2, ends copied."""
    p = p.astype(np.int64)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    return np.stack([even, odd], axis=2).reshape(p.shape[0], -1)


def _h2v2_fancy(p):
    """[ch, cw] -> [2*ch, 2*cw]: column sums 3*near + far (far = the row above for even output rows, below for odd ones, the
    edge rows repeated), then (3 this + neighbour + 8) >> 4 for even and (... + 7) >> 4 for odd columns, ends this * 4."""
    p = p.astype(np.int64)
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    rows = np.stack([3 * p + above, 3 * p + below], axis=1).reshape(-1, p.shape[1])
    left = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    even, odd = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    return np.stack([even, odd], axis=2).reshape(rows.shape[0], -1)


def upsample(plane, width, height, hs, vs):
    """A chroma plane on its padded grid -> [height, width] at full resolution."""
    cw, ch = -(-width // hs), -(-height // vs)
    p = plane[:ch, :cw]
    if hs == 1 and vs == 1:
        return p.astype(np.int64)
    if cw <= 2:                                                 # the library replicates such a component
        up = np.repeat(np.repeat(p, vs, axis=0), hs, axis=1).astype(np.int64)
    else:
        up = _h2v1_fancy(p) if vs == 1 else _h2v2_fancy(p)
    return up[:height, :width]


def decode(planes, width, height, hs, vs):
    """planes: [(coefs [bh, bw, 8, 8], quant [8, 8])] of 1 or 3 components -> uint8 [height, width, 3]."""
    y = idct_plane(*planes[0])[:height, :width].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    cb = upsample(idct_plane(*planes[1]), width, height, hs, vs) - 128
    cr = upsample(idct_plane(*planes[2]), width, height, hs, vs) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode_coefficients(c):
    """A `multiposenet_amd.inference.jpeg.Coefficients` -> uint8 [h, w, 3]."""
    d = c.desc[0]
    return decode(c.planes(), int(d['width']), int(d['height']), int(d['h_samp']), int(d['v_samp']))
