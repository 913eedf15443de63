"""The yardstick of the COCO mask rasteriser (multiposenet_amd/coco_records.py, csrc/coco_masks.hip): the four stages of the
record's mask feature as plain sequential loops, written from the published algorithms.

    1. polygon -> run-length code     COCO maskApi rleFrPoly: dense boundary walk at 5x, boundary crossings, a sort, run lengths
    2. merge and decode               maskApi rleMerge (union) over an annotation's polygons, rleDecode (column-major)
    3. image masks                    seg = OR over kept persons, loss = AND over dropped persons of (mask == 0)
    4. Lanczos4 to quarter size       OpenCV resize(INTER_LANCZOS4) on uint8: 8 taps, 11-bit fixed-point weights, (x + 2^21) >> 22;
                                      then `> 0` and numpy.packbits

Neither pycocotools nor OpenCV is a dependency of this project: this file is the definition the project adopts, and equality
with the two libraries is the intent, not something the suite checks. One case the C code leaves undefined is settled here:
an edge whose two ends round to the same 5x grid point (maskApi divides 0 by 0 and casts the NaN to int) emits that point once.

An annotation is a dict with 'segmentation' (a list of polygons, each a flat [x0, y0, x1, y1, ...] list, or a dict whose
'counts' is a list of run lengths or a compressed string) and 'dropped' (bool)."""
import math

import numpy as np

SCALE = 5.0
COEF_BITS = 11                                  # OpenCV's INTER_RESIZE_COEF_BITS
FLT_EPSILON = 1.1920928955078125e-07


# ---------------------------------------------------------------- stage 1: maskApi rleFrPoly
def _cint(v):
    """A C cast of a double to int: truncation toward zero."""
    return int(v)


def poly_to_rle(xy, h, w):
    """A flat polygon [x0, y0, x1, y1, ...] (float64) -> run lengths (column-major, starting with a run of zeros)."""
    xy = [float(v) for v in xy]
    k = len(xy) // 2
    if k == 0:
        return [h * w]
    x = [_cint(SCALE * xy[2 * j] + .5) for j in range(k)]
    y = [_cint(SCALE * xy[2 * j + 1] + .5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = float(ye - ys) / dx if dx > 0 else 0.0
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(_cint(ys + s * t + .5))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(_cint(xs + s * t + .5))
    a = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / SCALE - .5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / SCALE - .5
        if yd < 0:
            yd = 0.0
        elif yd > h:
            yd = float(h)
        yd = math.ceil(yd)
        a.append(int(xd) * h + int(yd))
    a.append(h * w)
    a.sort()
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    b = [a[0]]
    j = 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return b


# ---------------------------------------------------------------- stage 2: rleMerge (union), rleDecode, the string form
def rle_merge(rles):
    """maskApi rleMerge with intersect = 0 over run-length codes of one size."""
    cnts = list(rles[0])
    for other in rles[1:]:
        A, B = cnts, list(other)
        ca, cb = A[0], B[0]
        v = va = vb = 0
        a = b = 1
        cc, ct = 0, 1
        out = []
        while ct > 0:
            c = min(ca, cb)
            cc += c
            ct = 0
            ca -= c
            if not ca and a < len(A):
                ca = A[a]
                a += 1
                va = 1 - va
            ct += ca
            cb -= c
            if not cb and b < len(B):
                cb = B[b]
                b += 1
                vb = 1 - vb
            ct += cb
            vp = v
            v = 1 if (va or vb) else 0
            if v != vp or ct == 0:
                out.append(cc)
                cc = 0
        cnts = out
    return cnts


def rle_decode(cnts, h, w):
    """Run lengths -> uint8 [h, w] of 0 / 1 (runs fill the column-major order, alternately 0 and 1; what lies past h * w is
    cut off, what the runs do not reach stays 0)."""
    flat = np.zeros(h * w, np.uint8)
    at, val = 0, 0
    for c in cnts:
        c = int(c)
        if val and at < h * w:
            flat[at:min(at + c, h * w)] = 1
        at += c
        val = 1 - val
    return np.ascontiguousarray(flat.reshape(w, h).T)


def rle_encode(mask):
    """uint8 [h, w] -> run lengths (maskApi rleEncode)."""
    flat = np.asarray(mask).T.reshape(-1)
    cnts, prev, run = [], 0, 0
    for b in flat:
        b = 1 if b else 0
        if b != prev:
            cnts.append(run)
            run, prev = 0, b
        run += 1
    cnts.append(run)
    return cnts


def rle_to_string(cnts):
    """maskApi rleToString: COCO's compressed form of the run lengths."""
    s = []
    for i, c in enumerate(cnts):
        x = int(c)
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            c5 = x & 0x1f
            x >>= 5
            more = (x != -1) if (c5 & 0x10) else (x != 0)
            if more:
                c5 |= 0x20
            s.append(chr(c5 + 48))
    return "".join(s)


def rle_from_string(s):
    """maskApi rleFrString."""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def annotation_mask(segmentation, h, w):
    """COCO's annToMask: uint8 [h, w] of 0 / 1."""
    if isinstance(segmentation, dict):
        cnts = segmentation['counts']
        if isinstance(cnts, (str, bytes)):
            cnts = rle_from_string(cnts)
        return rle_decode(cnts, h, w)
    rles = [poly_to_rle(p, h, w) for p in segmentation]
    if not rles:
        return np.zeros((h, w), np.uint8)
    return rle_decode(rle_merge(rles), h, w)


# ---------------------------------------------------------------- stage 3
def image_masks(h, w, annotations):
    """uint8 [h, w, 2] of 0 / 1: channel 0 the loss mask, channel 1 the segmentation mask."""
    loss = np.ones((h, w), bool)
    seg = np.zeros((h, w), bool)
    for a in annotations:
        m = annotation_mask(a['segmentation'], h, w)
        if a['dropped']:
            loss = np.logical_and(m == 0, loss)
        else:
            seg = np.logical_or(m == 1, seg)
    return np.stack([loss, seg], 2).astype(np.uint8)


# ---------------------------------------------------------------- stage 4: OpenCV resize(INTER_LANCZOS4) on uint8
def _lanczos4(x):
    """OpenCV's interpolateLanczos4: the eight float32 weights of the fraction x (float32)."""
    f32 = np.float32
    if x < f32(FLT_EPSILON):
        return [f32(0)] * 3 + [f32(1)] + [f32(0)] * 4
    s45 = 0.70710678118654752440084436210485
    cs = [[1, 0], [-s45, -s45], [0, 1], [s45, -s45], [-1, 0], [s45, s45], [0, -1], [-s45, s45]]
    pi = 3.1415926535897932384626433832795
    y0 = -float(x + f32(3)) * pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    coeffs, total = [], f32(0)
    for i in range(8):
        y = -float(x + f32(3) - f32(i)) * pi * 0.25
        c = f32((cs[i][0] * s0 + cs[i][1] * c0) / (y * y))
        coeffs.append(c)
        total = f32(total + c)
    total = f32(f32(1) / total)
    return [f32(c * total) for c in coeffs]


def lanczos_taps(src, dst):
    """One axis: `first` int32 [dst] (floor of the source coordinate; the taps sit at first - 3 .. first + 4) and `weights`
    int16 [dst, 8] = saturate_cast<short>(weight * 2048), rounded half to even."""
    scale = 1.0 / (float(dst) / float(src))
    first = np.zeros(dst, np.int32)
    weights = np.zeros((dst, 8), np.int16)
    for d in range(dst):
        fx = np.float32((d + 0.5) * scale - 0.5)
        s = math.floor(float(fx))
        fx = np.float32(fx - np.float32(s))
        first[d] = s
        for k, c in enumerate(_lanczos4(fx)):
            q = int(np.rint(np.float32(c * np.float32(1 << COEF_BITS))))
            weights[d, k] = max(-32768, min(32767, q))
    return first, weights


def lanczos_quarter(masks):
    """uint8 [h, w, c] -> uint8 [ceil(h/4), ceil(w/4), c]: horizontal pass (integer sums), vertical pass, (x + 2^21) >> 22
    saturated to 0..255; replicate border."""
    masks = np.asarray(masks, np.uint8)
    h, w = masks.shape[:2]
    mh, mw = -(-h // 4), -(-w // 4)
    fx, wx = lanczos_taps(w, mw)
    fy, wy = lanczos_taps(h, mh)
    src = masks.astype(np.int64)
    rows = np.zeros((h, mw) + masks.shape[2:], np.int64)
    for k in range(8):
        cols = np.clip(fx - 3 + k, 0, w - 1)
        rows += src[:, cols] * wx[:, k].astype(np.int64).reshape((1, mw) + (1,) * (masks.ndim - 2))
    out = np.zeros((mh, mw) + masks.shape[2:], np.int64)
    for k in range(8):
        r = np.clip(fy - 3 + k, 0, h - 1)
        out += rows[r] * wy[:, k].astype(np.int64).reshape((mh, 1) + (1,) * (masks.ndim - 2))
    out = (out + (1 << (2 * COEF_BITS - 1))) >> (2 * COEF_BITS)
    return np.clip(out, 0, 255).astype(np.uint8)


def pack(small):
    return np.packbits(small > 0)


# ---------------------------------------------------------------- all four
def rasterize_image(h, w, annotations):
    """-> (packed uint8 [ceil(mh * mw * 2 / 8)], full uint8 [h, w, 2])."""
    full = image_masks(h, w, annotations)
    return pack(lanczos_quarter(full)), full


def rasterize(items, return_full=False):
    """The call of `CocoMaskRasterizer.rasterize` on the host: items = [(h, w, annotations)]."""
    res = [rasterize_image(h, w, anns) for h, w, anns in items]
    packed = [r[0] for r in res]
    return (packed, [r[1] for r in res]) if return_full else packed
