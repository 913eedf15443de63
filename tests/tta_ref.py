"""numpy float32 transcription of mpn_mirror_images and mpn_tta_merge (include/mpn.h): the yardstick of the test-time
augmentation tests. Every array operation below is one separately rounded IEEE f32 operation per element, in the order the
header states, so the kernels equal these functions bit for bit."""
import numpy as np

from multiposenet_amd.detector.input_pipeline.keypoint_augment import FLIP_ORDER

F = np.float32


def mirror_images(images):
    """uint8 [n, h, w, 3] -> out[i, y, x, :] = in[i, y, w-1-x, :]."""
    return np.ascontiguousarray(images[:, :, ::-1])


def unmirror(heat, seg):
    """The maps of a mirrored input, seen from the unmirrored image: columns reversed, left / right channels swapped."""
    return np.ascontiguousarray(heat[:, :, ::-1][..., FLIP_ORDER]), np.ascontiguousarray(seg[:, :, ::-1])


def _axis(n_in, n_out):
    i = np.arange(n_out, dtype=F)
    s = (i + F(0.5)) * (F(n_in) / F(n_out)) - F(0.5)
    s = np.minimum(np.maximum(s, F(0.0)), F(n_in - 1))
    assert s.dtype == F
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0.astype(F)


def resize(a, h0, w0):
    """f32 [b, h, w] or [b, h, w, c] -> [b, h0, w0(, c)]: bilinear, half-pixel centres, clamped edges; the same size is read
    directly."""
    assert a.dtype == F
    h, w = a.shape[1:3]
    if (h, w) == (h0, w0):
        return a
    y0, y1, fy = _axis(h, h0)
    x0, x1, fx = _axis(w, w0)
    tail = (1,) * (a.ndim - 3)
    fy, fx = fy.reshape((1, h0, 1) + tail), fx.reshape((1, 1, w0) + tail)
    r0, r1 = a[:, y0], a[:, y1]
    a00, a01, a10, a11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    top = a00 + (a01 - a00) * fx
    bot = a10 + (a11 - a10) * fx
    v = top + (bot - top) * fy
    assert v.dtype == F
    return v


def merge(sources, size=None):
    """sources: [(heat f32 [b, h_k, w_k, 17], seg f32 [b, h_k, w_k], mirrored)], at most 8. size: (h0, w0) of the output
    (default: the first source's). Returns (heat [b, h0, w0, 17], seg [b, h0, w0])."""
    assert 1 <= len(sources) <= 8
    h0, w0 = size if size is not None else sources[0][0].shape[1:3]
    out = []
    for which in (0, 1):
        acc = None
        for heat, seg, mirrored in sources:
            maps = unmirror(heat, seg) if mirrored else (heat, seg)
            v = resize(np.asarray(maps[which]), h0, w0)
            acc = v if acc is None else acc + v
        r = acc / F(len(sources))
        assert r.dtype == F
        out.append(np.ascontiguousarray(r))
    return out[0], out[1]
