"""Exact-integer inputs and references for the pixel reductions (weight gradients, A B^T, batch-norm slabs).

Every kernel covered here forms f32 sums of products of storage-typed operands. With integer-valued operands (and an affine
whose result is again a small integer) every product and every partial sum is an integer below 2^24, hence exactly
representable in f32 - in ANY summation order, on matrix cores or on the vector ALU. The kernels' results must then equal
these references bit for bit, whatever the split count, tile walk or grouping: `assert_exact` is `torch.equal`.

References are float64 on values that are integers by construction (products and sums far below 2^53: exact), written as
shifted slices and matrix products. They do not go through oracle.network; tests/test_reduction_exact_host.py checks them
against the oracle's autograd.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
X_MAX = 8          # |x| <= 8 (16 on channels of scale 0.5, even there): x * scale + shift spans [-19, 19], so ReLU6 clips about
SHIFT_MAX = 3      # half the elements at 0 and about a third at 6; |act(.)| <= 19 is exact in bf16 (8 bits) and fp16 (11 bits)
DY_MAX = 3
EXACT_LIMIT = float(2 ** 24)


# ------------------------------------------------------------------------------------------------------------ generators
def int_tensor(rs, shape, lo, hi):
    """Integer-valued f32 CPU tensor, uniform in [lo, hi]."""
    return torch.from_numpy(rs.randint(lo, hi + 1, size=shape).astype(np.float32))


def int_affine(rs, C):
    """Per-channel scale from {0.5, 1, 2} and integer shift in [-SHIFT_MAX, SHIFT_MAX] (f32)."""
    scale = torch.from_numpy(rs.choice(np.array([0.5, 1.0, 2.0], np.float32), size=C))
    shift = int_tensor(rs, (C,), -SHIFT_MAX, SHIFT_MAX)
    return scale, shift


def int_activations(rs, shape, scale, x_max=X_MAX):
    """x in [-x_max, x_max], doubled on the channels whose scale is 0.5: x * scale + shift is an integer on every channel."""
    x = int_tensor(rs, shape, -x_max, x_max)
    return x * torch.where(scale == 0.5, 2.0, 1.0)


def representable16(t):
    """True when every value survives a round trip through bf16 AND fp16."""
    t = t.float()
    return bool(torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t))


def act_affine(x, scale, shift, act):
    """act(x * scale + shift) in float64; asserts the result is integer-valued and exact in both 16-bit formats."""
    a = x.double() if scale is None else x.double() * scale.double() + shift.double()
    if act == ACT_RELU:
        a = a.clamp(min=0)
    elif act == ACT_RELU6:
        a = a.clamp(0, 6)
    assert bool((a == a.round()).all()) and representable16(a) and representable16(x)
    return a


# ------------------------------------------------------------------------------------------------------------ references
def tf_same(size, stride):
    """(output size, padding before) of a 3-tap TF SAME window."""
    out = -(-size // stride)
    total = max((out - 1) * stride + 3 - size, 0)
    return out, total // 2


def _taps(a, OH, OW, stride):
    """The nine strided views a_pad[n, oy * stride + ty, ox * stride + tx, c] of a [N,H,W,C] tensor under TF SAME padding."""
    N, H, W, C = a.shape
    (_, pt), (_, pl) = tf_same(H, stride), tf_same(W, stride)
    need_h, need_w = (OH - 1) * stride + 3, (OW - 1) * stride + 3
    ap = F.pad(a, (0, 0, pl, max(need_w - W - pl, 0), pt, max(need_h - H - pt, 0)))
    for ty in range(3):
        for tx in range(3):
            yield ty, tx, ap[:, ty:ty + (OH - 1) * stride + 1:stride, tx:tx + (OW - 1) * stride + 1:stride, :]


def conv_wgrad_ref(a, dy, ksize, stride=1):
    """dW[ty][tx][ci][co] = sum over pixels of a[pixel + tap][ci] * dy[pixel][co]: dense 3x3 (TF SAME; stride 1 = the symmetric
    SAME of the network's 3x3 layers, stride 2 = the stem) or 1x1. a [N,H,W,Cin], dy [N,OH,OW,Cout]; float64 [k,k,Cin,Cout]."""
    a, dy = a.double(), dy.double()
    Cin, Cout = a.shape[3], dy.shape[3]
    if ksize == 1:
        return (a.reshape(-1, Cin).t() @ dy.reshape(-1, Cout)).reshape(1, 1, Cin, Cout)
    OH, OW = dy.shape[1], dy.shape[2]
    assert OH == tf_same(a.shape[1], stride)[0] and OW == tf_same(a.shape[2], stride)[0]
    dw = torch.zeros(3, 3, Cin, Cout, dtype=torch.float64)
    d2 = dy.reshape(-1, Cout)
    for ty, tx, v in _taps(a, OH, OW, stride):
        dw[ty, tx] = v.reshape(-1, Cin).t() @ d2
    return dw


def stem_wgrad_ref(images, dy):
    """The stem's weight gradient: 3x3, stride 2, TF SAME over 2 * image - 1."""
    return conv_wgrad_ref(2.0 * images.double() - 1.0, dy, 3, 2)


def dwconv_wgrad_ref(a, dy, stride):
    """Depthwise dW[ty][tx][c] = sum over output pixels of a_pad[n, oy * s + ty, ox * s + tx, c] * dy[n, oy, ox, c]; [3,3,C]."""
    a, dy = a.double(), dy.double()
    OH, OW = dy.shape[1], dy.shape[2]
    assert OH == tf_same(a.shape[1], stride)[0] and OW == tf_same(a.shape[2], stride)[0]
    dw = torch.zeros(3, 3, a.shape[3], dtype=torch.float64)
    for ty, tx, v in _taps(a, OH, OW, stride):
        dw[ty, tx] = (v * dy).sum((0, 1, 2))
    return dw


def gemm_nt_ref(a, b):
    """A [M,K] B[N,K]^T."""
    return a.double() @ b.double().t()


def head_ref(a, dl):
    """The heatmap head's dW [C,18] = a^T dlogits and db [18] = column sums of dlogits, flat as the kernel's slab row."""
    a, dl = a.double().reshape(-1, a.shape[-1]), dl.double().reshape(-1, dl.shape[-1])
    return torch.cat([(a.t() @ dl).reshape(-1), dl.sum(0)])


def stats_ref(x):
    """[2][C]: sum x and sum x^2 over the rows."""
    x = x.double().reshape(-1, x.shape[-1])
    return torch.stack([x.sum(0), (x * x).sum(0)])


def bn_bwd_sums_ref(dA, x, scale, shift, mean, invstd, act):
    """[2][C]: sum g and sum g * xhat, g = dA where the activation of x * scale + shift passes, xhat = (x - mean) * invstd."""
    C = x.shape[-1]
    dA, x = dA.double().reshape(-1, C), x.double().reshape(-1, C)
    pre = x * scale.double() + shift.double()
    ok = torch.ones_like(pre, dtype=torch.bool)
    if act != ACT_NONE:
        ok = pre > 0
    if act == ACT_RELU6:
        ok = ok & (pre < 6)
    g = torch.where(ok, dA, torch.zeros_like(dA))
    return torch.stack([g.sum(0), (g * ((x - mean.double()) * invstd.double())).sum(0)])


def exact_headroom(ref, *operands, unit=1.0, **kw):
    """max(|a|^T |dy|) / unit: the largest absolute value any partial sum of the reduction `ref` can take on these operands, in
    units of the smallest step of its products (1 for integers, 0.5 when one operand holds halves ...). Below 2^24 every
    partial sum, in every order, is a multiple of `unit` that f32 holds exactly. A condition on the INPUTS: it is computed
    from the reference on the absolute values alone, never from a kernel's output."""
    return float(ref(*[o.abs() for o in operands], **kw).max()) / unit


# -------------------------------------------------------------------------------------------------------------- comparing
def assert_exact(got, want, geom=None):
    """torch.equal on f32. On failure: the count and first index of differing elements; for a conv weight gradient
    [k,k,Cin,Cout] with geom = (channel group, output block) also the taps, channel groups and output blocks they fall in."""
    got = got.detach().float().cpu()
    want32 = want.detach().float().cpu()
    assert bool(torch.equal(want32.double(), want.detach().double().cpu())), "reference is not exact in f32"
    assert got.shape == want32.shape, (tuple(got.shape), tuple(want32.shape))
    if torch.equal(got, want32):
        return
    bad = ~(got == want32)              # (NaN differs from everything)
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    msg = (f"{int(bad.sum())} of {bad.numel()} elements differ; first at {first}: got {float(got[first])!r}, "
           f"want {float(want32[first])!r}; NaN in {int(torch.isnan(got).sum())}; max |diff| "
           f"{float(torch.nan_to_num((got - want32).abs(), nan=float('inf'))[bad].max()):g}")
    if geom is not None and got.dim() == 4:
        cg, cb = geom
        taps = sorted({(int(i[0]), int(i[1])) for i in idx})
        groups = sorted({int(i[2]) // cg for i in idx})
        blocks = sorted({int(i[3]) // cb for i in idx})
        msg += f"; taps {taps}, channel groups (of {cg}) {groups}, output blocks (of {cb}) {blocks}"
    raise AssertionError(msg)


# ------------------------------------------------------------------------------------------------------ conv case table
# claims: what a case is in the table FOR (proven on the host through the library's *_num_parts, test_reduction_exact_host.py)
#   multi_rem  more than one split and ntiles % nparts != 0        single      nparts == 1
#   partial_cg Cin is not a multiple of the channel group           partial_cb  Cout is not a multiple of the output block
ConvCase = namedtuple("ConvCase", "name N H W Cin Cout k dtypes acts claims")
B16, ALL = ("bf16", "fp16"), ("bf16", "fp16", "f32")


def _c(name, N, H, W, Cin, Cout, k, dtypes, acts, *claims):
    return ConvCase(name, N, H, W, Cin, Cout, k, dtypes, acts, frozenset(claims))


CONV_CASES = [
    # wide 3x3 (16-bit: Cout > 64; channel group 64, output block 128)
    _c("wide-128to128-588tiles", 6, 112, 112, 128, 128, 3, B16, (1,), "multi_rem"),
    _c("wide-64to256-ragged", 3, 45, 35, 64, 256, 3, B16, (2,), "multi_rem"),
    _c("wide-128to192", 1, 24, 40, 128, 192, 3, B16, (0,), "multi_rem", "partial_cb"),
    _c("wide-40to72", 2, 17, 40, 40, 72, 3, B16, (0, 1, 2), "multi_rem", "partial_cg", "partial_cb"),
    _c("wide-64to640", 1, 20, 20, 64, 640, 3, B16, (1,), "single"),
    # narrow 3x3 (16-bit: Cout <= 64; channel group 128, output block 64)
    _c("narrow-64to64-tower", 2, 50, 38, 64, 64, 3, B16, (0, 1, 2), "multi_rem", "partial_cg"),
    _c("narrow-128to64", 1, 16, 16, 128, 64, 3, B16, (2,), "single"),
    _c("narrow-256to64", 2, 33, 17, 256, 64, 3, B16, (1,)),
    _c("narrow-512to64-640tiles", 5, 128, 128, 512, 64, 3, B16, (2,)),
    _c("narrow-64to24", 2, 20, 20, 64, 24, 3, B16, (1,), "partial_cb"),
    _c("narrow-64to8", 1, 9, 7, 64, 8, 3, ALL, (2,), "single"),
    _c("narrow-40to24", 1, 19, 21, 40, 24, 3, ALL, (0, 1, 2), "partial_cg", "partial_cb"),
    # general 1x1 (16-bit: channel group 128, output block 128)
    _c("pw-256to512-576tiles", 8, 96, 96, 256, 512, 1, B16, (2,)),
    _c("pw-256to256-ragged", 9, 85, 83, 256, 256, 1, B16, (1,), "multi_rem"),
    _c("pw-136to200", 2, 37, 37, 136, 200, 1, B16, (0, 1, 2), "multi_rem", "partial_cg", "partial_cb"),
    _c("pw-32to128", 2, 16, 24, 32, 128, 1, B16, (2,), "single", "partial_cg"),
    _c("pw-48to96", 1, 37, 29, 48, 96, 1, B16, (2,), "multi_rem", "partial_cg", "partial_cb"),
    _c("pw-96to192", 2, 24, 24, 96, 192, 1, B16, (1,), "partial_cg", "partial_cb"),
    _c("pw-1024to1024", 4, 32, 33, 1024, 1024, 1, B16, (2,), "multi_rem"),
    _c("pw-64to128-128px", 1, 8, 16, 64, 128, 1, ALL, (2,), "single"),
    _c("pw-64to128-129px", 1, 3, 43, 64, 128, 1, ALL, (1,), "single"),
    # thin 1x1 (16-bit: Cin <= 32 and Cout <= 64; tile 32 x 64)
    _c("thin-32to64", 2, 61, 47, 32, 64, 1, B16, (0, 1, 2), "multi_rem"),
    _c("thin-16to32", 2, 61, 47, 16, 32, 1, B16, (2,), "multi_rem", "partial_cg", "partial_cb"),
    _c("thin-24to48", 2, 61, 47, 24, 48, 1, B16, (2,), "multi_rem", "partial_cg", "partial_cb"),
    _c("thin-8to16", 2, 61, 47, 8, 16, 1, B16, (1,), "multi_rem", "partial_cg", "partial_cb"),
    _c("thin-32to64-1tile", 1, 10, 6, 32, 64, 1, B16, (2,), "single"),
    _c("thin-16to32-1tile", 1, 10, 6, 16, 32, 1, B16, (1,), "single"),
    _c("thin-24to48-1tile", 1, 10, 6, 24, 48, 1, B16, (0,), "single"),
    _c("thin-8to16-1tile", 1, 10, 6, 8, 16, 1, B16, (2,), "single"),
    # f32 (3x3 narrow: Cout <= 32, group 32 / block 32; 3x3 wide: group 16 / block 64; 1x1: group 64 / block 64)
    _c("f32-narrow-64to24-300tiles", 3, 80, 150, 64, 24, 3, ("f32",), (2,), "multi_rem", "partial_cb"),
    _c("f32-wide-40to72-126tiles", 2, 50, 130, 40, 72, 3, ("f32",), (1,), "multi_rem", "partial_cg", "partial_cb"),
    _c("f32-pw-136to200-45tiles", 2, 61, 47, 136, 200, 1, ("f32",), (2,), "multi_rem", "partial_cg", "partial_cb"),
    # maps smaller than any tile
    _c("edge-128to128-1x1x1", 1, 1, 1, 128, 128, 3, ALL, (1,), "single"),
    _c("edge-128to128-1x3x5", 1, 3, 5, 128, 128, 3, ALL, (2,), "single"),
    _c("edge-64to64-1x1x1", 1, 1, 1, 64, 64, 3, ALL, (2,), "single"),
    _c("edge-64to64-1x3x5", 1, 3, 5, 64, 64, 3, ALL, (0,), "single"),
    _c("edge-64to24-1x3x5", 1, 3, 5, 64, 24, 3, ALL, (1,), "single", "partial_cb"),
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}

# grouped launches (16-bit): (name, N, Cin, Cout, k, act, [(H, W) per level]); every table ends in a level of a single tile
GROUPED_CASES = [
    ("wide-128to128-4levels", 1, 128, 128, 3, 1, [(80, 96), (40, 48), (20, 24), (8, 16)]),
    ("narrow-64to64-5levels", 1, 64, 64, 3, 2, [(100, 76), (50, 38), (25, 19), (13, 10), (7, 5)]),
    ("wide-40to72-2levels", 1, 40, 72, 3, 0, [(34, 40), (8, 16)]),
    ("pw-256to128-4levels", 8, 256, 128, 1, 2, [(80, 96), (40, 48), (20, 24), (2, 4)]),
    ("pw-136to200-3levels", 2, 136, 200, 1, 1, [(37, 37), (19, 19), (8, 8)]),
    ("thin-16to32-3levels", 2, 16, 32, 1, 2, [(61, 47), (31, 24), (8, 8)]),
]


def geometry(k, Cin, Cout, dtype):
    """(name, channel group, output block) of the weight-gradient kernel a shape is dispatched to: the geometries of
    csrc/conv_wgrad.hip restated (16-bit storage: four; f32: three)."""
    if dtype == "f32":
        if k == 3 and Cout <= 32:
            return "f32-narrow3x3", 32, 32
        return ("f32-wide3x3", 16, 64) if k == 3 else ("f32-1x1", 64, 64)
    if k == 1 and Cin <= 32 and Cout <= 64:
        return "thin1x1", 32, 64
    if k == 1:
        return "general1x1", 128, 128
    return ("narrow3x3", 128, 64) if Cout <= 64 else ("wide3x3", 64, 128)


def ntiles(N, H, W, k):
    """Pixel tiles the splits of a weight gradient walk: 8 x 16 pixels per image (3x3), 128 consecutive pixels (1x1)."""
    return N * (-(-H // 8)) * (-(-W // 16)) if k == 3 else -(-(N * H * W) // 128)


ConvData = namedtuple("ConvData", "x dy scale shift want headroom")


@lru_cache(maxsize=3)
def conv_case_data(name, act, N=None, H=None, W=None, Cin=None, Cout=None, k=None):
    """Inputs (integer-valued f32 CPU tensors), the float64 reference dW and the headroom of one conv case and activation.
    Cached: the storage types share the values (all exactly representable), so one reference serves them all."""
    if N is None:
        c = CONV_BY_NAME[name]
        N, H, W, Cin, Cout, k = c.N, c.H, c.W, c.Cin, c.Cout, c.k
    rs = np.random.RandomState((hash_name(name) + 7 * act) % (2 ** 31))
    scale, shift = int_affine(rs, Cin)
    x = int_activations(rs, (N, H, W, Cin), scale)
    dy = int_tensor(rs, (N, H, W, Cout), -DY_MAX, DY_MAX)
    a = act_affine(x, scale, shift, act)
    want = conv_wgrad_ref(a, dy, k)
    return ConvData(x, dy, scale, shift, want, exact_headroom(conv_wgrad_ref, a, dy, ksize=k))


def hash_name(name):
    """A stable seed from a case name (Python's hash() is salted per process)."""
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


# ------------------------------------------------------------------------------------------- the other reductions' tables
def _rs(*key):
    return np.random.RandomState(hash_name(repr(key)) % (2 ** 31))


FUSED1X1_CASES = [(2, 61, 47, 32, 64, 2), (1, 37, 29, 16, 32, 1), (1, 64, 64, 24, 48, 2), (3, 40, 40, 64, 128, 1), (2, 24, 24, 128, 128, 2),
                  (1, 10, 6, 32, 64, 2)]          # N, H, W, Cin, Cout, activation of the batch-norm below
W_NONZERO = 8                                     # nonzero weights per input channel: |dx| <= 8 * max |dy|


@lru_cache(maxsize=2)
def fused1x1_case_data(N, H, W, Cin, Cout, act, apply):
    """mpn_conv1x1_bwd_fused[_apply] on integers. Weights in {-1, 0, 1} with W_NONZERO nonzeros per input channel, so the data
    gradient stays an integer of magnitude <= 256 (exact in bf16). apply: the layer's own batch-norm apply
    dY = s * (g_masked - k1 - (y - mean) * invstd * k2) with s in {1, 2}, integer shift / mean / k1, invstd in {0.5, 1} and
    k2 in {-2, 0, 2} - every term an integer, |dY| <= 26."""
    rs = _rs("fused", N, H, W, Cin, Cout, act, apply)
    scale, shift = int_affine(rs, Cin)
    x = int_activations(rs, (N, H, W, Cin), scale)
    w = torch.zeros(Cin, Cout)
    for ci in range(Cin):
        cols = rs.choice(Cout, size=W_NONZERO, replace=False)
        w[ci, cols] = torch.from_numpy(rs.choice(np.array([-1.0, 1.0], np.float32), size=W_NONZERO))
    d = {"x": x, "scale": scale, "shift": shift, "w": w.reshape(1, 1, Cin, Cout)}
    if apply:
        g = int_tensor(rs, (N, H, W, Cout), -2, 2)
        y = int_tensor(rs, (N, H, W, Cout), -4, 4)
        ap = {"scale": torch.from_numpy(rs.choice(np.array([1.0, 2.0], np.float32), size=Cout)), "shift": int_tensor(rs, (Cout,), -2, 2),
              "mean": int_tensor(rs, (Cout,), -1, 1), "invstd": torch.from_numpy(rs.choice(np.array([0.5, 1.0], np.float32), size=Cout)),
              "k1": int_tensor(rs, (Cout,), -1, 1), "k2": 2.0 * int_tensor(rs, (Cout,), -1, 1)}
        pre = y.double() * ap["scale"].double() + ap["shift"].double()
        gm = torch.where((pre > 0) & (pre < 6), g.double(), torch.zeros(1, dtype=torch.float64))
        dy = ap["scale"].double() * (gm - ap["k1"].double() - (y.double() - ap["mean"].double()) * ap["invstd"].double() * ap["k2"].double())
        assert bool((dy == dy.round()).all()) and representable16(dy)
        d.update(g=g, y=y, ap=ap)
    else:
        dy = int_tensor(rs, (N, H, W, Cout), -DY_MAX, DY_MAX).double()
    a = act_affine(x, scale, shift, act)
    d["dy"] = dy.float()
    d["want_dw"] = conv_wgrad_ref(a, dy, 1)
    d["headroom"] = exact_headroom(conv_wgrad_ref, a, dy, ksize=1)
    dx = dy.reshape(-1, Cout) @ w.double().t()
    pre = (x.double() * scale.double() + shift.double()).reshape(-1, Cin)
    ok = torch.ones_like(pre, dtype=torch.bool)
    if act != ACT_NONE:
        ok = pre > 0
    if act == ACT_RELU6:
        ok = ok & (pre < 6)
    d["want_dx"] = torch.where(ok, dx, torch.zeros_like(dx)).reshape(N, H, W, Cin)
    d["dx_bound"] = float(dx.abs().max())                      # must be <= 256: then dx is exact in bf16
    d["bn_headroom"] = float((d["want_dx"].abs().reshape(-1, Cin) * x.double().abs().reshape(-1, Cin)).sum(0).max())
    return d


# depthwise: the odd shapes of test_ops_bwd_gpu.py::test_dwconv_backward + strips of 64 rows, many channel blocks, one pixel, two rows
DW_CASES = [(1, 9, 7, 64), (2, 5, 13, 32), (1, 70, 33, 128), (1, 14, 10, 256), (1, 130, 70, 32), (2, 64, 64, 128), (1, 1, 1, 64),
            (1, 2, 37, 32), (1, 12, 20, 128)]


@lru_cache(maxsize=2)
def dw_case_data(N, H, W, C, stride):
    rs = _rs("dw", N, H, W, C, stride)
    scale, shift = int_affine(rs, C)
    x = int_activations(rs, (N, H, W, C), scale)
    dy = int_tensor(rs, (N, tf_same(H, stride)[0], tf_same(W, stride)[0], C), -DY_MAX, DY_MAX)
    a = act_affine(x, scale, shift, ACT_RELU6)
    return {"x": x, "dy": dy, "scale": scale, "shift": shift, "want": dwconv_wgrad_ref(a, dy, stride),
            "headroom": exact_headroom(dwconv_wgrad_ref, a, dy, stride=stride)}


STEM_MAPS = [(3, 128, 128), (1, 30, 34), (1, 17, 9)]
STEM_C0 = [16, 32, 64]


@lru_cache(maxsize=2)
def stem_case_data(N, H, W, C0):
    """Images in {0, 0.5, 1}: 2 * image - 1 is in {-1, 0, 1} (the matrix-core kernel's bf16 hi / lo split has a zero low part)."""
    rs = _rs("stem", N, H, W, C0)
    img = int_tensor(rs, (N, H, W, 3), 0, 2) * 0.5
    dy = int_tensor(rs, (N, (H + 1) // 2, (W + 1) // 2, C0), -DY_MAX, DY_MAX)
    return {"img": img, "dy": dy, "want": stem_wgrad_ref(img, dy),
            "headroom": exact_headroom(conv_wgrad_ref, 2.0 * img.double() - 1.0, dy, ksize=3, stride=2)}


HEAD_M = [640, 1000, 128 * 300 + 77]
HEAD_C = [16, 32, 64]


@lru_cache(maxsize=2)
def head_case_data(M, C):
    rs = _rs("head", M, C)
    scale, shift = int_affine(rs, C)
    x = int_activations(rs, (1, 1, M, C), scale)
    dl = int_tensor(rs, (1, 1, M, 18), -DY_MAX, DY_MAX)
    a = act_affine(x, scale, shift, ACT_RELU)
    return {"x": x, "dl": dl, "scale": scale, "shift": shift, "want": head_ref(a, dl), "headroom": exact_headroom(head_ref, a, dl)}


GEMM_CASES = [(128, 1024, 34272), (24, 256, 2056), (130, 132, 72), (8, 4, 8)]     # test_prn_gpu.py::test_gemm_nt_split_k


@lru_cache(maxsize=2)
def gemm_case_data(M, N, K):
    """|a|, |b| <= 3: at K = 34 272 no sum exceeds 9 * 34 272 = 308 448."""
    rs = _rs("gemm", M, N, K)
    a, b = int_tensor(rs, (M, K), -3, 3), int_tensor(rs, (N, K), -3, 3)
    return {"a": a, "b": b, "want": gemm_nt_ref(a, b), "headroom": exact_headroom(gemm_nt_ref, a, b)}


BN_M = [777, 4096, 50000, 300001]     # 300 001 rows: mpn_bn_stats_num_parts is at its 2048 blocks, 147 rows per block (> 128)
BN_C = [8, 24, 64, 1024]
BN_MAX_ELEMENTS = 64 << 20           # 300 001 x 1024 would be 1.2 GB per f32 tensor (the 2048-block grid does not depend on C)
BN_MC = [(M, C) for M in BN_M for C in BN_C if M * C <= BN_MAX_ELEMENTS]
# |x| <= 8 (16 where the scale is 0.5) puts sum x^2 of a doubled channel at about 96 M = 28.8 M > 2^24 for M = 300 001. With
# |x| <= 4 (8) for that M the generated data has sum x^2 <= 8.1 M and sum |g| |xhat| / 0.5 <= 13.3 M < 2^24 = 16.8 M
# (tests/test_reduction_exact_host.py asserts it); x * scale + shift still spans [-7, 7]: 0.55 of it <= 0, 0.1 of it >= 6
BN_X_MAX = {300001: 4}


@lru_cache(maxsize=2)
def bn_case_data(M, C, act):
    """Integer mean in [-2, 2], invstd in {0.5, 1, 2}: xhat is a multiple of 0.5 and so is every product g * xhat."""
    rs = _rs("bn", M, C, act)
    scale, shift = int_affine(rs, C)
    x = int_activations(rs, (M, C), scale, BN_X_MAX.get(M, X_MAX))
    dA = int_tensor(rs, (M, C), -DY_MAX, DY_MAX)
    mean = int_tensor(rs, (C,), -2, 2)
    invstd = torch.from_numpy(rs.choice(np.array([0.5, 1.0, 2.0], np.float32), size=C))
    assert representable16(x) and representable16(dA)
    xhat_abs = (x.double().abs() + mean.double().abs()) * invstd.double()
    return {"x": x, "dA": dA, "scale": scale, "shift": shift, "mean": mean, "invstd": invstd,
            "want_stats": stats_ref(x), "want_bwd": bn_bwd_sums_ref(dA, x, scale, shift, mean, invstd, act),
            "headroom": max(float(stats_ref(x).max()), float((dA.double().abs() * xhat_abs).sum(0).max()) / 0.5)}
