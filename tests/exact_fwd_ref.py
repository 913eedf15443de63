"""Exact-integer inputs and references for the dense convolution's forward pass, its data gradient and their fused epilogues
(statistics rows, upsample-add, the batch-norm reduction behind a data gradient): the sibling of tests/exact_ref.py.

The kernels form f32 sums of products of storage-typed operands and round ONCE, at the store. With integer operands whose
absolute sums stay below 2^24 (`exact_headroom`) every partial sum is exact in f32 in any order, so the only rounding a correct
kernel performs is that store and its output is `reference_f64.float().to(dtype)`, bit for bit. Two data regimes:

  narrow  every output |y| <= 256 (exact in bf16 and fp16) and, per channel, sum |y| and sum y^2 below 2^24: output, statistics
          rows and fused-reduction rows are all exact. The limits are reached by THINNING the activations (more zeros); every
          weight is nonzero and every input channel is nonzero at some pixel under every tap.
  wide    outputs grow past what the storage type holds exactly (at least 5 % of them are not representable in it): a partial
          sum rounded to 16 bits on the way, a residual added after the rounding or statistics taken before it change bits.
          Where the map is small enough that sum y_r^2 of the ROUNDED outputs stays below 2^24 the statistics are compared too.

All conditions are conditions on the INPUTS: they are computed from the float64 references (on absolute values for the headroom),
never from a kernel's output, and asserted case by case in tests/test_forward_exact_host.py. References are float64, written as
shifted slices and matrix products; they do not go through oracle.network (the host test checks them against it).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

import exact_ref as E
from exact_ref import ACT_NONE, ACT_RELU6, EXACT_LIMIT

Y_MAX = 256.0                 # integers up to 256 are exact in bf16 (8 significant bits) and fp16 (11)
MIN_WIDE_SHARE = 0.05         # wide regime: at least this share of the outputs is not representable in the storage type
RES_MAX = 20                  # |residual| of the upsample-add cases
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}


# ------------------------------------------------------------------------------------------------------------ references
def conv_fwd_ref(a, w, k):
    """The SAME convolution of the network's layers (stride 1): y[n,y,x,co] = sum over taps and ci of
    a_pad[n, y + ty - 1, x + tx - 1, ci] * w[ty,tx,ci,co] (3x3; zero padding of one pixel) or a @ w (1x1). a [N,H,W,Cin],
    w [k,k,Cin,Cout]; float64 [N,H,W,Cout]."""
    a, w = a.double(), w.double()
    N, H, W, Cin = a.shape
    Cout = w.shape[3]
    if k == 1:
        return (a.reshape(-1, Cin) @ w[0, 0]).reshape(N, H, W, Cout)
    y = torch.zeros(N * H * W, Cout, dtype=torch.float64)
    for ty, tx, v in E._taps(a, H, W, 1):
        y += v.reshape(-1, Cin) @ w[ty, tx]
    return y.reshape(N, H, W, Cout)


def conv_dgrad_ref(dy, w, k):
    """The data gradient of conv_fwd_ref: dx[n,y,x,ci] = sum over taps and co of dy_pad[n, y - (ty - 1), x - (tx - 1), co] *
    w[ty,tx,ci,co]. dy [N,H,W,Cout], w [k,k,Cin,Cout] (the FORWARD layer's weights); float64 [N,H,W,Cin]."""
    dy, w = dy.double(), w.double()
    N, H, W, Cout = dy.shape
    Cin = w.shape[2]
    if k == 1:
        return (dy.reshape(-1, Cout) @ w[0, 0].t()).reshape(N, H, W, Cin)
    dx = torch.zeros(N * H * W, Cin, dtype=torch.float64)
    for sy, sx, v in E._taps(dy, H, W, 1):          # v[y, x] = dy_pad[y + sy - 1, x + sx - 1]: the tap (2 - sy, 2 - sx)
        dx += v.reshape(-1, Cout) @ w[2 - sy, 2 - sx].t()
    return dx.reshape(N, H, W, Cin)


def upsample2_ref(res):
    """Nearest-neighbour 2x of [N,h,w,C]: out[n, y, x] = res[n, y // 2, x // 2]."""
    return res.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def upsample_add_ref(a, w, res):
    """conv1x1(a) + nearest-2x(res), added in float64: the kernel's epilogue adds the residual into its f32 accumulators, so the
    one rounding of the store is the rounding of THIS sum."""
    return conv_fwd_ref(a, w, 1) + upsample2_ref(res.double())


def once_rounded(ref, dt):
    """The expected tensor of a kernel that rounds once: float64 -> f32 (exact below 2^24) -> the storage type, as float64."""
    return ref.float().to(TORCH_DT[dt]).double()


def share_not_representable(ref, dt):
    """Share of the elements of a float64 reference that the storage type does not hold exactly."""
    return float((once_rounded(ref, dt) != ref).double().mean())


def act_mask(x, scale, shift, act):
    """Where the derivative of act(x * scale + shift) is 1: everywhere (none), pre > 0 (ReLU), 0 < pre < 6 (ReLU6)."""
    pre = x.double() * scale.double() + shift.double()
    ok = torch.ones_like(pre, dtype=torch.bool)
    if act != ACT_NONE:
        ok = pre > 0
    if act == ACT_RELU6:
        ok = ok & (pre < 6)
    return ok


def bwd_data_bn_ref(dx, x, scale, shift, act):
    """What mpn_conv_bwd_data_bn leaves behind a data gradient dx [N,H,W,C] that feeds the batch-norm layer with raw input x:
    g = dx where the layer's activation passes (act_mask of x * scale + shift), else 0, and the rows [2][C] = sum g and
    sum g * x over the pixels - the RAW x (the finalize forms sum g * xhat from them). Returns (g, rows), float64."""
    C = x.shape[-1]
    g = torch.where(act_mask(x, scale, shift, act), dx.double(), torch.zeros(1, dtype=torch.float64))
    g2, x2 = g.reshape(-1, C), x.double().reshape(-1, C)
    return g, torch.stack([g2.sum(0), (g2 * x2).sum(0)])


def stats_headroom(y):
    """max over channels of sum |y| and of sum y^2: below 2^24 every partial sum of a statistics row is an exact f32."""
    y = y.double().reshape(-1, y.shape[-1])
    return float(max(y.abs().sum(0).max(), (y * y).sum(0).max()))


# --------------------------------------------------------------------------------------------------------------- routing
def conv_route(k, Kin, Nout, dt):
    """(route, packed bytes) of a dense convolution Kin -> Nout: the launcher's routing (pack_geom in csrc/conv_mfma.hip, with
    pw_gemm_eligible of pointwise.hip and eligible / eligible64 of conv3x3.h) restated.
      gemm          bf16 1x1, 256 <= Kin <= 2048, Kin % 64 == 0, Nout % 256 == 0: weights as a plain [Nout][Kin] matrix
      c3            16-bit 3x3, Kin % 64 == 0, Kin <= 512, Nout % 128 == 0: the persistent kernel, 9 * Kin * Nout * 2 bytes
      c3-64         ... Nout % 128 == 64: its 64-channel-tile variant, the same bytes
      tiled<k>-<rb> everything else (all of f32): n-tiles of 128 (Nout % 128 == 0) or 64 channels, K rows of rb = 256 bytes for
                    1x1 layers with at least 1024 bytes of K, else 128; chunks * taps * (rb / 128) * 2 * BN * 64 bytes per n-tile"""
    es = 4 if dt == "f32" else 2
    if dt == "bf16" and k == 1 and 256 <= Kin <= 2048 and Kin % 64 == 0 and Nout % 256 == 0:
        return "gemm", Nout * Kin * 2
    if es == 2 and k == 3 and Kin % 64 == 0 and Kin <= 512 and Nout % 128 in (0, 64):
        return ("c3" if Nout % 128 == 0 else "c3-64"), 9 * Kin * Nout * 2
    bn = 128 if Nout % 128 == 0 else 64
    n_tiles = -(-Nout // bn)
    kbytes = Kin * es
    rb = 256 if (k == 1 and kbytes >= 1024) else 128
    nchunk = -(-kbytes // rb)
    return f"tiled{k}-{rb}", nchunk * k * k * (rb // 128) * 2 * bn * 64 * n_tiles


def gemm_pixel_tile(M, Nout):
    """Pixels per block of the GEMM kernel (pw_gemm_launch in pointwise.hip): 256 when the 256-pixel tiles still give each of
    256 compute units a block (ceil(M / 256) * Nout / 256 >= 256), else 128."""
    return 256 if -(-M // 256) * (Nout // 256) >= 256 else 128


# ------------------------------------------------------------------------------------------------------------ generators
def _weights(rs, k, Kin, Nout, m):
    """Integer weights, every element nonzero: magnitudes uniform in [1, m], signs balanced over the input channels of every
    (tap, output channel) column so that the (non-negative) activations' mean does not pile up in one output channel."""
    mag = rs.randint(1, m + 1, size=(k, k, Kin, Nout)).astype(np.float32)
    order = np.argsort(rs.rand(k, k, Kin, Nout), axis=2)
    sign = np.where(order < Kin // 2, -1.0, 1.0).astype(np.float32)
    return torch.from_numpy(mag * sign)


def _mean_w2(m):
    return (m + 1) * (2 * m + 1) / 6.0


def _thin(rs, x, a0, scale, shift, keep, k):
    """x with all but a share `keep` of its elements moved to where the activation is 0 (the most negative input of its channel;
    0 when there is no affine) - but one element per channel, nonzero after the activation and off the map's border (so that
    every tap reads it), always stays."""
    N, H, W, C = x.shape
    mask = torch.from_numpy(rs.rand(N, H, W, C) < keep)
    inner = torch.ones(N, H, W, 1, dtype=torch.bool)
    if k == 3 and H >= 3 and W >= 3:
        inner[:] = False
        inner[:, 1:H - 1, 1:W - 1] = True
    # the element that stays: a random inner one, among those that are nonzero where the channel has any
    score = (torch.from_numpy(rs.rand(N, H, W, C)) + (a0 != 0)) * inner
    pick, ch = score.reshape(-1, C).argmax(0), torch.arange(C)
    mask.reshape(-1, C)[pick, ch] = True
    if scale is None:
        off, on = torch.zeros(C), torch.ones(C)
    else:
        off = -E.X_MAX * torch.where(scale == 0.5, 2.0, 1.0)
        # (a channel that is zero on all inner pixels gets x * scale + shift = 4, or 4 + shift where the scale is 2, there)
        on = torch.where(scale == 0.5, 2.0 * (4.0 - shift), torch.where(scale == 1.0, 4.0 - shift, torch.full((C,), 2.0)))
    x = x.clone()
    dead = a0.reshape(-1, C)[pick, ch] == 0
    x.reshape(-1, C)[pick[dead], ch[dead]] = on[dead]
    return torch.where(mask, x, off.expand_as(x))


ConvData = namedtuple("ConvData", "x scale shift act a w res want headroom keep wmax")


def _generate(seed, N, H, W, Kin, Nout, k, act, sigma, wmax_cap, res, accept, shrink=0.8):
    """Inputs of one convolution whose outputs have a standard deviation of about `sigma`: the smallest weight magnitude bound
    (up to wmax_cap) that reaches it on the dense activations, then thinned activations to come down to it. `accept(want)` judges
    the reference (the regime's conditions on the inputs); while it says no, sigma shrinks by the factor `shrink` (and the seed
    changes) - at most 12 times."""
    for attempt in range(12):
        rs = np.random.RandomState((E.hash_name(seed) + 1009 * attempt) % (2 ** 31))
        if act == ACT_NONE:      # no affine at all (the data-gradient configuration)
            scale = shift = None
            x = E.int_tensor(rs, (N, H, W, Kin), -E.DY_MAX, E.DY_MAX)
            a0 = x.double()
        else:
            scale, shift = E.int_affine(rs, Kin)
            x = E.int_activations(rs, (N, H, W, Kin), scale)
            a0 = E.act_affine(x, scale, shift, act)
        unit = k * k * Kin * float((a0 * a0).mean())          # the outputs' variance with weights of mean square 1, dense
        wmax = 1
        while wmax < wmax_cap and unit * _mean_w2(wmax) < sigma * sigma:
            wmax += 1 if wmax < 8 else wmax // 8
        wmax = min(wmax, wmax_cap)
        keep = min(1.0, sigma * sigma / (unit * _mean_w2(wmax)))
        x = _thin(rs, x, a0, scale, shift, keep, k)
        a = x.double() if scale is None else E.act_affine(x, scale, shift, act)
        w = _weights(rs, k, Kin, Nout, wmax)
        want = conv_fwd_ref(a, w, k)
        headroom = E.exact_headroom(conv_fwd_ref, a, w, k=k)
        r = None
        if res:
            r = E.int_tensor(rs, (N, H // 2, W // 2, Nout), -RES_MAX, RES_MAX)
            want = want + upsample2_ref(r.double())
            headroom += RES_MAX
        if accept(want):
            break
        sigma *= shrink
    return ConvData(x, scale, shift, act, a, w, r, want, headroom, keep, wmax)


WIDE_STATS_MAX_PIXELS = 330   # wide regime: above this no sigma gives both 5 % of unrepresentable outputs and sum y_r^2 < 2^24
WIDE_SIGMA = {"bf16": 1500.0, "fp16": 12000.0}     # outputs far past 256 (bf16) / 2048 (fp16) where no statistics are compared
WIDE_WMAX = {"bf16": 120, "fp16": 1000}            # |w| <= 256 is exact in bf16, <= 2048 in fp16


def narrow_ok(want):
    return float(want.abs().max()) <= Y_MAX and stats_headroom(want) < EXACT_LIMIT


def narrow_data(seed, N, H, W, Kin, Nout, k, act):
    """Narrow regime: sigma of at most 40 (5.5 sigma of the about 10^7 outputs of the largest cases stay below 256), less where
    the map has so many pixels that sum y^2 per channel would pass 2^24. Weights in +-[1, 3] at most."""
    M = N * H * W
    sigma = min(40.0, (0.6 * EXACT_LIMIT / M) ** 0.5)
    return _generate(f"narrow/{seed}", N, H, W, Kin, Nout, k, act, sigma, 3, False, narrow_ok)


def wide_data(seed, N, H, W, Kin, Nout, k, act, dt, with_stats, res=False):
    """Wide regime for one storage type. with_stats: sigma as large as sum y_r^2 < 2^24 allows on this map (at most 400)."""
    M = N * H * W

    def ok(want):
        if share_not_representable(want, dt) < MIN_WIDE_SHARE:
            return False
        return not with_stats or stats_headroom(once_rounded(want, dt)) < EXACT_LIMIT

    # (with statistics the window is narrow at 256 pixels: small steps down from a sigma that is rather too large)
    sigma = min(400.0, (0.75 * EXACT_LIMIT / M) ** 0.5) if with_stats else WIDE_SIGMA[dt]
    return _generate(f"wide/{dt}/{int(with_stats)}/{seed}", N, H, W, Kin, Nout, k, act, sigma, WIDE_WMAX[dt], res, ok, shrink=0.96)


# ------------------------------------------------------------------------------------------------------------ case tables
# route: the kernel a case is in the table FOR (conv_route; proven on the host through mpn_conv_packed_bytes as far as the packed
#        size tells the routes apart, test_forward_exact_host.py).   act: 0 = no producer affine, 1 = ReLU, 2 = ReLU6.
# stats: the statistics rows are compared (narrow regime: always exact).   wide_stats: ... in the wide regime too, bf16 only:
#        the map has at most WIDE_STATS_MAX_PIXELS pixels. False where sum y_r^2 < 2^24 cannot be met together with the 5 % share
#        (larger maps; fp16, whose unrepresentable integers start at 2048).
# f32 runs the narrow regime only: every integer below 2^24 is representable, so there is nothing for the wide regime to see.
FwdCase = namedtuple("FwdCase", "name N H W Cin Cout k dtypes act route stats wide_stats regimes")
B16, ALL, BF = ("bf16", "fp16"), ("bf16", "fp16", "f32"), ("bf16",)
BOTH = ("narrow", "wide")


def _f(name, N, H, W, Cin, Cout, k, dtypes, act, route, stats=True, wide_stats=False, regimes=BOTH):
    return FwdCase(name, N, H, W, Cin, Cout, k, dtypes, act, route, stats, wide_stats, regimes)


FWD_CASES = [
    # tiled 1x1, 128-byte K rows
    _f("t1-64to128", 2, 16, 16, 64, 128, 1, ALL, 2, "tiled1-128"),                       # 512 pixels: no wide statistics
    _f("t1-32to64-ragged", 1, 10, 6, 32, 64, 1, B16, 2, "tiled1-128", wide_stats=True),  # a ragged single tile, BN 64
    _f("t1-136to200", 2, 6, 10, 136, 200, 1, B16, 1, "tiled1-128", wide_stats=True),     # partial K chunk, partial n-tile, XCD remap
    # tiled 1x1, 256-byte K rows
    _f("t2-512to128", 1, 8, 8, 512, 128, 1, ALL, 2, "tiled1-256", wide_stats=True),
    _f("t2-512to512-fp16", 2, 16, 16, 512, 512, 1, ("fp16",), 2, "tiled1-256"),          # fp16 never takes the GEMM route
    # tiled 3x3
    _f("t3-40to72", 1, 10, 14, 40, 72, 3, B16, 1, "tiled3-128", wide_stats=True),
    _f("t3-32to64", 1, 12, 20, 32, 64, 3, B16, 2, "tiled3-128", wide_stats=True),
    _f("t3-128to128-f32", 1, 4, 4, 128, 128, 3, ("f32",), 1, "tiled3-128"),
    # the persistent 3x3 kernel
    _f("c3-128to128", 2, 16, 16, 128, 128, 3, B16, 1, "c3"),                             # 512 pixels: no wide statistics
    _f("c3-64to256-ragged", 1, 20, 36, 64, 256, 3, B16, 2, "c3"),                        # a ragged 16x16 tile; 720 pixels
    _f("c3-256to128", 1, 16, 16, 256, 128, 3, B16, 0, "c3", wide_stats=True),            # four chunks
    _f("c3-128to128-294tiles", 6, 112, 112, 128, 128, 3, BF, 1, "c3", regimes=("narrow",)),   # more tiles than compute units
    # its 64-channel-tile variant
    _f("cs-64to64", 2, 50, 38, 64, 64, 3, B16, 1, "c3-64"),                              # 3800 pixels
    _f("cs-512to64", 1, 16, 16, 512, 64, 3, B16, 2, "c3-64", wide_stats=True),           # 8 chunks: the deepest cross-wave sum
    _f("cs-128to192", 1, 24, 40, 128, 192, 3, B16, 2, "c3-64"),                          # 960 pixels
    # the bf16 GEMM kernel
    _f("g-256to256-143px", 1, 13, 11, 256, 256, 1, BF, 1, "gemm", wide_stats=True),      # a partial statistics row
    _f("g-512to512", 2, 16, 16, 512, 512, 1, BF, 2, "gemm"),                             # 512 pixels
    _f("g-320to512-affine", 1, 9, 15, 320, 512, 1, BF, 2, "gemm", wide_stats=True),      # five k-steps
    _f("g-320to512-dma", 1, 9, 15, 320, 512, 1, BF, 0, "gemm", wide_stats=True),         # ... no affine: the LDS-DMA A path
    _f("g-256to1024-256px-tiles", 1, 127, 127, 256, 1024, 1, BF, 1, "gemm"),             # 16 129 pixels: the first M on 256-pixel tiles
]
FWD_BY_NAME = {c.name: c for c in FWD_CASES}

# upsample-add epilogue (tiled 1x1): wide data only - the expectation rounds conv + up(res) once. No statistics (the network's
# laterals take none).
UP_CASES = [
    _f("u-256to128", 2, 16, 16, 256, 128, 1, B16, 2, "tiled1-128", stats=False, regimes=("wide",)),   # W < 32: the direct epilogue
    _f("u-128to128", 1, 32, 32, 128, 128, 1, B16, 2, "tiled1-128", stats=False, regimes=("wide",)),
    _f("u-64to128", 3, 10, 40, 64, 128, 1, B16, 1, "tiled1-128", stats=False, regimes=("wide",)),     # tiles cross an image boundary
]
UP_BY_NAME = {c.name: c for c in UP_CASES}

# data gradients through PackedConv.bwd: (k, Cin, Cout) of the FORWARD layer - the gradient runs Cout -> Cin -, the route of that
# convolution per storage type; all at 2 x 12 x 16
DGRAD_NHW = (2, 12, 16)
DGRAD_CASES = [
    (3, 512, 64, {"bf16": "c3", "fp16": "c3"}),
    (3, 64, 64, {"bf16": "c3-64", "fp16": "c3-64"}),
    (3, 64, 192, {"bf16": "c3-64", "fp16": "c3-64"}),
    (1, 512, 1024, {"bf16": "gemm", "fp16": "tiled1-256"}),
    (1, 256, 512, {"bf16": "gemm", "fp16": "tiled1-256"}),
    (1, 256, 128, {"bf16": "tiled1-128", "fp16": "tiled1-128"}),
    (1, 64, 128, {"bf16": "tiled1-128", "fp16": "tiled1-128"}),
]

# grouped forward (bf16, narrow data, statistics): seven images of three pyramid levels that end in a one-tile level - 280 tiles of
# 16 x 16 pixels, more than the 256 compute units, so a persistent block walks from one job into the next
GROUPED_N = 7
GROUPED_HW = [(80, 96), (40, 48), (8, 16)]
GROUPED_CASES = [("grp-128to128", 128, 128, 3, 1, "c3"), ("grp-64to64", 64, 64, 3, 2, "c3-64"), ("grp-256to128", 256, 128, 1, 2, "tiled1-128")]

# mpn_conv_bwd_data_bn (narrow data, ReLU6 mask): (name, N, H, W, K, C, ksize, route of the gradient K -> C); the 3x3 ones also run
# as mpn_conv_bwd_data_bn_grouped with the sizes below
BNR_CASES = [
    ("bnr-tiled-128to64", 3, 21, 19, 128, 64, 1, "tiled1-128"),
    ("bnr-gemm-512to512", 2, 16, 16, 512, 512, 1, "gemm"),
    ("bnr-c3-128to128", 2, 20, 36, 128, 128, 3, "c3"),
    ("bnr-tiled-24to64", 2, 12, 20, 24, 64, 3, "tiled3-128"),
]
BNR_GROUPED_HW = [(37, 21), (16, 16), (9, 5)]
BNR_GROUPED_N = 2


@lru_cache(maxsize=2)
def fwd_case_data(name, regime, dt=None):
    """The data of one forward (or upsample-add) case. Narrow data is shared by the storage types (dt None: every value is exact in
    all of them); wide data is made for one storage type."""
    c = FWD_BY_NAME.get(name) or UP_BY_NAME[name]
    if regime == "narrow":
        return narrow_data(name, c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.act)
    return wide_data(name, c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.act, dt, c.stats and wide_stats_for(c, dt), res=name in UP_BY_NAME)


def wide_stats_for(c, dt):
    return c.wide_stats and dt == "bf16"


DgradData = namedtuple("DgradData", "dy w want headroom")


@lru_cache(maxsize=2)
def dgrad_case_data(k, Cin, Cout, regime, dt=None):
    """dy [N,H,W,Cout] and the forward layer's weights w [k,k,Cin,Cout]. The data is generated for the convolution the kernel
    runs (Cout -> Cin with the flipped, transposed weights); the reference is conv_dgrad_ref on the forward weights."""
    N, H, W = DGRAD_NHW
    seed = f"dgrad-{k}-{Cin}-{Cout}"
    d = narrow_data(seed, N, H, W, Cout, Cin, k, ACT_NONE) if regime == "narrow" else wide_data(seed, N, H, W, Cout, Cin, k, ACT_NONE, dt, False)
    w = d.w.flip(0, 1).transpose(2, 3).contiguous()
    return DgradData(d.x, w, conv_dgrad_ref(d.x, w, k), E.exact_headroom(conv_dgrad_ref, d.x, w, k=k))


BnrData = namedtuple("BnrData", "dy w x scale shift act dx g rows headroom rows_headroom")


@lru_cache(maxsize=4)
def bnr_case_data(seed, N, H, W, K, C, k):
    """mpn_conv_bwd_data_bn on narrow data: dy [N,H,W,K], forward weights w [k,k,C,K] (the gradient runs K -> C), the fed layer's
    raw input x with an integer affine and ReLU6 (clips at both ends). rows_headroom: max over channels of sum |g| and
    sum |g| |x|."""
    d = narrow_data(seed, N, H, W, K, C, k, ACT_NONE)
    w = d.w.flip(0, 1).transpose(2, 3).contiguous()
    rs = np.random.RandomState(E.hash_name("bnr/" + seed) % (2 ** 31))
    scale, shift = E.int_affine(rs, C)
    x = E.int_activations(rs, (N, H, W, C), scale)
    assert E.representable16(x)
    dx = conv_dgrad_ref(d.x, w, k)
    g, rows = bwd_data_bn_ref(dx, x, scale, shift, ACT_RELU6)
    g2, x2 = g.abs().reshape(-1, C), x.double().abs().reshape(-1, C)
    return BnrData(d.x, w, x, scale, shift, ACT_RELU6, dx, g, rows, E.exact_headroom(conv_dgrad_ref, d.x, w, k=k),
                   float(max(g2.sum(0).max(), (g2 * x2).sum(0).max())))
