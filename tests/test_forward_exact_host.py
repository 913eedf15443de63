"""CPU: the references of tests/exact_fwd_ref.py against the oracle, the regime conditions of every case of
tests/test_forward_exact_gpu.py (conditions on the INPUTS, from the float64 references), the proof that the instrument tells an
intermediate rounding from the single one, and the route claims of the case tables against the library's packed sizes (host code:
loads without a GPU)."""
import numpy as np
import pytest
import torch

import exact_fwd_ref as F
import exact_ref as E
from multiposenet_amd import _lib
from oracle import network as onet
from util import nchw, nhwc

CODE = {"bf16": _lib.MPN_BF16, "fp16": _lib.MPN_F16, "f32": _lib.MPN_F32}
LIMIT = E.EXACT_LIMIT


# ------------------------------------------------------------------------------------------- references against the oracle
@pytest.mark.parametrize("k,act", [(3, 0), (3, 2), (1, 1), (1, 2)])
def test_forward_and_data_gradient_references_equal_the_oracle(k, act):
    rs = np.random.RandomState(10 + k + act)
    N, H, W, Cin, Cout = 2, 7, 11, 24, 16
    scale, shift = E.int_affine(rs, Cin)
    a = E.act_affine(E.int_activations(rs, (N, H, W, Cin), scale), scale, shift, act)
    w = E.int_tensor(rs, (k, k, Cin, Cout), -3, 3).double()
    x = nchw(a).clone().requires_grad_(True)
    y = onet.conv2d_same(x, w)
    assert torch.equal(F.conv_fwd_ref(a, w, k), nhwc(y))
    dy = E.int_tensor(rs, (N, H, W, Cout), -3, 3)
    y.backward(nchw(dy.double()))
    assert torch.equal(F.conv_dgrad_ref(dy, w, k), nhwc(x.grad))
    # the data gradient IS the forward convolution of dy with the flipped, transposed weights (what PackedConv.bwd packs)
    assert torch.equal(F.conv_dgrad_ref(dy, w, k), F.conv_fwd_ref(dy, w.flip(0, 1).transpose(2, 3), k))


def test_upsample_add_statistics_and_fused_sum_references():
    rs = np.random.RandomState(3)
    N, H, W, Cin, Cout = 2, 6, 10, 16, 8
    a, w = E.int_tensor(rs, (N, H, W, Cin), 0, 6), E.int_tensor(rs, (1, 1, Cin, Cout), -3, 3)
    res = E.int_tensor(rs, (N, H // 2, W // 2, Cout), -F.RES_MAX, F.RES_MAX)
    want = nhwc(onet.conv2d_same(nchw(a.double()), w.double()) + onet.nearest_neighbor_upsample(nchw(res.double())))
    assert torch.equal(F.upsample_add_ref(a, w, res), want)
    assert torch.equal(E.stats_ref(want), torch.stack([want.sum((0, 1, 2)), (want * want).sum((0, 1, 2))]))
    # one pixel left out of a statistics row is seen, on any map (the tolerance of test_conv_fwd lets it pass at 75 000 pixels)
    assert not torch.equal(E.stats_ref(want.reshape(-1, Cout)[1:]), E.stats_ref(want))
    # fused sums behind a data gradient: with pre = x * s + b and the gradient passed strictly inside (0, 6), the gradients of
    # b and s are sum g and sum g * x (RAW x)
    scale, shift = E.int_affine(rs, Cout)
    x = E.int_activations(rs, (N, H, W, Cout), scale)
    for act in (0, 1, 2):
        s, b = scale.double().requires_grad_(True), shift.double().requires_grad_(True)
        pre = x.double() * s + b
        ok = F.act_mask(x, scale, shift, act)
        assert act != 2 or (bool((pre <= 0).any()) and bool((pre >= 6).any()))
        torch.where(ok, pre, pre.detach()).backward(want)
        g, rows = F.bwd_data_bn_ref(want, x, scale, shift, act)
        assert torch.equal(rows, torch.stack([b.grad, s.grad])) and torch.equal(g, torch.where(ok, want, torch.zeros_like(want)))


# ------------------------------------------------------------------------------------------------------ regime conditions
def _covers_every_tap(a, k):
    """Every input channel is nonzero at some pixel under every tap."""
    if k == 1:
        return bool((a != 0).reshape(-1, a.shape[-1]).any(0).all())
    return all(bool((v != 0).reshape(-1, a.shape[-1]).any(0).all()) for _, _, v in E._taps(a, a.shape[1], a.shape[2], 1))


def _check_narrow(d, k, what):
    assert d.headroom < LIMIT, (what, d.headroom)
    assert float(d.want.abs().max()) <= F.Y_MAX, (what, float(d.want.abs().max()))
    assert E.representable16(d.want)
    assert F.stats_headroom(d.want) < LIMIT, (what, F.stats_headroom(d.want))
    assert bool((d.w != 0).all()), what
    assert _covers_every_tap(d.a, k), what
    assert float(d.want.abs().max()) >= 32, (what, "outputs too small to exercise anything")


def _check_wide(d, k, dt, with_stats, what):
    assert d.headroom < LIMIT, (what, d.headroom)
    share = F.share_not_representable(d.want, dt)
    assert share >= F.MIN_WIDE_SHARE, (what, share)
    assert bool((d.w != 0).all()) and _covers_every_tap(d.a, k), what
    assert E.representable16(d.a) and torch.equal(d.w.to(F.TORCH_DT[dt]).float(), d.w), what
    if with_stats:
        r = F.once_rounded(d.want, dt)
        assert F.stats_headroom(r) < LIMIT, (what, F.stats_headroom(r))
        assert not torch.equal(E.stats_ref(r), E.stats_ref(d.want)), (what, "the statistics candidates do not differ")


@pytest.mark.parametrize("name", [c.name for c in F.FWD_CASES + F.UP_CASES])
def test_forward_cases_meet_their_regimes(name):
    c = F.FWD_BY_NAME.get(name) or F.UP_BY_NAME[name]
    assert c.H >= 3 and c.W >= 3 and set(c.regimes) <= set(F.BOTH)
    if "narrow" in c.regimes:
        _check_narrow(F.fwd_case_data(name, "narrow"), c.k, name)
    for dt in c.dtypes:
        if "wide" in c.regimes and dt != "f32":
            ws = c.stats and F.wide_stats_for(c, dt)
            d = F.fwd_case_data(name, "wide", dt)
            _check_wide(d, c.k, dt, ws, (name, dt))
            assert (d.res is not None) == (name in F.UP_BY_NAME)
            if d.res is not None:
                assert E.representable16(d.res) and bool((d.res != 0).any())
    # the table's wide_stats column says no exactly where the map is too large for it
    assert c.wide_stats == (c.stats and "bf16" in c.dtypes and "wide" in c.regimes and c.N * c.H * c.W <= F.WIDE_STATS_MAX_PIXELS), name


def test_every_route_has_both_regimes_and_wide_statistics():
    for route in ("tiled1-128", "tiled1-256", "tiled3-128", "c3", "c3-64", "gemm"):
        cases = [c for c in F.FWD_CASES if c.route == route]
        assert any("narrow" in c.regimes and c.stats for c in cases), route
        assert any("wide" in c.regimes and c.wide_stats for c in cases), route
        assert any("wide" in c.regimes and "bf16" in c.dtypes for c in cases), route
        if route != "gemm":
            assert any("wide" in c.regimes and "fp16" in c.dtypes for c in cases), route
    assert {c.route for c in F.FWD_CASES if "f32" in c.dtypes} == {"tiled1-128", "tiled1-256", "tiled3-128"}


@pytest.mark.parametrize("k,Cin,Cout,routes", F.DGRAD_CASES, ids=[f"{c[0]}x{c[0]}-{c[1]}to{c[2]}" for c in F.DGRAD_CASES])
def test_data_gradient_cases_meet_their_regimes(k, Cin, Cout, routes):
    d = F.dgrad_case_data(k, Cin, Cout, "narrow")
    assert d.headroom < LIMIT and float(d.want.abs().max()) <= F.Y_MAX and bool((d.w != 0).all()) and _covers_every_tap(d.dy, k)
    for dt in routes:
        d = F.dgrad_case_data(k, Cin, Cout, "wide", dt)
        assert d.headroom < LIMIT and bool((d.w != 0).all()) and _covers_every_tap(d.dy, k)
        assert F.share_not_representable(d.want, dt) >= F.MIN_WIDE_SHARE, (dt, F.share_not_representable(d.want, dt))
        assert torch.equal(d.w.to(F.TORCH_DT[dt]).float(), d.w) and E.representable16(d.dy)


@pytest.mark.parametrize("case", F.GROUPED_CASES, ids=[g[0] for g in F.GROUPED_CASES])
def test_grouped_cases_meet_the_narrow_regime(case):
    name, Cin, Cout, k, act, route = case
    tiles = 0
    for j, (h, w) in enumerate(F.GROUPED_HW):
        _check_narrow(F.narrow_data(f"{name}/{j}", F.GROUPED_N, h, w, Cin, Cout, k, act), k, (name, j))
        tiles += F.GROUPED_N * -(-h // 16) * -(-w // 16)
    assert tiles > 256 and -(-F.GROUPED_HW[-1][0] // 16) * -(-F.GROUPED_HW[-1][1] // 16) == 1     # more tiles than compute units


def _bnr_jobs():
    for name, N, H, W, K, C, k, route in F.BNR_CASES:
        yield name, (name, N, H, W, K, C, k), route
        if k == 3:
            for j, (h, w) in enumerate(F.BNR_GROUPED_HW):
                yield name, (f"{name}/{j}", F.BNR_GROUPED_N, h, w, K, C, k), route


def test_fused_reduction_cases_meet_the_narrow_regime():
    lib = _lib.lib()
    for name, args, route in _bnr_jobs():
        d = F.bnr_case_data(*args)
        K, C, k = args[4:]
        assert d.headroom < LIMIT and float(d.dx.abs().max()) <= F.Y_MAX and d.rows_headroom < LIMIT, (args, d.rows_headroom)
        assert bool((d.w != 0).all()) and _covers_every_tap(d.dy, k), args
        pre = d.x.double() * d.scale.double() + d.shift.double()
        assert float((pre <= 0).double().mean()) > 0.2 and float((pre >= 6).double().mean()) > 0.1, args      # ReLU6 clips both ends
        assert bool((d.g != 0).any()) and not torch.equal(d.g, d.dx), args
        assert lib.mpn_conv_bwd_data_bn_supported(K, C, k, CODE["bf16"]) == 1 and F.conv_route(k, K, C, "bf16")[0] == route, args


# ------------------------------------------------------------------------------------------- the instrument discriminates
def _eval_f32(a, w, k, halves=None):
    """The convolution as a kernel forms it: f32 sums of products (shifted slices, f32 matrix products). halves: the two halves
    of the input channels are summed apart and each ROUNDED to that type before they are added - the exchange a kernel whose
    waves split K must not make."""
    a, w = a.float(), w.float()
    N, H, W, Cin = a.shape
    parts = []
    for lo, hi in ([(0, Cin)] if halves is None else [(0, Cin // 2), (Cin // 2, Cin)]):
        y = torch.zeros(N * H * W, w.shape[3])
        if k == 1:
            y += a[..., lo:hi].reshape(-1, hi - lo) @ w[0, 0, lo:hi]
        else:
            for ty, tx, v in E._taps(a[..., lo:hi], H, W, 1):
                y += v.reshape(-1, hi - lo) @ w[ty, tx, lo:hi]
        parts.append(y if halves is None else y.to(halves).float())
    return sum(parts).reshape(N, H, W, -1)


@pytest.mark.parametrize("name", ["g-320to512-affine", "cs-512to64"], ids=["1x1", "3x3"])
def test_an_intermediate_rounding_changes_bits(name):
    c = F.FWD_BY_NAME[name]
    d = F.fwd_case_data(name, "wide", "bf16")
    want = F.once_rounded(d.want, "bf16")
    honest = _eval_f32(d.a, d.w, c.k)
    assert torch.equal(honest.double(), d.want)                       # below 2^24: the f32 evaluation is exact ...
    E.assert_exact(honest.to(torch.bfloat16), want)                   # ... and rounded once it IS the expectation
    exchanged = _eval_f32(d.a, d.w, c.k, halves=torch.bfloat16).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="elements differ"):
        E.assert_exact(exchanged, want)
    assert float((exchanged.double() != want).double().mean()) > 0.01
    # ... and the statistics of the unrounded sums are not those of the rounded tensor
    assert F.wide_stats_for(c, "bf16") and not torch.equal(E.stats_ref(honest), E.stats_ref(want))


def test_a_residual_added_after_the_rounding_changes_bits():
    name = "u-256to128"
    d = F.fwd_case_data(name, "wide", "bf16")
    want = F.once_rounded(d.want, "bf16")
    conv = _eval_f32(d.a, d.w, 1)
    up = F.upsample2_ref(d.res).float()
    E.assert_exact((conv + up).to(torch.bfloat16), want)              # added in f32, rounded once
    late = (conv.to(torch.bfloat16).float() + up).to(torch.bfloat16)  # rounded, then added (and rounded again)
    with pytest.raises(AssertionError, match="elements differ"):
        E.assert_exact(late, want)
    assert float((late.double() != want).double().mean()) > 0.01


# ------------------------------------------------------------------------------------------------------------ route claims
def _packed(Cin, Cout, k, transpose, dt):
    return _lib.lib().mpn_conv_packed_bytes(Cin, Cout, k, transpose, CODE[dt])


def test_route_claims_against_the_packed_sizes():
    """The library's packed size equals what the claimed route packs. (The GEMM matrix and the persistent kernel's image have
    the bytes of an unpadded tiled image, so the size tells the routes apart only off the tile grid; the eligibility rules are
    restated in conv_route, and on the GPU the persistent routes show in mpn_conv_stats_rows.)"""
    for c in F.FWD_CASES + F.UP_CASES:
        for dt in c.dtypes:
            route, size = F.conv_route(c.k, c.Cin, c.Cout, dt)
            assert route == c.route, (c.name, dt, route)
            assert _packed(c.Cin, c.Cout, c.k, 0, dt) == size, (c.name, dt, size)
    for k, Cin, Cout, routes in F.DGRAD_CASES:
        for dt, claim in routes.items():
            route, size = F.conv_route(k, Cout, Cin, dt)
            assert route == claim and _packed(Cin, Cout, k, 1, dt) == size, (k, Cin, Cout, dt, route)
    for name, Cin, Cout, k, act, claim in F.GROUPED_CASES:
        route, size = F.conv_route(k, Cin, Cout, "bf16")
        assert route == claim and _packed(Cin, Cout, k, 0, "bf16") == size, name
    for name, N, H, W, K, C, k, claim in F.BNR_CASES:
        route, size = F.conv_route(k, K, C, "bf16")
        assert route == claim and _packed(C, K, k, 1, "bf16") == size, name
    # the packed sizes of shapes off the grid, where the routes differ: 136 -> 200 pads to 3 chunks x 4 n-tiles of 64
    assert F.conv_route(1, 136, 200, "bf16") == ("tiled1-128", 3 * 2 * 64 * 64 * 4) and _packed(136, 200, 1, 0, "bf16") == 98304
    assert F.conv_route(3, 40, 72, "fp16") == ("tiled3-128", 9 * 2 * 64 * 64 * 2) and _packed(40, 72, 3, 0, "fp16") == 147456
    # the GEMM rule's edges
    assert F.conv_route(1, 192, 256, "bf16")[0] == "tiled1-128" and F.conv_route(1, 256, 128, "bf16")[0] == "tiled1-128"
    assert F.conv_route(1, 512, 512, "fp16")[0] == "tiled1-256" and F.conv_route(1, 512, 512, "f32")[0] == "tiled1-256"
    assert F.conv_route(3, 576, 128, "bf16")[0] == "tiled3-128" and F.conv_route(3, 128, 128, "f32")[0] == "tiled3-128"


def test_the_gemm_case_on_256_pixel_tiles_is_the_first_such_map():
    c = F.FWD_BY_NAME["g-256to1024-256px-tiles"]
    M = c.N * c.H * c.W
    assert F.gemm_pixel_tile(M, c.Cout) == 256 and F.gemm_pixel_tile(M - 1, c.Cout) == 128 and M % 256 != 0 and M % 128 != 0
    for other in F.FWD_CASES:
        if other.route == "gemm" and other is not c:
            assert F.gemm_pixel_tile(other.N * other.H * other.W, other.Cout) == 128, other.name
    assert F.gemm_pixel_tile(2 * 16 * 16, 512) == 128       # the fused reduction's GEMM case: 128-pixel tiles
