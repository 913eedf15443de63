"""CPU: the exact-integer references of tests/exact_ref.py against the oracle's autograd, their sensitivity to one pixel, and the
case table of tests/test_reduction_exact_gpu.py against the library's own split counts (host code: loads without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import exact_ref as E
from multiposenet_amd import _lib
from oracle import network as onet
from util import nchw, nhwc

CODE = {"bf16": _lib.MPN_BF16, "fp16": _lib.MPN_F16, "f32": _lib.MPN_F32}
PROPERTIES = ("multi_rem", "single", "partial_cg", "partial_cb")


# ------------------------------------------------------------------------------------------- references against the oracle
@pytest.mark.parametrize("k,act", [(3, 0), (3, 2), (1, 1), (1, 2)])
def test_conv_reference_equals_the_oracles_autograd(k, act):
    rs = np.random.RandomState(k + act)
    N, H, W, Cin, Cout = 2, 11, 19, 24, 16
    scale, shift = E.int_affine(rs, Cin)
    x = E.int_activations(rs, (N, H, W, Cin), scale)
    dy = E.int_tensor(rs, (N, H, W, Cout), -E.DY_MAX, E.DY_MAX)
    a = E.act_affine(x, scale, shift, act)
    assert act != 2 or (bool((a == 0).float().mean() > 0.2) and bool((a == 6).float().mean() > 0.2))   # ReLU6 clips both ends
    w = torch.zeros(k, k, Cin, Cout, dtype=torch.float64, requires_grad=True)
    onet.conv2d_same(nchw(a), w).backward(nchw(dy.double()))
    assert torch.equal(E.conv_wgrad_ref(a, dy, k), w.grad)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", [(9, 7), (12, 20), (1, 1), (2, 5)])
def test_depthwise_reference_equals_the_oracles_autograd(H, W, stride):
    rs = np.random.RandomState(H + stride)
    C = 16
    x = E.int_tensor(rs, (2, H, W, C), 0, 6)
    w = torch.zeros(3, 3, C, 1, dtype=torch.float64, requires_grad=True)
    out = onet.depthwise_conv2d_tf_same(nchw(x.double()), w, stride)
    dy = E.int_tensor(rs, tuple(nhwc(out).shape), -3, 3)
    out.backward(nchw(dy.double()))
    assert torch.equal(E.dwconv_wgrad_ref(x, dy, stride), w.grad[..., 0])


@pytest.mark.parametrize("H,W", [(30, 34), (17, 9), (8, 8)])
def test_stem_reference_equals_the_oracles_autograd(H, W):
    rs = np.random.RandomState(H)
    img = E.int_tensor(rs, (2, H, W, 3), 0, 2) * 0.5
    w = torch.zeros(3, 3, 3, 16, dtype=torch.float64, requires_grad=True)
    out = onet.conv2d_tf_same(nchw(2.0 * img.double() - 1.0), w, 2)
    dy = E.int_tensor(rs, tuple(nhwc(out).shape), -3, 3)
    out.backward(nchw(dy.double()))
    assert torch.equal(E.stem_wgrad_ref(img, dy), w.grad)


def test_matrix_and_slab_references_equal_autograd():
    rs = np.random.RandomState(4)
    a, dl = E.int_tensor(rs, (77, 32), 0, 9), E.int_tensor(rs, (77, 18), -3, 3)
    w = torch.zeros(32, 18, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(18, dtype=torch.float64, requires_grad=True)
    (a.double() @ w + b).backward(dl.double())
    assert torch.equal(E.head_ref(a, dl), torch.cat([w.grad.reshape(-1), b.grad]))
    p, q = E.int_tensor(rs, (5, 40), -3, 3), E.int_tensor(rs, (12, 40), -3, 3)
    assert torch.equal(E.gemm_nt_ref(p, q), torch.einsum("mk,nk->mn", p.double(), q.double()))
    x = E.int_tensor(rs, (50, 8), -8, 8)
    assert torch.equal(E.stats_ref(x), torch.stack([x.double().sum(0), x.double().pow(2).sum(0)]))
    # batch-norm backward sums: dbeta = sum g and dgamma = sum g * xhat of y = act(gamma * xhat + beta) at gamma = scale / invstd
    d = E.bn_case_data(777, 8, 2)
    gamma = (d["scale"] / d["invstd"]).double().requires_grad_(True)
    beta = (d["shift"].double() + d["mean"].double() * d["scale"].double()).requires_grad_(True)
    xhat = (d["x"].double() - d["mean"].double()) * d["invstd"].double()
    pre = gamma * xhat + beta
    # (the kernels' ReLU6 passes the gradient strictly inside (0, 6); torch.clamp's also passes it AT 0 and 6, where integers do land)
    torch.where((pre > 0) & (pre < 6), pre, pre.detach().clamp(0, 6)).backward(d["dA"].double())
    assert torch.equal(d["want_bwd"], torch.stack([beta.grad, gamma.grad]))


# ------------------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("name,act", [("narrow-40to24", 2), ("wide-128to128-588tiles", 1)], ids=["small", "largest"])
def test_one_pixel_fails_assert_exact(name, act):
    """The reference with ONE pixel's contribution removed, added twice, or added at the wrong tap is not `exact` any more -
    on a small case and on the case with the most pixels (where 1.2e-2 * max|dW| hides whole tiles)."""
    c = E.CONV_BY_NAME[name]
    d = E.conv_case_data(name, act)
    a = E.act_affine(d.x, d.scale, d.shift, act)
    geom = E.geometry(c.k, c.Cin, c.Cout, "bf16")[1:]
    E.assert_exact(d.want.float(), d.want, geom)
    # a pixel whose activation and gradient are both non-zero somewhere
    n, y, x = c.N - 1, c.H // 2, c.W // 2
    one = torch.outer(a[n, y, x], d.dy[n, y, x].double())
    assert bool((one != 0).any())
    for tap, sign in (((1, 1), -1.0), ((1, 1), 1.0), ((0, 2), 1.0)):
        bad = d.want.clone()
        bad[tap] += sign * one
        with pytest.raises(AssertionError, match="elements differ") as e:
            E.assert_exact(bad.float(), d.want, geom)
        assert f"taps [{tap}]" in str(e.value) and "channel groups" in str(e.value) and "output blocks" in str(e.value)
    nan = d.want.float().clone()
    nan[2, 2, c.Cin - 1, c.Cout - 1] = float("nan")
    with pytest.raises(AssertionError, match="1 of"):
        E.assert_exact(nan, d.want, geom)


# ------------------------------------------------------------------------------------------------------------- case table
def _nparts(c, dtype):
    return _lib.lib().mpn_conv_wgrad_num_parts(c.N, c.H, c.W, c.Cin, c.Cout, c.k, CODE[dtype])


def _properties(c, dtype):
    _, cg, cb = E.geometry(c.k, c.Cin, c.Cout, dtype)
    nt, nparts = E.ntiles(c.N, c.H, c.W, c.k), _nparts(c, dtype)
    got = set()
    if nparts > 1 and nt % nparts != 0:
        got.add("multi_rem")
    if nparts == 1:
        got.add("single")
    if c.Cin % cg:
        got.add("partial_cg")
    if c.Cout % cb:
        got.add("partial_cb")
    return got


def test_split_formula_restated():
    """mpn_conv_wgrad_num_parts = min(blocks / (channel groups * output blocks), ntiles / min tiles per split), at least 1, with
    ntiles = 8 x 16-pixel tiles per image (3x3) or 128-pixel tiles (1x1) - the restatement the table's claims rest on."""
    for c in E.CONV_CASES:
        for dtype in c.dtypes:
            _, cg, cb = E.geometry(c.k, c.Cin, c.Cout, dtype)
            blocks, min_tiles = (512, 1) if dtype == "f32" else (256, 4)
            nt = E.ntiles(c.N, c.H, c.W, c.k)
            want = max(1, min(max(1, blocks // (-(-c.Cin // cg) * -(-c.Cout // cb))), nt // min_tiles))
            assert _nparts(c, dtype) == want, (c.name, dtype, _nparts(c, dtype), want)


def test_every_case_keeps_the_property_it_is_in_the_table_for():
    for c in E.CONV_CASES:
        got = _properties(c, c.dtypes[0])
        assert c.claims <= got, f"{c.name} ({c.dtypes[0]}) lost {sorted(c.claims - got)}: the kernel's tiling changed - move the case"
        if "fp16" in c.dtypes:
            assert _properties(c, "fp16") == _properties(c, "bf16")


@pytest.mark.parametrize("dtype,geom", [(d, g) for d in ("bf16", "fp16") for g in ("wide3x3", "narrow3x3", "general1x1", "thin1x1")] +
                         [("f32", g) for g in ("f32-narrow3x3", "f32-wide3x3", "f32-1x1")])
def test_every_geometry_has_every_property(dtype, geom):
    have = set()
    for c in E.CONV_CASES:
        if dtype in c.dtypes and E.geometry(c.k, c.Cin, c.Cout, dtype)[0] == geom:
            have |= _properties(c, dtype)
    assert have >= set(PROPERTIES), f"{geom} / {dtype}: no case with {sorted(set(PROPERTIES) - have)}"


def test_required_shapes_are_in_the_table():
    shapes = {(c.Cin, c.Cout, c.k) for c in E.CONV_CASES}
    for s in [(128, 128, 3), (64, 256, 3), (128, 192, 3), (40, 72, 3), (64, 640, 3), (64, 64, 3), (128, 64, 3), (256, 64, 3), (512, 64, 3),
              (64, 24, 3), (64, 8, 3), (256, 512, 1), (256, 256, 1), (136, 200, 1), (32, 128, 1), (48, 96, 1), (96, 192, 1), (1024, 1024, 1),
              (32, 64, 1), (16, 32, 1), (24, 48, 1), (8, 16, 1)]:
        assert s in shapes, s
    by = E.CONV_BY_NAME
    assert E.ntiles(*by["wide-128to128-588tiles"][1:4], 3) == 588 and _nparts(by["wide-128to128-588tiles"], "bf16") == 128
    assert E.ntiles(*by["wide-40to72"][1:4], 3) >= 16 and E.ntiles(*by["pw-136to200"][1:4], 1) >= 20
    c = by["pw-1024to1024"]
    assert E.ntiles(c.N, c.H, c.W, 1) // _nparts(c, "bf16") >= 8
    assert by["pw-64to128-128px"].H * by["pw-64to128-128px"].W == 128 and by["pw-64to128-129px"].H * by["pw-64to128-129px"].W == 129
    # batch boundaries: N > 1 with H, W off the (8, 16) tile, so a split's walk crosses from one image into the next
    assert any(c.k == 3 and c.N > 1 and c.H % 8 and c.W % 16 and _nparts(c, c.dtypes[0]) > 1 for c in E.CONV_CASES)


def test_grouped_tables():
    """Two to five levels per table, the last of a single tile; the library gives every job at least one slab, the 16-bit
    grouped grid gives a job another split count than the job would get alone somewhere (else the table proves nothing new),
    and several jobs have splits of unequal tile counts."""
    lib = _lib.lib()
    differs, uneven = False, 0
    for name, N, Cin, Cout, k, act, hws in E.GROUPED_CASES:
        n = len(hws)
        assert 2 <= n <= 5 and E.ntiles(N, *hws[-1], k) == 1, name
        IA = ctypes.c_int * n
        out = IA()
        assert lib.mpn_conv_wgrad_grouped_num_parts(n, N, IA(*[h for h, _ in hws]), IA(*[w for _, w in hws]), Cin, Cout, k, CODE["bf16"], out) == 0
        assert all(v >= 1 for v in out), (name, list(out))
        alone = [lib.mpn_conv_wgrad_num_parts(N, h, w, Cin, Cout, k, CODE["bf16"]) for h, w in hws]
        differs = differs or list(out) != alone
        uneven += sum(1 for v, (h, w) in zip(out, hws) if v > 1 and E.ntiles(N, h, w, k) % v)
    assert differs and uneven >= 3, uneven


def test_depthwise_table_has_single_and_multiple_slabs():
    lib = _lib.lib()
    for dtype in ("bf16", "f32"):
        counts = [lib.mpn_dwconv_wgrad_num_parts(N, H, W, C, s, CODE[dtype]) for (N, H, W, C) in E.DW_CASES for s in (1, 2)]
        assert all(n > 0 for n in counts) and min(counts) == 1 and max(counts) > 8, counts


def test_batch_norm_table_reaches_blocks_of_more_than_128_rows():
    """The largest row count is past the cap of the slab grid (2048 blocks of 128 rows): a block then walks more rows."""
    lib = _lib.lib()
    M = max(E.BN_M)
    parts = lib.mpn_bn_stats_num_parts(M)
    assert parts == 2048 and -(-M // parts) > 128
    assert all(lib.mpn_bn_stats_num_parts(m) < 2048 for m in E.BN_M if m != M)
    assert {C for m, C in E.BN_MC if m == M} == {8, 24, 64}          # 16-, 32-byte and odd (6 / 3 vectors) rows


# --------------------------------------------------------------------------------------------------------------- headroom
def test_headroom_below_2_pow_24_everywhere():
    worst = {}
    for c in E.CONV_CASES:
        worst[c.name] = max(E.conv_case_data(c.name, act).headroom for act in c.acts)
    for name, N, Cin, Cout, k, act, hws in E.GROUPED_CASES:
        worst[name] = max(E.conv_case_data(f"{name}/{j}", act, N, h, w, Cin, Cout, k).headroom for j, (h, w) in enumerate(hws))
    for c in E.FUSED1X1_CASES:
        for apply in (False, True):
            if apply and c[3] > 64:
                continue
            d = E.fused1x1_case_data(*c, apply)
            assert d["dx_bound"] <= 256, (c, apply, d["dx_bound"])
            worst[("fused", c, apply)] = max(d["headroom"], d["bn_headroom"])
    for c in E.DW_CASES:
        for s in (1, 2):
            worst[("dw", c, s)] = E.dw_case_data(*c, s)["headroom"]
    for m in E.STEM_MAPS:
        worst[("stem", m)] = E.stem_case_data(*m, 64)["headroom"]
    for M in E.HEAD_M:
        worst[("head", M)] = E.head_case_data(M, 64)["headroom"]
    for g in E.GEMM_CASES:
        worst[("gemm", g)] = E.gemm_case_data(*g)["headroom"]
    for M, C in E.BN_MC:
        worst[("bn", M, C)] = max(E.bn_case_data(M, C, act)["headroom"] for act in ((1, 2) if M in E.BN_X_MAX else (2,)))
    over = {k: v for k, v in worst.items() if not v < E.EXACT_LIMIT}
    assert not over, over
    assert max(worst.values()) > 2 ** 20        # ... and the largest cases are large: not far below the limit either
