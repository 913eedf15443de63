"""GPU: the fused depthwise backward walks with the apply pass of the depthwise conv's own batch-norm on load
(mpn_dwconv_bwd_fused_apply / _s2_apply) against mpn_bn_bwd_apply followed by the plain walk: bit for bit."""
import numpy as np
import pytest
import torch

from util import dev, rnd

pytestmark = pytest.mark.gpu

S1 = [(2, 16, 16, 64), (1, 37, 29, 32),      # a strip and a column pair end inside the map
      (1, 130, 70, 32),                      # more than one 64-row strip
      (1, 9, 11, 1024),                      # many channel blocks
      (3, 24, 24, 256)]
S2 = [(2, 16, 16, 64), (1, 32, 32, 512), (1, 38, 30, 32)]
CASES = ([(1, s, False, act) for s in S1 for act in (2, 1)] + [(2, s, add, act) for s in S2 for add in (False, True) for act in (2, 1)]
         + [(1, S1[1], False, 0), (2, S2[2], True, 0)])                                   # no activation: nothing to mask
IDS = [f"s{st}-{'x'.join(map(str, s))}{'-add' if add else ''}-{('none', 'relu', 'relu6')[act]}" for st, s, add, act in CASES]


def _bn(ops, rs, C, act):
    """Random per-channel state, as mkbn() of test_ops_bwd_gpu.py, with the k1 / k2 a finalize would leave."""
    one = lambda: dev(torch.tensor((0.5 + rs.rand(C)).astype(np.float32)))
    bn = ops.BNState(one(), one(), one(), one(), act)
    bn.scale.copy_(one()); bn.invstd.copy_(one())
    bn.shift.copy_(dev((rs.randn(C) * 0.5).astype(np.float32))); bn.mean.copy_(dev((rs.randn(C) * 0.3).astype(np.float32)))
    bn.k1.copy_(dev((rs.randn(C) * 0.05).astype(np.float32))); bn.k2.copy_(dev((rs.randn(C) * 0.05).astype(np.float32)))
    return bn


def _operands(ops, stride, shape, add, act, dtype):
    N, H, W, C = shape
    rs = np.random.RandomState(H + W + C + 7 * stride + act)
    oshape = (N, H // stride, W // stride, C)
    x = dev(rnd(rs.randn(*shape), dtype), dtype)                        # the conv's raw input = raw output of the layer below
    w = dev((rs.randn(3, 3, C) / 3).astype(np.float32))
    bn_in, bn_ap = _bn(ops, rs, C, 2), _bn(ops, rs, C, act)
    # the conv's raw output: y * scale + shift at least 1e-3 away from 0 and from 6, so that the mask built here and the one of
    # mpn_bn_bwd_apply agree whatever the rounding of the product; an element too close moves to the middle of the interval
    y = rnd(rs.randn(*oshape) * 1.5 + 0.5, dtype)
    sc, sh = bn_ap.scale.cpu(), bn_ap.shift.cpu()
    pre = y * sc + sh
    close = ((pre.abs() < 1e-3) | ((pre - 6).abs() < 1e-3))
    y = torch.where(close, rnd(((3.0 - sh) / sc).expand_as(y), dtype), y)
    pre = y * sc + sh
    assert not bool(((pre.abs() < 1e-3) | ((pre - 6).abs() < 1e-3)).any())
    lo, hi = (0.0 if act else -np.inf), (6.0 if act == 2 else np.inf)
    passes = (pre > lo) & (pre < hi)
    assert act == 0 or (bool(passes.any()) and not bool(passes.all()))
    g = rnd(rs.randn(*oshape), dtype) * passes                          # ALREADY masked, as the producers that reduce write it
    addend = dev(rnd(rs.randn(*shape), dtype), dtype) if add else None
    return x, w, bn_in, bn_ap, dev(y, dtype), dev(g, dtype), addend


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("stride,shape,add,act", CASES, ids=IDS)
def test_apply_on_load_equals_the_apply_pass_then_the_walk(cuda, dtype, stride, shape, add, act):
    """Path A: mpn_bn_bwd_apply over a copy of g, then the fused walk. Path B: the folded walk over the untouched g. The data
    gradient, the whole weight-partial slab and the reduction rows: torch.equal; g unchanged. The depthwise walks store bf16
    and f32 only: in fp16 both paths refuse the layer, the same way."""
    from multiposenet_amd import ops
    N, H, W, C = shape
    if dtype == torch.float16:
        assert not ops.dwconv_bwd_fused_supported(N, H, W, C, stride, dtype) and not ops.dwconv_bwd_fused_apply_supported(N, H, W, C, stride, dtype)
        x = torch.zeros(shape, dtype=dtype, device="cuda")
        d = torch.zeros((N, H // stride, W // stride, C), dtype=dtype, device="cuda")
        wz, bn = torch.zeros(3, 3, C, device="cuda"), _bn(ops, np.random.RandomState(0), C, act)
        for kw in ({}, {"apply_bn": bn, "y_raw": d}):
            with pytest.raises(ValueError):
                ops.dwconv_bwd_fused(x, d, wz, bn, None, reduce=False, stride=stride, **kw)
        return
    assert ops.dwconv_bwd_fused_apply_supported(N, H, W, C, stride, dtype)
    x, w, bn_in, bn_ap, y, g, addend = _operands(ops, stride, shape, add, act, dtype)
    rows = ops.dwconv_wgrad_num_parts(N, H, W, C, stride, dtype)
    mk = lambda: (torch.full((rows * 9 * C,), float("nan"), device="cuda"), torch.full((rows * 2 * C,), float("nan"), device="cuda"))
    # A: the separate pass, then the walk
    dy = g.clone()
    ops.bn_bwd_apply(bn_ap, dy, y)
    assert not torch.equal(dy, g)
    wp_a, sp_a = mk()
    dA_a, r_a = ops.dwconv_bwd_fused(x, dy, w, bn_in, None, wpart=wp_a, bn_part=sp_a, reduce=False, stride=stride, addend=addend)
    # B: applied on load
    g0, y0 = g.clone(), y.clone()
    wp_b, sp_b = mk()
    dA_b, r_b = ops.dwconv_bwd_fused(x, g, w, bn_in, None, wpart=wp_b, bn_part=sp_b, reduce=False, stride=stride, addend=addend,
                                     apply_bn=bn_ap, y_raw=y)
    assert r_a == r_b == rows
    assert torch.equal(g, g0) and torch.equal(y, y0)
    assert not bool(torch.isnan(wp_a).any()) and not bool(torch.isnan(sp_a).any()) and not bool(torch.isnan(dA_a.float()).any())
    assert torch.equal(dA_b, dA_a)
    assert torch.equal(wp_b, wp_a)
    assert torch.equal(sp_b, sp_a)
    # without the reduction: the other instantiation, the same gradients
    wp_n, _ = mk()
    dA_n, r_n = ops.dwconv_bwd_fused(x, g, w, bn_in, None, wpart=wp_n, reduce=False, reduce_bn=False, stride=stride, addend=addend,
                                     apply_bn=bn_ap, y_raw=y)
    assert r_n == 0 and torch.equal(dA_n, dA_a) and torch.equal(wp_n, wp_a)


def test_network_gradients_do_not_change_with_the_apply_folded_into_the_walks(cuda):
    """Forward, losses and backward at 2 x 128 x 128 in bf16 with KeypointNet.fuse_dw_apply on and off: the same losses and the
    same flat gradient, bit for bit - and the folded entry points are what ran."""
    from test_network_gpu import _labels, _params
    from multiposenet_amd import _lib
    from multiposenet_amd.net import KeypointNet
    from multiposenet_amd.train import Trainer
    rs = np.random.RandomState(21)
    B, H, W = 2, 128, 128
    params = _params(9)
    img = torch.tensor(rs.rand(B, H, W, 3).astype(np.float32)).cuda()
    dlab = {k: torch.tensor(val).cuda() for k, val in _labels(rs, B, H // 4, W // 4).items()}
    hp = {"initial_learning_rate": 3e-4, "num_steps": 200000, "weight_decay": 0.0, "depth_multiplier": 1.0}
    out = {}
    for fold in (False, True):
        net = KeypointNet(values=params, dtype=torch.bfloat16)
        assert net.fuse_dw_apply                                        # on by default
        net.fuse_dw_apply = fold
        tr = Trainer(net, hp, use_graph=False)
        _lib.PROFILE = []
        try:
            loss = tr.step({"images": img}, dlab).clone()
            names = [name for _, name, _, _ in _lib.PROFILE]
        finally:
            _lib.PROFILE = None
        folded = sum(n in ("mpn_dwconv_bwd_fused_apply", "mpn_dwconv_bwd_fused_s2_apply") for n in names)
        assert (folded > 0) == fold
        out[fold] = (loss, net.grad.clone(), folded, names.count("mpn_bn_bwd_apply"))
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])
    assert out[False][3] - out[True][3] == out[True][2]                 # one apply launch less per folded walk
