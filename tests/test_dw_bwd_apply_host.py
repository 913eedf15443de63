"""CPU: the fused depthwise backward walks with the batch-norm backward apply on load (mpn_dwconv_bwd_fused_apply / _s2_apply) - the
support query and the argument checks that run before any HIP call. No GPU, no compute call."""
import ctypes

import pytest

from multiposenet_amd import _lib

L = _lib.lib
BF16, F32, F16 = _lib.MPN_BF16, _lib.MPN_F32, _lib.MPN_F16

# (N, H, W, C, stride): the bench layers' classes, odd sizes, the channel counts and odd stride-2 maps the fused walk refuses
SHAPES = [(32, 256, 256, 32, 1), (32, 256, 256, 64, 2), (32, 32, 32, 512, 1), (32, 32, 32, 512, 2), (32, 16, 16, 1024, 1),
          (2, 16, 16, 64, 1), (1, 37, 29, 32, 1), (1, 130, 70, 32, 1), (1, 9, 11, 1024, 1), (1, 38, 30, 32, 2),
          (1, 37, 29, 32, 2), (1, 12, 20, 24, 1), (1, 14, 10, 24, 2), (1, 1, 600, 8, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_apply_supported_follows_the_fused_walk_in_16_bit_storage_and_refuses_f32(shape):
    lib = L()
    for dt in (BF16, F16):
        assert lib.mpn_dwconv_bwd_fused_apply_supported(*shape, dt) == lib.mpn_dwconv_bwd_fused_supported(*shape, dt)
    assert lib.mpn_dwconv_bwd_fused_apply_supported(*shape, F32) == 0
    assert lib.mpn_dwconv_bwd_fused_apply_supported(*shape[:4], 3, BF16) == 0          # no such stride


def test_the_table_holds_shapes_of_both_kinds():
    lib = L()
    got = [lib.mpn_dwconv_bwd_fused_apply_supported(*s, BF16) for s in SHAPES]
    assert 0 in got and 1 in got


def _args(stride, **null):
    """The argument list of the entry point with fake non-null pointers (nothing is dereferenced before the checks fail)."""
    seen = []

    def P(name):
        seen.append(name)
        return None if name in null else ctypes.c_void_p(0x1000 * len(seen))
    N, H, W, C = 2, 16, 16, 64
    a = [P("x"), P("g"), P("y"), P("w"), P("dx"), P("wpart"), N, H, W, C, BF16, P("in_scale"), P("in_shift"), 2, P("mean"), P("invstd"),
         P("bn_part")]
    if stride == 2:
        a.append(P("addend"))
    return a + [P("scale"), P("shift"), P("ap_mean"), P("ap_invstd"), P("k1"), P("k2"), 2, None]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("missing", ["y", "k1", "k2", "scale", "g", "dx"])
def test_null_pointers_are_refused_before_any_hip_call(stride, missing):
    name = "mpn_dwconv_bwd_fused_apply" if stride == 1 else "mpn_dwconv_bwd_fused_s2_apply"
    with pytest.raises(ValueError, match="null pointer"):
        _lib.call(name, *_args(stride, **{missing: True}))


@pytest.mark.parametrize("stride", [1, 2])
def test_f32_and_unsupported_shapes_are_refused_before_any_hip_call(stride):
    name = "mpn_dwconv_bwd_fused_apply" if stride == 1 else "mpn_dwconv_bwd_fused_s2_apply"
    a = _args(stride)
    a[10] = F32
    with pytest.raises(ValueError, match="not supported"):
        _lib.call(name, *a)
    a = _args(stride)
    a[9] = 24                                                                           # the LDS-tile weight gradient's channel count
    with pytest.raises(ValueError, match="not supported"):
        _lib.call(name, *a)
