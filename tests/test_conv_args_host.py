"""CPU: the argument checks of the eight dense-convolution entry points (mpn_conv_fwd[_grouped], mpn_conv_bwd_data_bn[_grouped],
mpn_conv_bwd_weight[_grouped], mpn_conv1x1_bwd_fused[_apply]). Every row is a valid argument list with fake non-null pointers and
exactly ONE defect, so it is refused before any HIP call and nothing is dereferenced: no GPU, no compute call, and never a fully
valid list. The grouped entries get every row twice - as their only job, and as job 1 behind a valid job 0 - so that a single call
and a group of one, and every job of a group, are refused alike."""
import ctypes

import pytest

from multiposenet_amd import _lib

BF16, F32 = _lib.MPN_BF16, _lib.MPN_F32
P, I = ctypes.c_void_p, ctypes.c_int
POINTERS = ("x", "w", "y", "in_scale", "in_shift", "part", "up_res", "bn_x", "bn_scale", "bn_shift", "wf", "dx", "bn_part", "y_raw",
            "ap_scale", "ap_shift", "ap_mean", "ap_invstd", "k1", "k2")


def _job(j):
    """One valid job: x / y are the entry's input / output tensors (dy / dx of a data gradient, x / dy of a weight gradient)."""
    d = {name: 0x100000 * (j + 1) + 0x1000 * (k + 1) for k, name in enumerate(POINTERS)}
    d.update(up_res=None, H=16 - 2 * j, W=16 - 2 * j, x_stride=0, y_stride=0, bn_x_stride=0, dx_stride=0, y_raw_stride=0)
    return d


def _ints(jobs, n):
    return (I * len(jobs))(*[j[n] for j in jobs])


def _ptrs(jobs, n):
    return None if any(j[n] == "no array" for j in jobs) else (P * len(jobs))(*[j[n] for j in jobs])


# entry point -> its argument list from the layer `l` and the jobs `js` (single entries: one job)
def _fwd(l, js):
    j = js[0]
    return [j["x"], j["w"], j["y"], l["N"], j["H"], j["W"], l["Cin"], l["Cout"], j["x_stride"], j["y_stride"], l["ksize"], l["dtype"],
            j["in_scale"], j["in_shift"], 1, j["part"], j["up_res"], None]


def _fwd_grouped(l, js):
    return [l["njobs"], _ptrs(js, "x"), _ptrs(js, "w"), _ptrs(js, "y"), l["N"], _ints(js, "H"), _ints(js, "W"), l["Cin"], l["Cout"],
            _ints(js, "x_stride"), _ints(js, "y_stride"), l["ksize"], l["dtype"], _ptrs(js, "in_scale"), _ptrs(js, "in_shift"), 1,
            _ptrs(js, "part"), None]


def _bwd_data_bn(l, js):
    j = js[0]
    return [j["x"], j["w"], j["y"], l["N"], j["H"], j["W"], l["Cin"], l["Cout"], j["x_stride"], j["y_stride"], l["ksize"], l["dtype"],
            j["bn_x"], j["bn_x_stride"], j["bn_scale"], j["bn_shift"], 1, j["part"], None]


def _bwd_data_bn_grouped(l, js):
    return [l["njobs"], _ptrs(js, "x"), _ptrs(js, "w"), _ptrs(js, "y"), l["N"], _ints(js, "H"), _ints(js, "W"), l["Cin"], l["Cout"],
            _ints(js, "x_stride"), _ints(js, "y_stride"), l["dtype"], _ptrs(js, "bn_x"), _ints(js, "bn_x_stride"), _ptrs(js, "bn_scale"),
            _ptrs(js, "bn_shift"), 1, _ptrs(js, "part"), None]


def _bwd_weight(l, js):
    j = js[0]
    return [j["x"], j["y"], j["part"], l["N"], j["H"], j["W"], l["Cin"], l["Cout"], j["x_stride"], j["y_stride"], l["ksize"], l["dtype"],
            j["in_scale"], j["in_shift"], 1, None]


def _bwd_weight_grouped(l, js):
    return [l["njobs"], _ptrs(js, "x"), _ptrs(js, "y"), _ptrs(js, "part"), l["N"], _ints(js, "H"), _ints(js, "W"), l["Cin"], l["Cout"],
            _ints(js, "x_stride"), _ints(js, "y_stride"), l["ksize"], l["dtype"], _ptrs(js, "in_scale"), _ptrs(js, "in_shift"), 1, None]


def _fused(l, js):
    j = js[0]
    return [j["x"], j["y"], j["wf"], j["dx"], j["part"], j["bn_part"], l["N"], j["H"], j["W"], l["Cin"], l["Cout"], j["x_stride"],
            j["y_stride"], j["dx_stride"], l["dtype"], j["in_scale"], j["in_shift"], 1, None]


def _fused_apply(l, js):
    j = js[0]
    return [j["x"], j["y"], j["y_raw"], j["wf"], j["dx"], j["part"], j["bn_part"], l["N"], j["H"], j["W"], l["Cin"], l["Cout"],
            j["x_stride"], j["y_stride"], j["y_raw_stride"], j["dx_stride"], l["dtype"], j["in_scale"], j["in_shift"], 1, j["ap_scale"],
            j["ap_shift"], j["ap_mean"], j["ap_invstd"], j["k1"], j["k2"], 1, None]


def _layer(cin, cout, ksize, dtype=BF16):
    return dict(N=2, Cin=cin, Cout=cout, ksize=ksize, dtype=dtype)


FWD_PTRS, BNR_PTRS, WGRAD_PTRS = ("x", "w", "y"), ("x", "w", "y", "bn_x", "bn_scale", "bn_shift", "part"), ("x", "y", "part")
FUSED_PTRS = ("x", "y", "wf", "dx", "part", "in_scale", "in_shift")
APPLY_PTRS = FUSED_PTRS + ("bn_part", "y_raw", "ap_scale", "ap_shift", "ap_mean", "ap_invstd", "k1", "k2")

# name -> (argument list, pointer arrays of a grouped entry, valid layers (one per kernel route), required pointers, 16-byte-aligned
#          pointers, takes f32, has ksize, pairs in_scale with in_shift, pixel strides)
ENTRIES = {
    # routes: the persistent 3x3 kernel, the tiled kernel (3x3 and 1x1), the GEMM kernel
    "mpn_conv_fwd": (_fwd, (), [_layer(64, 64, 3), _layer(24, 64, 3), _layer(64, 64, 1), _layer(256, 256, 1)], FWD_PTRS, FWD_PTRS,
                     True, True, True, ("x_stride", "y_stride")),
    # routes: one grid of the persistent 3x3 kernel, one of the tiled kernel, separate launches
    "mpn_conv_fwd_grouped": (_fwd_grouped, FWD_PTRS + ("in_scale", "in_shift", "part"), [_layer(64, 64, 3), _layer(24, 64, 3), _layer(64, 64, 1)],
                             FWD_PTRS, FWD_PTRS, True, True, True, ("x_stride", "y_stride")),
    "mpn_conv_bwd_data_bn": (_bwd_data_bn, (), [_layer(64, 64, 3), _layer(64, 24, 3), _layer(64, 64, 1), _layer(256, 256, 1)],
                             BNR_PTRS, ("x", "w", "y", "bn_x"), False, True, False, ("x_stride", "y_stride", "bn_x_stride")),
    "mpn_conv_bwd_data_bn_grouped": (_bwd_data_bn_grouped, BNR_PTRS, [_layer(64, 64, 3), _layer(64, 24, 3)], BNR_PTRS, ("x", "w", "y", "bn_x"),
                                     False, False, False, ("x_stride", "y_stride", "bn_x_stride")),
    "mpn_conv_bwd_weight": (_bwd_weight, (), [_layer(64, 64, 3), _layer(64, 128, 3), _layer(64, 64, 1), _layer(32, 64, 1)],
                            WGRAD_PTRS, ("x", "y"), True, True, True, ("x_stride", "y_stride")),
    "mpn_conv_bwd_weight_grouped": (_bwd_weight_grouped, WGRAD_PTRS + ("in_scale", "in_shift"), [_layer(64, 64, 3), _layer(64, 64, 1)],
                                    WGRAD_PTRS, ("x", "y"),
                                    True, True, True, ("x_stride", "y_stride")),
    "mpn_conv1x1_bwd_fused": (_fused, (), [_layer(64, 64, 1), _layer(128, 128, 1)], FUSED_PTRS, ("x", "y", "dx"), False, False, False,
                              ("x_stride", "y_stride", "dx_stride")),
    "mpn_conv1x1_bwd_fused_apply": (_fused_apply, (), [_layer(64, 64, 1), _layer(32, 64, 1)], APPLY_PTRS, ("x", "y", "dx", "y_raw"),
                                    False, False, False, ("x_stride", "y_stride", "dx_stride", "y_raw_stride")),
}
CHANNELS = {"x_stride": "Cin", "y_stride": "Cout", "bn_x_stride": "Cout", "dx_stride": "Cin", "y_raw_stride": "Cout"}
# (the vector kernels fetch bn_scale / bn_shift as 16-byte vectors: the tiled and the GEMM routes of the data gradients)
VEC_AFFINE = {("mpn_conv_bwd_data_bn", 1), ("mpn_conv_bwd_data_bn", 2), ("mpn_conv_bwd_data_bn", 3), ("mpn_conv_bwd_data_bn_grouped", 1)}


def _rows():
    """(entry, layer, jobs, message to match): every defect of every entry on every route."""
    rows = []
    for name, (_, arrays, layers, required, aligned, f32, has_ksize, pairs, strides) in ENTRIES.items():
        for route, base in enumerate(layers):
            defects = [(f"{p}-null", "job", {p: None}) for p in required]
            defects += [(f"{p}-at-0x1008", "job", {p: 0x1008}) for p in aligned]
            if (name, route) in VEC_AFFINE:
                defects += [(f"{p}-at-0x1008", "job", {p: 0x1008}) for p in ("bn_scale", "bn_shift")]
            defects += [("Cin-20", "layer", {"Cin": 20}), ("dtype-7", "layer", {"dtype": 7}), ("N-0", "layer", {"N": 0}),
                        ("H-0", "job", {"H": 0}), ("W-0", "job", {"W": 0})]
            if f32:
                defects.append(("f32-Cin-6", "layer", {"Cin": 6, "dtype": F32}))
            if has_ksize:
                defects.append(("ksize-2", "layer", {"ksize": 2}))
            if pairs:
                defects.append(("scale-without-shift", "job", {"in_shift": None}))
            for s in strides:
                defects.append((f"{s}-below-channels", "job", {s: base[CHANNELS[s]] - 8}))
                defects.append((f"{s}-not-whole-vectors", "job", {s: base[CHANNELS[s]] + 4}))
            defects += [(f"{p}-array-null", "job", {p: "no array"}) for p in arrays]
            for what, scope, change in defects:
                for njobs in ((1, 2) if arrays else (1,)):
                    layer, jobs = dict(base, njobs=njobs), [_job(j) for j in range(njobs)]
                    (layer if scope == "layer" else jobs[-1]).update(change)
                    rows.append(pytest.param(name, layer, jobs, None, id=f"{name}-route{route}-{what}-of-{njobs}"))

    def one(name, what, layer, match=None, njobs=1, **job):
        jobs = [_job(j) for j in range(njobs)]
        jobs[-1].update(job)
        rows.append(pytest.param(name, dict(layer, njobs=njobs), jobs, match, id=f"{name}-{what}-of-{njobs}"))

    # the 16-bit 1x1 weight gradient addresses its tiles with 32-bit byte offsets: the same refusal from both entries
    big = dict(_layer(8, 8, 1), N=32)
    one("mpn_conv_bwd_weight", "2^31-bytes", big, "2\\^31 bytes", H=2048, W=2048)
    for njobs in (1, 2):
        one("mpn_conv_bwd_weight_grouped", "2^31-bytes", big, "2\\^31 bytes", njobs, H=2048, W=2048)
    # the data gradient with the reduction: a geometry no kernel covers, f32 storage, more jobs than a grid takes
    one("mpn_conv_bwd_data_bn", "K-128-C-1024", _layer(128, 1024, 3))
    one("mpn_conv_bwd_data_bn", "f32", _layer(64, 64, 3, F32))
    for njobs in (1, 2):
        one("mpn_conv_bwd_data_bn_grouped", "K-128-C-1024", _layer(128, 1024, 3), None, njobs)
        one("mpn_conv_bwd_data_bn_grouped", "f32", _layer(64, 64, 3, F32), None, njobs)
    one("mpn_conv_bwd_data_bn_grouped", "six-jobs", _layer(64, 64, 3), None, 6)
    one("mpn_conv_bwd_data_bn_grouped", "six-jobs-tiled", _layer(64, 24, 3), None, 6)
    # the fused thin 1x1 backward
    for name in ("mpn_conv1x1_bwd_fused", "mpn_conv1x1_bwd_fused_apply"):
        one(name, "dx-is-x", _layer(64, 64, 1), dx=_job(0)["x"])
        one(name, "dx-is-dy", _layer(64, 64, 1), dx=_job(0)["y"])
        one(name, "Cin-256", _layer(256, 64, 1))
    one("mpn_conv1x1_bwd_fused_apply", "Cin-128", _layer(128, 64, 1))
    # the upsample-add epilogue: 1x1 layers on even maps
    one("mpn_conv_fwd", "up_res-with-3x3", _layer(64, 64, 3), up_res=0x7000)
    one("mpn_conv_fwd", "up_res-with-odd-H", _layer(64, 64, 1), up_res=0x7000, H=15)
    one("mpn_conv_fwd", "up_res-into-the-GEMM-kernel", _layer(256, 256, 1), up_res=0x7000)
    return rows


@pytest.mark.parametrize("name, layer, jobs, match", _rows())
def test_one_defect_is_refused_before_any_hip_call(name, layer, jobs, match):
    with pytest.raises(ValueError, match=match):
        _lib.call(name, *ENTRIES[name][0](layer, jobs))


def test_the_table_covers_the_eight_entry_points_on_every_route():
    seen = {p.values[0] for p in _rows()}
    assert seen == set(ENTRIES) and len(seen) == 8
