"""GPU: the pixel reductions (weight gradients, A B^T, batch-norm slabs, slab reductions) on exact-integer inputs against the
int-valued float64 references of tests/exact_ref.py - by EQUALITY. With small-integer operands every product and every partial
sum is exactly representable in f32 in any summation order (each test asserts exact_headroom < 2^24 first), so a result that
differs in one bit is a lost pixel, a pixel counted twice, a wrong halo tap, a channel read from beyond Cin or a stale slab
row - never rounding. tests/test_reduction_exact_host.py proves what each case of the table is in it for.

Comparisons at a tolerance instead of equality (item 4 of the plan): none."""
import numpy as np
import pytest
import torch

import exact_ref as E

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
NAN = float("nan")
GUARD = 2          # slab rows of NaN behind the promised count


def _ops():
    from multiposenet_amd import ops
    return ops


def _dev(t, dtype=torch.float32):
    return t.to(dtype).contiguous().cuda()


def _sliced(t, dtype):
    """`t` as a channel slice of a tensor 16 channels wider whose other channels hold NaN."""
    C = t.shape[-1]
    wide = torch.full(tuple(t.shape[:-1]) + (C + 16,), NAN, dtype=dtype, device="cuda")
    wide[..., 8:8 + C] = t.to(dtype).cuda()
    return wide[..., 8:8 + C]


def _slab(rows, n):
    return torch.full(((rows + GUARD) * n,), NAN, device="cuda")


def _check_slab(slab, rows, n, what=""):
    """Exactly `rows` slabs are written (finite), nothing behind them is touched."""
    assert bool(torch.isfinite(slab[:rows * n]).all()), f"{what}: a promised slab row holds a non-finite value"
    assert bool(torch.isnan(slab[rows * n:]).all()), f"{what}: written behind the promised {rows} rows"


def _reduced(slab, rows, n):
    out = torch.full((n,), NAN, device="cuda")
    _ops().reduce_partials(slab, rows, n, out)
    return out


# ---------------------------------------------------------------------------------------------- a. mpn_conv_bwd_weight
CONV_PARAMS = [(c.name, dt, act, layout) for c in E.CONV_CASES for act in c.acts for dt in c.dtypes for layout in ("dense", "slice")]


@pytest.mark.parametrize("name,dt,act,layout", CONV_PARAMS, ids=["-".join(map(str, p)) for p in CONV_PARAMS])
def test_conv_wgrad_exact(cuda, name, dt, act, layout):
    ops = _ops()
    c, dtype = E.CONV_BY_NAME[name], DT[dt]
    d = E.conv_case_data(name, act)
    assert d.headroom < E.EXACT_LIMIT
    if layout == "slice":
        x, dy = _sliced(d.x, dtype), _sliced(d.dy, dtype)
    else:
        x, dy = _dev(d.x, dtype), _dev(d.dy, dtype)
    # (activation 0 still applies the integer affine; test_conv_wgrad_exact_without_an_affine passes no table at all)
    aff = ops.Affine(_dev(d.scale), _dev(d.shift), act)
    n = c.k * c.k * c.Cin * c.Cout
    rows = ops.conv_wgrad_num_parts(c.N, c.H, c.W, c.Cin, c.Cout, c.k, dtype)
    slab = _slab(rows, n)
    ops.conv_bwd_weight(x, dy, c.k, aff, None, part=slab, reduce=False)
    _check_slab(slab, rows, n, name)
    geom = E.geometry(c.k, c.Cin, c.Cout, dt)[1:]
    E.assert_exact(_reduced(slab, rows, n).view(c.k, c.k, c.Cin, c.Cout), d.want, geom)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "f32"])
@pytest.mark.parametrize("k,Cin,Cout", [(3, 64, 64), (1, 136, 200)])
def test_conv_wgrad_exact_without_an_affine(cuda, dt, k, Cin, Cout):
    """in_scale = in_shift = NULL: the raw x is the operand."""
    ops = _ops()
    N, H, W = 2, 21, 19
    rs = np.random.RandomState(k + Cin)
    x, dy = E.int_tensor(rs, (N, H, W, Cin), -E.X_MAX, E.X_MAX), E.int_tensor(rs, (N, H, W, Cout), -E.DY_MAX, E.DY_MAX)
    assert E.exact_headroom(E.conv_wgrad_ref, x, dy, ksize=k) < E.EXACT_LIMIT
    n = k * k * Cin * Cout
    rows = ops.conv_wgrad_num_parts(N, H, W, Cin, Cout, k, DT[dt])
    slab = _slab(rows, n)
    ops.conv_bwd_weight(_sliced(x, DT[dt]), _dev(dy, DT[dt]), k, None, None, part=slab, reduce=False)
    _check_slab(slab, rows, n)
    E.assert_exact(_reduced(slab, rows, n).view(k, k, Cin, Cout), E.conv_wgrad_ref(x, dy, k), E.geometry(k, Cin, Cout, dt)[1:])


# -------------------------------------------------------------------------------------- b. mpn_conv_bwd_weight_grouped
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", E.GROUPED_CASES, ids=[g[0] for g in E.GROUPED_CASES])
def test_conv_wgrad_grouped_exact(cuda, dt, case):
    """Every job's reduced slab equals that job's reference - the absolute statement, for grouped and single launches alike
    (test_ops_bwd_gpu.py::test_conv_wgrad_grouped_equals_separate_launches compares the two kernels with each other)."""
    ops = _ops()
    name, N, Cin, Cout, k, act, hws = case
    dtype = DT[dt]
    data = [E.conv_case_data(f"{name}/{j}", act, N, h, w, Cin, Cout, k) for j, (h, w) in enumerate(hws)]
    assert all(d.headroom < E.EXACT_LIMIT for d in data)
    xs = [_sliced(d.x, dtype) if j % 2 else _dev(d.x, dtype) for j, d in enumerate(data)]
    dys = [_dev(d.dy, dtype) if j % 2 else _sliced(d.dy, dtype) for j, d in enumerate(data)]
    affs = [ops.Affine(_dev(d.scale), _dev(d.shift), act) for d in data]
    nps = ops.conv_wgrad_grouped_num_parts(N, hws, Cin, Cout, k, dtype)
    n = k * k * Cin * Cout
    slabs = [_slab(r, n) for r in nps]
    ops.conv_bwd_weight_grouped(xs, dys, k, affs, slabs)
    for j, (d, slab, r) in enumerate(zip(data, slabs, nps)):
        _check_slab(slab, r, n, f"job {j}")
        try:
            E.assert_exact(_reduced(slab, r, n).view(k, k, Cin, Cout), d.want, E.geometry(k, Cin, Cout, dt)[1:])
        except AssertionError as e:
            raise AssertionError(f"job {j} ({hws[j]}, {r} slabs): {e}") from None


# ------------------------------------------------------------------------------- c. mpn_conv1x1_bwd_fused[_apply]
FUSED_PARAMS = [(c, ap) for c in E.FUSED1X1_CASES for ap in (False, True) if not (ap and c[3] > 64)]


@pytest.mark.parametrize("case,apply", FUSED_PARAMS, ids=[f"{c[3]}to{c[4]}_{c[0]}x{c[1]}x{c[2]}" + ("_apply" if a else "") for c, a in FUSED_PARAMS])
def test_conv1x1_bwd_fused_exact(cuda, case, apply):
    """wpart (reduced), the masked data gradient dx and the bn_part row sums, all by equality. The weights are in {-1, 0, 1} with
    8 nonzeros per input channel, so |dx| <= 256 (asserted from the reference) and dx is exact in bf16. The apply variant's
    dY = s * (g_masked - k1 - (y - mean) * invstd * k2) stays an exact small integer with s in {1, 2}, integer shift / mean / k1,
    invstd in {0.5, 1} and k2 in {-2, 0, 2} (exact_ref.fused1x1_case_data): such a choice exists, all three outputs are compared."""
    ops = _ops()
    N, H, W, Cin, Cout, act = case
    dtype = torch.bfloat16
    d = E.fused1x1_case_data(N, H, W, Cin, Cout, act, apply)
    assert d["headroom"] < E.EXACT_LIMIT and d["bn_headroom"] < E.EXACT_LIMIT and d["dx_bound"] <= 256
    assert ops.conv1x1_bwd_fused_supported(Cin, Cout, dtype)
    f = lambda v: _dev(v)
    bn = ops.BNState(torch.ones(Cin, device="cuda"), torch.zeros(Cin, device="cuda"), torch.zeros(Cin, device="cuda"), torch.ones(Cin, device="cuda"), act)
    bn.scale.copy_(f(d["scale"])); bn.shift.copy_(f(d["shift"]))
    x = _sliced(d["x"], dtype)
    rows = ops.conv_wgrad_num_parts(N, H, W, Cin, Cout, 1, dtype)
    wpart, bn_part = _slab(rows, Cin * Cout), _slab(rows, 2 * Cin)
    dx = torch.full((N, H, W, Cin), NAN, dtype=dtype, device="cuda")
    if apply:
        assert ops.conv1x1_bwd_fused_apply_supported(Cin, Cout, dtype)
        ap = d["ap"]
        own = ops.BNState(torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda"), torch.zeros(Cout, device="cuda"), torch.ones(Cout, device="cuda"), 2)
        for k_ in ("scale", "shift", "mean", "invstd", "k1", "k2"):
            getattr(own, k_).copy_(f(ap[k_]))
        g, y = _dev(d["g"], dtype), _sliced(d["y"], dtype)
        g0, y0 = g.clone(), y.clone()
        r = ops.conv1x1_bwd_fused(x, g, f(d["w"]), bn, dx, wpart, bn_part, apply_bn=own, y_raw=y)
        assert torch.equal(g, g0) and torch.equal(y, y0)
    else:
        r = ops.conv1x1_bwd_fused(x, _sliced(d["dy"], dtype), f(d["w"]), bn, dx, wpart, bn_part)
    assert r == rows
    _check_slab(wpart, rows, Cin * Cout, "wpart")
    _check_slab(bn_part, rows, 2 * Cin, "bn_part")
    E.assert_exact(_reduced(wpart, rows, Cin * Cout).view(1, 1, Cin, Cout), d["want_dw"], E.geometry(1, Cin, Cout, "bf16")[1:])
    E.assert_exact(dx, d["want_dx"])
    # the slab's row sums against sum g and sum g * x over the kernel's own stored dx (float64 on integers: exact)
    gd, xd = dx.double().reshape(-1, Cin).cpu(), d["x"].double().reshape(-1, Cin)
    sums = bn_part[:rows * 2 * Cin].view(rows, 2, Cin).double().sum(0).cpu()
    E.assert_exact(sums.float(), torch.stack([gd.sum(0), (gd * xd).sum(0)]))


# ------------------------------------------------------------------------------------- d. depthwise weight gradients
DW_PARAMS = [(c, s) for c in E.DW_CASES for s in (1, 2)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case,stride", DW_PARAMS, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}_s{s}" for c, s in DW_PARAMS])
def test_dwconv_wgrad_exact(cuda, dt, case, stride):
    """mpn_dwconv_bwd_weight and the wpart of mpn_dwconv_bwd_fused (stride 1) / mpn_dwconv_bwd_fused_s2 (stride 2, even H and W)."""
    ops = _ops()
    N, H, W, C = case
    dtype = DT[dt]
    d = E.dw_case_data(N, H, W, C, stride)
    assert d["headroom"] < E.EXACT_LIMIT
    x, dy = _dev(d["x"], dtype), _dev(d["dy"], dtype)
    aff = ops.Affine(_dev(d["scale"]), _dev(d["shift"]), 2)
    rows = ops.dwconv_wgrad_num_parts(N, H, W, C, stride, dtype)
    assert rows > 0
    slab = _slab(rows, 9 * C)
    ops.dwconv_bwd_weight(x, dy, stride, aff, None, part=slab, reduce=False)
    _check_slab(slab, rows, 9 * C, "dwconv_bwd_weight")
    E.assert_exact(_reduced(slab, rows, 9 * C).view(3, 3, C), d["want"])
    fused = stride == 1 or (H % 2 == 0 and W % 2 == 0)
    assert ops.dwconv_bwd_fused_supported(N, H, W, C, stride, dtype) == fused
    if not fused:
        return
    bn = ops.BNState(torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), 2)
    bn.scale.copy_(aff.scale); bn.shift.copy_(aff.shift); bn.mean.zero_(); bn.invstd.fill_(1.0)
    rs = np.random.RandomState(C + H)
    w = _dev(E.int_tensor(rs, (3, 3, C), -2, 2))
    for reduce_bn in (True, False):
        wpart = _slab(rows, 9 * C)
        ops.dwconv_bwd_fused(x, dy, w, bn, None, wpart=wpart, bn_part=_slab(rows, 2 * C) if reduce_bn else None, reduce=False,
                             reduce_bn=reduce_bn, stride=stride)
        _check_slab(wpart, rows, 9 * C, "dwconv_bwd_fused")
        E.assert_exact(_reduced(wpart, rows, 9 * C).view(3, 3, C), d["want"])


# --------------------------------------------------------------------------------------- e. mpn_stem_conv_bwd_weight
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C0", E.STEM_C0)
@pytest.mark.parametrize("N,H,W", E.STEM_MAPS)
def test_stem_wgrad_exact(cuda, dt, C0, N, H, W):
    """Float images in {0, 0.5, 1} (the u8 path scales by 1/255, which is not exact: it stays with the tolerance test)."""
    ops = _ops()
    dtype = DT[dt]
    d = E.stem_case_data(N, H, W, C0)
    assert d["headroom"] < E.EXACT_LIMIT
    rows = ops._lib.lib().mpn_stem_conv_wgrad_num_parts(N, H, W)
    slab = _slab(rows, 27 * C0)
    if C0 == 64 and dtype == torch.float32:       # the f32 build's VALU kernel keeps a 256 x C0 f32 tile in 64 KB of LDS
        with pytest.raises(ValueError, match="C0 too large"):
            ops.stem_conv_bwd_weight(_dev(d["img"]), _dev(d["dy"], dtype), None, part=slab, reduce=False)
        return
    ops.stem_conv_bwd_weight(_dev(d["img"]), _dev(d["dy"], dtype), None, part=slab, reduce=False)
    _check_slab(slab, rows, 27 * C0, "stem")
    E.assert_exact(_reduced(slab, rows, 27 * C0).view(3, 3, 3, C0), d["want"])


# ------------------------------------------------------------------------------------------- f. mpn_heatmap_head_bwd
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", E.HEAD_C)
@pytest.mark.parametrize("M", E.HEAD_M)
def test_heatmap_head_dw_db_exact(cuda, dt, C, M):
    ops = _ops()
    dtype = DT[dt]
    d = E.head_case_data(M, C)
    assert d["headroom"] < E.EXACT_LIMIT
    rs = np.random.RandomState(M + C)
    w = _dev(E.int_tensor(rs, (1, 1, C, 18), -1, 1))
    rows = ops._lib.lib().mpn_heatmap_head_bwd_num_parts(M)
    n = C * 18 + 18
    slab = _slab(rows, n)
    dA = torch.empty((1, 1, M, C), dtype=dtype, device="cuda")
    ops.heatmap_head_bwd(_dev(d["x"], dtype), _dev(d["dl"]), w, ops.Affine(_dev(d["scale"]), _dev(d["shift"]), 1), dA, None, part=slab, reduce=False)
    _check_slab(slab, rows, n, "head")
    E.assert_exact(_reduced(slab, rows, n), d["want"])


# ---------------------------------------------------------------------------------------------------- g. mpn_gemm_nt
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("M,N,K", E.GEMM_CASES)
def test_gemm_nt_exact(cuda, dt, M, N, K):
    ops = _ops()
    d = E.gemm_case_data(M, N, K)
    assert d["headroom"] < E.EXACT_LIMIT
    rows = ops.gemm_nt_num_parts(K)
    slab = _slab(rows, M * N)
    out = torch.full((M, N), NAN, device="cuda")
    ops.gemm_nt(_dev(d["a"], DT[dt]), _dev(d["b"], DT[dt]), out, slab)
    _check_slab(slab, rows, M * N, "gemm_nt")
    E.assert_exact(out, d["want"])


# ---------------------------------------------------------------------------------------- h. batch-norm partial slabs
def _row_sums(slab, rows, C):
    return slab[:rows * 2 * C].view(rows, 2, C).double().sum(0).cpu().float()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,C", [(M, C) for C in E.BN_C for M in E.BN_M if (M, C) in E.BN_MC])
def test_bn_slabs_exact(cuda, dt, C, M):
    """mpn_bn_stats (sum x, sum x^2) and mpn_bn_bwd_reduce (sum g, sum g * xhat; integer mean, power-of-two invstd): the slab's
    row sums by equality, rows behind the promised count untouched."""
    ops = _ops()
    dtype = DT[dt]
    d = E.bn_case_data(M, C, 2)
    assert d["headroom"] < E.EXACT_LIMIT
    rows = ops._lib.lib().mpn_bn_stats_num_parts(M)
    x, dA = _dev(d["x"], dtype), _dev(d["dA"], dtype)
    slab = _slab(rows, 2 * C)
    _, r = ops.bn_stats(x, slab)
    assert r == rows
    _check_slab(slab, rows, 2 * C, "bn_stats")
    E.assert_exact(_row_sums(slab, rows, C), d["want_stats"])
    bn = ops.BNState(torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), 2)
    for k_ in ("scale", "shift", "mean", "invstd"):
        getattr(bn, k_).copy_(_dev(d[k_]))
    slab = _slab(rows, 2 * C)
    assert ops.bn_bwd_reduce(bn, dA, x, slab) == rows
    _check_slab(slab, rows, 2 * C, "bn_bwd_reduce")
    E.assert_exact(_row_sums(slab, rows, C), d["want_bwd"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", E.BN_C)
def test_bn_bwd_reduce_grouped_exact(cuda, dt, C):
    """The row counts of the table (those E.BN_MC keeps for this C) as jobs of one grid, each with its own batch-norm; job 1 on
    channel slices of wider tensors where the grouped grid takes row strides."""
    ops = _ops()
    dtype = DT[dt]
    data = [E.bn_case_data(M, C, 1) for M in E.BN_M if (M, C) in E.BN_MC]
    assert all(d["headroom"] < E.EXACT_LIMIT for d in data)
    strided = C % (4 if dt == "f32" else 8) == 0 and 256 % (C // (4 if dt == "f32" else 8)) == 0     # bn_group_ok (csrc/bn.hip)
    bns, xs, dAs, slabs, rows = [], [], [], [], []
    for j, d in enumerate(data):
        bn = ops.BNState(torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), 1)
        for k_ in ("scale", "shift", "mean", "invstd"):
            getattr(bn, k_).copy_(_dev(d[k_]))
        bns.append(bn)
        sl = strided and j == 1
        xs.append(_sliced(d["x"], dtype) if sl else _dev(d["x"], dtype))
        dAs.append(_sliced(d["dA"], dtype) if sl else _dev(d["dA"], dtype))
        rows.append(ops._lib.lib().mpn_bn_stats_num_parts(d["x"].shape[0]))
        slabs.append(_slab(rows[-1], 2 * C))
    ops.bn_bwd_reduce_grouped(bns, dAs, xs, slabs)
    for j, d in enumerate(data):
        _check_slab(slabs[j], rows[j], 2 * C, f"job {j}")
        E.assert_exact(_row_sums(slabs[j], rows[j], C), d["want_bwd"])


# ------------------------------------------------------------------------- i. mpn_reduce_partials[_batched]
@pytest.mark.parametrize("n", [1000, 18 * 64 + 18 + 1], ids=["float4-rows", "scalar-rows"])
@pytest.mark.parametrize("rows", [1, 37, 4096, 4097])
def test_reduce_partials_exact(cuda, rows, n):
    ops = _ops()
    rs = np.random.RandomState(rows + n)
    part = E.int_tensor(rs, (rows, n), -100, 100)
    want = part.double().sum(0)
    assert float(part.abs().double().sum(0).max()) + 1000 < E.EXACT_LIMIT
    out = torch.full((n + 8,), NAN, device="cuda")
    ops.reduce_partials(_dev(part), rows, n, out[:n])
    E.assert_exact(out[:n], want)
    assert bool(torch.isnan(out[n:]).all())
    # accumulate, with a power-of-two scale
    out0 = E.int_tensor(rs, (n,), -1000, 1000)
    for scale in (0.5, 4.0):
        acc = _dev(out0)
        ops.reduce_partials(_dev(part), rows, n, acc, accumulate=True, scale=scale)
        E.assert_exact(acc, out0.double() + scale * want)
    acc = _dev(out0)
    ops.reduce_partials(_dev(part), rows, n, acc, accumulate=False, scale=0.25)
    E.assert_exact(acc, 0.25 * want)


def test_reduce_partials_batched_exact(cuda):
    """All the row counts and both row widths as jobs of ONE launch."""
    ops = _ops()
    rs = np.random.RandomState(11)
    shapes = [(r, n) for r in (1, 37, 4096, 4097) for n in (1000, 18 * 64 + 18 + 1, 4)]
    parts = [E.int_tensor(rs, s, -100, 100) for s in shapes]
    dparts = [_dev(p) for p in parts]
    outs = [torch.full((n + 8,), NAN, device="cuda") for _, n in shapes]
    ops.SlabReducer([(p, r, n, o[:n]) for p, (r, n), o in zip(dparts, shapes, outs)], "cuda:0").run()
    for p, dp, (r, n), o in zip(parts, dparts, shapes, outs):
        E.assert_exact(o[:n], p.double().sum(0))
        assert bool(torch.isnan(o[n:]).all()) and torch.equal(dp.cpu(), p)        # the batched kernel reads its slabs only
