"""GPU: the dense convolution's forward pass, data gradient and fused epilogues on exact-integer inputs against the float64
references of tests/exact_fwd_ref.py - by EQUALITY, on every kernel the launcher routes a layer to (the tiled MFMA kernel with
128- and 256-byte K rows, the persistent 3x3 kernel, its 64-channel-tile variant, the bf16 GEMM kernel).

Narrow regime: the outputs are integers of magnitude <= 256, the statistics rows and fused-reduction rows sums below 2^24 -
everything is exact. Wide regime: the outputs pass what the storage type holds, so the expected tensor is the float64 reference
ROUNDED ONCE; a partial sum that went through 16 bits, a residual added after the rounding or statistics of the unrounded sums
differ from it in thousands of elements (tests/test_forward_exact_host.py shows it on the CPU, and asserts every regime condition
and route claim of the tables).

Comparisons at a tolerance instead of equality: none."""
import pytest
import torch

import exact_fwd_ref as F
import exact_ref as E

pytestmark = pytest.mark.gpu
DT = F.TORCH_DT
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


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _slab_sums(part, rows, what=""):
    """The column sums (float64) of the `rows` rows a kernel promised - all of them written, nothing behind them touched."""
    assert 0 < rows <= part.shape[0] - GUARD, (what, rows)
    assert bool(torch.isfinite(part[:rows]).all()), f"{what}: a promised statistics row holds a non-finite value"
    assert bool(torch.isnan(part[rows:]).all()), f"{what}: written behind the promised {rows} rows"
    return part[:rows].double().sum(0).cpu()


def _promised_rows(c):
    """Statistics rows of a case by its route: the persistent kernels write one row per block that has a tile of the layer
    (min(16 x 16 tiles x channel tiles, compute units rounded down to the channel tiles) / channel tiles), the others one per
    8 x 16 (3x3) or 128-pixel (1x1) tile - so the count the library promises shows which kernel family the layer runs on."""
    if c.route not in ("c3", "c3-64"):
        return _ops().conv_num_parts(c.N, c.H, c.W, c.k)
    n_tiles = c.Cout // (64 if c.route == "c3-64" else 128)
    tiles = c.N * -(-c.H // 16) * -(-c.W // 16) * n_tiles
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return min(tiles, cus - cus % n_tiles) // n_tiles


def _run_conv(c, d, dt, with_stats, sliced=False):
    """One mpn_conv_fwd launch of case c on data d: output and slab prefilled with NaN. Returns (output, column sums or None)."""
    ops = _ops()
    dtype = DT[dt]
    pc = ops.PackedConv(_dev(d.w), dtype)
    assert pc.fwd.numel() == F.conv_route(c.k, c.Cin, c.Cout, dt)[1]
    aff = None if d.scale is None else ops.Affine(_dev(d.scale), _dev(d.shift), d.act)
    x = _sliced(d.x, dtype) if sliced else _dev(d.x, dtype)
    wide = torch.full((c.N, c.H, c.W, c.Cout + (16 if sliced else 0)), NAN, dtype=dtype, device="cuda")
    out = wide[..., 8:8 + c.Cout] if sliced else wide
    before = _bits(wide).clone()
    part = torch.full((ops.conv_num_parts(c.N, c.H, c.W, c.k) + GUARD, 2, c.Cout), NAN, device="cuda") if with_stats else None
    res = None if d.res is None else _dev(d.res, dtype)
    ops.conv_fwd(x, pc.fwd, c.Cout, c.k, aff, out=out, stats_part=part, up_res=res)
    if sliced:      # the neighbouring channels are untouched, bit for bit
        after = _bits(wide)
        assert torch.equal(after[..., :8], before[..., :8]) and torch.equal(after[..., 8 + c.Cout:], before[..., 8 + c.Cout:])
    sums = None
    if with_stats:
        rows = ops.conv_stats_rows(c.N, c.H, c.W, c.Cin, c.Cout, c.k, dtype)
        assert rows == _promised_rows(c), (c.name, c.route, rows)
        sums = _slab_sums(part, rows, c.name)
    return out, sums


def _check(c, dt, regime, sliced=False):
    d = F.fwd_case_data(c.name, regime, None if regime == "narrow" else dt)
    assert d.headroom < E.EXACT_LIMIT
    if regime == "narrow":
        want, with_stats = d.want, c.stats
        assert float(want.abs().max()) <= F.Y_MAX
    else:
        want, with_stats = F.once_rounded(d.want, dt), c.stats and F.wide_stats_for(c, dt)
        assert F.share_not_representable(d.want, dt) >= F.MIN_WIDE_SHARE
    out, sums = _run_conv(c, d, dt, with_stats, sliced)
    E.assert_exact(out, want)
    if with_stats:
        rounded = E.stats_ref(want)
        assert F.stats_headroom(want) < E.EXACT_LIMIT
        if regime == "wide":     # the two candidates differ, so the comparison decides between them
            assert not torch.equal(rounded, E.stats_ref(d.want))
        E.assert_exact(sums, rounded)      # the statistics are those of the ROUNDED outputs


# ------------------------------------------------------------------------------------------------- a. mpn_conv_fwd, per route
FWD_PARAMS = [(c.name, dt, regime) for c in F.FWD_CASES for regime in c.regimes for dt in c.dtypes if not (regime == "wide" and dt == "f32")]


@pytest.mark.parametrize("name,dt,regime", FWD_PARAMS, ids=["-".join(p) for p in FWD_PARAMS])
def test_conv_fwd_exact(cuda, name, dt, regime):
    """Output and statistics rows of every route in both regimes. c3-128to128-294tiles (6 x 112 x 112, more 16 x 16 tiles than
    compute units: some blocks walk two tiles and write one statistics row for both) is the largest case of the file."""
    c = F.FWD_BY_NAME[name]
    if name == "c3-128to128-294tiles":
        assert c.N * -(-c.H // 16) * -(-c.W // 16) > torch.cuda.get_device_properties(0).multi_processor_count
    _check(c, dt, regime)


# ---------------------------------------------------------------------------------------------- b. the upsample-add epilogue
UP_PARAMS = [(c.name, dt) for c in F.UP_CASES for dt in c.dtypes]


@pytest.mark.parametrize("name,dt", UP_PARAMS, ids=["-".join(p) for p in UP_PARAMS])
def test_conv_fwd_upsample_add_rounds_once(cuda, name, dt):
    """Wide data: the output is conv + nearest-2x(res) rounded ONCE (the residual goes into the f32 accumulators)."""
    c = F.UP_BY_NAME[name]
    d = F.fwd_case_data(name, "wide", dt)
    # the instrument sees the other order on this very data: rounding the convolution first gives another tensor
    conv = F.conv_fwd_ref(d.a, d.w, 1)
    late = F.once_rounded(F.once_rounded(conv, dt) + F.upsample2_ref(d.res.double()), dt)
    assert not torch.equal(late, F.once_rounded(d.want, dt))
    _check(c, dt, "wide")


# ---------------------------------------------------------------------------------------------------------- c. channel slices
SLICE_PARAMS = [("t3-40to72", "bf16", "wide"), ("c3-256to128", "fp16", "wide"), ("cs-512to64", "bf16", "narrow"),
                ("g-256to256-143px", "bf16", "wide"), ("t1-136to200", "fp16", "narrow"), ("u-64to128", "bf16", "wide")]


@pytest.mark.parametrize("name,dt,regime", SLICE_PARAMS, ids=["-".join(p) for p in SLICE_PARAMS])
def test_conv_fwd_exact_on_channel_slices(cuda, name, dt, regime):
    """x_stride / y_stride: input and output are the channels [8, 8 + C) of tensors 16 channels wider that hold NaN elsewhere. A
    read beyond the slice poisons the output; the output's neighbouring channels keep their bits."""
    _check(F.FWD_BY_NAME.get(name) or F.UP_BY_NAME[name], dt, regime, sliced=True)


# ------------------------------------------------------------------------------------- d. data gradients: PackedConv.bwd
DGRAD_PARAMS = [(k, Cin, Cout, dt, regime) for k, Cin, Cout, routes in F.DGRAD_CASES for dt in routes for regime in F.BOTH]


@pytest.mark.parametrize("k,Cin,Cout,dt,regime", DGRAD_PARAMS, ids=[f"{p[0]}x{p[0]}-{p[1]}to{p[2]}-{p[3]}-{p[4]}" for p in DGRAD_PARAMS])
def test_conv_dgrad_exact(cuda, k, Cin, Cout, dt, regime):
    """The forward kernels on the transposed packed weights (Cout -> Cin) equal conv_dgrad_ref on the layer's own weights."""
    ops = _ops()
    dtype = DT[dt]
    d = F.dgrad_case_data(k, Cin, Cout, regime, None if regime == "narrow" else dt)
    assert d.headroom < E.EXACT_LIMIT
    pc = ops.PackedConv(_dev(d.w), dtype)
    assert pc.bwd.numel() == F.conv_route(k, Cout, Cin, dt)[1]
    N, H, W = F.DGRAD_NHW
    dx = torch.full((N, H, W, Cin), NAN, dtype=dtype, device="cuda")
    ops.conv_fwd(_dev(d.dy, dtype), pc.bwd, Cin, k, out=dx)
    if regime == "narrow":
        assert float(d.want.abs().max()) <= F.Y_MAX
        E.assert_exact(dx, d.want)
    else:
        assert F.share_not_representable(d.want, dt) >= F.MIN_WIDE_SHARE
        E.assert_exact(dx, F.once_rounded(d.want, dt))


# ------------------------------------------------------------------------------------------------- e. mpn_conv_fwd_grouped
@pytest.mark.parametrize("case", F.GROUPED_CASES, ids=[g[0] for g in F.GROUPED_CASES])
def test_conv_fwd_grouped_exact(cuda, case):
    """Three pyramid levels in one launch, 280 tiles of 16 x 16 pixels ending in a one-tile level: on the persistent kernels a
    block walks from one job into the next. Every job's output equals its own reference and every job's rows sum to its own
    statistics (the 1x1 layer runs as the separate launches the entry point documents)."""
    ops = _ops()
    name, Cin, Cout, k, act, route = case
    dtype, N = torch.bfloat16, F.GROUPED_N
    data = [F.narrow_data(f"{name}/{j}", N, h, w, Cin, Cout, k, act) for j, (h, w) in enumerate(F.GROUPED_HW)]
    assert all(d.headroom < E.EXACT_LIMIT and F.stats_headroom(d.want) < E.EXACT_LIMIT for d in data)
    pcs = [ops.PackedConv(_dev(d.w), dtype) for d in data]
    affs = [ops.Affine(_dev(d.scale), _dev(d.shift), act) for d in data]
    xs = [_sliced(d.x, dtype) if j == 1 else _dev(d.x, dtype) for j, d in enumerate(data)]
    outs = [torch.full((N, h, w, Cout), NAN, dtype=dtype, device="cuda") for h, w in F.GROUPED_HW]
    parts = [torch.full((ops.conv_num_parts(N, h, w, k) + GUARD, 2, Cout), NAN, device="cuda") for h, w in F.GROUPED_HW]
    ops.conv_fwd_grouped(xs, [pc.fwd for pc in pcs], Cout, k, affs, outs, parts)
    for j, (d, (h, w)) in enumerate(zip(data, F.GROUPED_HW)):
        try:
            E.assert_exact(outs[j], d.want)
            E.assert_exact(_slab_sums(parts[j], ops.conv_stats_rows(N, h, w, Cin, Cout, k, dtype), f"job {j}"), E.stats_ref(d.want))
        except AssertionError as e:
            raise AssertionError(f"job {j} ({h} x {w}): {e}") from None


# ------------------------------------------------------------------------------ f. mpn_conv_bwd_data_bn[_grouped]
def _bnr_inputs(d, dtype, N, H, W, C, k, j=0):
    ops = _ops()
    bn = ops.Affine(_dev(d.scale), _dev(d.shift), d.act)
    x = _sliced(d.x, dtype) if j % 2 == 0 else _dev(d.x, dtype)      # the raw tensor as a channel slice (pixel stride C + 16)
    out = torch.full((N, H, W, C), NAN, dtype=dtype, device="cuda")
    part = torch.full(((ops.conv_num_parts(N, H, W, k) + GUARD) * 2 * C,), NAN, device="cuda")
    return bn, x, out, part


def _bnr_check(d, out, part, rows, C, what):
    assert d.headroom < E.EXACT_LIMIT and d.rows_headroom < E.EXACT_LIMIT and float(d.dx.abs().max()) <= F.Y_MAX
    E.assert_exact(out, d.g)                                           # the masked gradient: ReLU6 clips at both ends
    E.assert_exact(_slab_sums(part.view(-1, 2, C), rows, what), d.rows)   # sum g and sum g * x with the RAW x


BNR_PARAMS = [(c, dt) for c in F.BNR_CASES for dt in (("bf16", "fp16") if c[7] == "c3" else ("bf16",))]


@pytest.mark.parametrize("case,dt", BNR_PARAMS, ids=[f"{c[0]}-{dt}" for c, dt in BNR_PARAMS])
def test_conv_bwd_data_bn_exact(cuda, case, dt):
    """dx masked by the fed layer's activation and the reduced rows, exact, on the tiled, GEMM and persistent 3x3 routes."""
    ops = _ops()
    name, N, H, W, K, C, k, route = case
    dtype = DT[dt]
    assert ops.conv_bwd_data_bn_supported(K, C, k, dtype)
    d = F.bnr_case_data(name, N, H, W, K, C, k)
    pc = ops.PackedConv(_dev(d.w), dtype)
    bn, x, out, part = _bnr_inputs(d, dtype, N, H, W, C, k)
    rows = ops.conv_bwd_data_bn(_dev(d.dy, dtype), pc.bwd, C, k, bn, x, out, part)
    _bnr_check(d, out, part, rows, C, name)


@pytest.mark.parametrize("case", [c for c in F.BNR_CASES if c[6] == 3], ids=[c[0] for c in F.BNR_CASES if c[6] == 3])
def test_conv_bwd_data_bn_grouped_exact(cuda, case):
    """Three jobs (ragged tiles, one smaller than a tile) in one grid, each with its own batch-norm and slab."""
    ops = _ops()
    name, _, _, _, K, C, k, route = case
    dtype, N = torch.bfloat16, F.BNR_GROUPED_N
    assert ops.conv_bwd_data_bn_supported(K, C, 3, dtype)
    data = [F.bnr_case_data(f"{name}/{j}", N, h, w, K, C, k) for j, (h, w) in enumerate(F.BNR_GROUPED_HW)]
    pcs = [ops.PackedConv(_dev(d.w), dtype) for d in data]
    ins = [_bnr_inputs(d, dtype, N, h, w, C, k, j) for j, (d, (h, w)) in enumerate(zip(data, F.BNR_GROUPED_HW))]
    rows = ops.conv_bwd_data_bn_grouped([_dev(d.dy, dtype) for d in data], [pc.bwd for pc in pcs], C, [i[0] for i in ins],
                                        [i[1] for i in ins], [i[2] for i in ins], [i[3] for i in ins])
    for j, d in enumerate(data):
        _bnr_check(d, ins[j][2], ins[j][3], rows[j], C, f"{name} job {j}")
