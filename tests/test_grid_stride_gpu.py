"""GPU: the streaming kernels PAST their grid caps, against float64 references.

Every element-wise and reduction kernel at the tail of the training step launches a capped grid and walks the rest of its
tensor in a grid-stride loop, most of them with several vectors in flight per iteration, a clamped load and a guarded store
for the last, partly out-of-range piece. The other modules compare these kernels with a reference inside their FIRST
iteration only; tests/test_fullsize_gpu.py runs the production sizes but asserts self-consistency, which a kernel that skips
or repeats part of its second iteration in the same way on every run passes. Here every size is chosen by one rule:

    n > one full grid stride at today's cap, and (n mod stride) is not a whole number of a block's per-iteration pieces

so that a first, (where it is cheap) a middle and a partial last iteration exist. CAPS restates the caps; `_iterations` asserts
the rule for each chosen size, and where the library exports a block count the test asserts that the count IS the cap - a
change of a cap then fails here instead of silently moving a case back into the first iteration.

References are float64 (numpy, torch on the CPU; for the two largest cases chunked torch.float64 arithmetic on the device,
which shares no code with the kernels)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as E
from oracle import network as onet
from oracle import prn_post as oprn
from util import DTYPES, act_ref, assert_close, dev, nchw, nhwc, rnd, tol

pytestmark = pytest.mark.gpu
IDS = ["f32", "bf16"]
NAN = float("nan")

# what ONE full grid stride covers at the cap, the piece a block takes per iteration (same unit), where the cap is set
CAPS = {
    "loss": (768 * 256, 256, "pixels: mpn_keypoint_loss_num_parts, csrc/loss.hip (768 blocks x 256 threads)"),
    "adam": (4096 * 512, 512, "float4: mpn_adam_step[_cast], csrc/optim.hip (4096 blocks x U = 2 pieces of 256 float4)"),
    "axpy": (2048 * 256, 256, "floats: mpn_axpy, csrc/optim.hip (2048 blocks)"),
    "reduce": (2048 * 256, 256, "float4 per row: mpn_reduce_partials, csrc/optim.hip (bx <= 2048)"),
    "bn_act_apply": (4096 * 256, 256, "16-byte vectors: stream_blocks, csrc/bn.hip (4096 blocks)"),
    "bn_stats": (2048 * 128, 128, "rows: mpn_bn_stats_num_parts, csrc/bn.hip (2048 blocks of 128 rows, more rows per block above)"),
    "bn_bwd_apply": (16384 * 1024, 1024, "16-byte vectors: kApplyBlocks, csrc/bn.hip (16 384 blocks x 4 pieces of 256 vectors)"),
    "pool": (8192 * 256, 256, "16-byte vectors: blocks_for, csrc/resize.hip (8192 blocks): sumpool2x2, add_inplace"),
    "slice": (4096 * 1024, 256, "16-byte vectors: mpn_bilinear_up_fwd / _bwd at upsample 1, csrc/resize.hip (4096 blocks x 4 "
                                "vectors per thread, one grid width apart)"),
    "crop": (16384 * 256, 256, "elements: mpn_prn_crop, csrc/prn_post.hip (16 384 blocks)"),
}
L2_MAX_TENSORS, L2_CHUNK = 96, 16384      # kL2Max, kL2Chunk of mpn_l2_loss_batched, csrc/optim.hip


def _iterations(n, key, partial=True):
    """Grid-stride iterations of `n` units at the cap of CAPS[key]; asserts the size rule (partial=False: a shape the plan
    fixes whose remainder is a whole number of pieces - the case beside it supplies the partial piece)."""
    stride, piece, where = CAPS[key]
    assert n > stride, f"{n} does not get past one grid stride of {stride} ({where})"
    assert not partial or (n % stride) % piece != 0, f"{n}: the last iteration ends on a whole piece of {piece} ({where})"
    return -(-n // stride)


def _ops():
    from multiposenet_amd import ops
    return ops


def _lib():
    from multiposenet_amd import _lib as L
    return L.lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _assert_allclose_on_device(got, want64, rtol, atol, what):
    """np.testing.assert_allclose's statement |got - want| <= atol + rtol * |want|, evaluated in float64 on the device
    (the arrays here have up to 16.8 M elements)."""
    want = torch.as_tensor(want64).cuda()
    err = (got.double() - want).abs()
    bad = ~(err <= atol + rtol * want.abs())
    nbad = int(bad.sum())
    assert nbad == 0, (f"{what}: {nbad} of {bad.numel()} outside rtol {rtol:g} / atol {atol:g}; first at {int(bad.nonzero()[0])}, "
                       f"max |err| {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e}")


# ------------------------------------------------------------------------------------------- 1. keypoint loss and gradients
SATURATED = (-100.0, -40.0, -30.0, 30.0, 40.0, 100.0)
LOSS_SHAPES = [(3, 384, 384), (2, 264, 400), (3, 264, 328), (2, 16, 24)]
LOSS_CP = 8               # channels of the p2..p5 tensors (the kernel reads channel 0 at stride Cp)


def _loss_inputs(B, h, w, dtype):
    rs = np.random.RandomState(B * 1000 + h)
    hm = (rs.rand(B, h, w, 17) * 0.9).astype(np.float32)
    for b in range(B):
        for _ in range(6):
            hm[b, rs.randint(h), rs.randint(w), rs.randint(17)] = 1.0
    lmask = (rs.rand(B, h, w) < 0.9).astype(np.float32)
    dead = 1 if B == 3 else 0                       # one image without a single live pixel; the others reach every iteration
    lmask[dead] = 0.0
    logits = (rs.randn(B, h, w, 18) * 2).astype(np.float32)
    for val in SATURATED:                           # saturated logits on positive and on negative labels, at live pixels
        for b in (i for i in range(B) if i != dead):
            for positive in (True, False):
                for _ in range(2):
                    y, x, c = rs.randint(h), rs.randint(w), rs.randint(17)
                    logits[b, y, x, c] = val
                    hm[b, y, x, c] = 1.0 if positive else 0.45
                    lmask[b, y, x] = 1.0
    lab = {"heatmaps": hm, "loss_masks": lmask, "segmentation_masks": (rs.rand(B, h, w) < 0.3).astype(np.float32),
           "num_boxes": np.array([3, 5, 0] if B == 3 else [0, 3], np.int32)}
    ps = [rnd(rs.randn(B, h >> k, w >> k, LOSS_CP), dtype) for k in range(4)]
    return logits, lab, ps


def _loss_reference(logits, lab, ps, T=torch.float64):
    """oracle.network.losses_fn / per_pixel_reg_loss and autograd in precision T: eight losses, dlogits, [d p_l[..., 0]]."""
    lg = torch.tensor(logits, dtype=T, requires_grad=True)
    pp = [p.to(T).requires_grad_(True) for p in ps]
    tl = {k: torch.tensor(v) if k == "num_boxes" else torch.tensor(v, dtype=T) for k, v in lab.items()}
    total, losses = onet.losses_fn(lg, {f"p{l}": pp[l - 2] for l in range(2, 6)}, tl)
    total.backward()
    want = [float(v.detach()) for v in losses.values()] + [float(total.detach()), float(onet.per_pixel_reg_loss(lg.detach(), tl))]
    return np.array(want, np.float64), lg.grad, [p.grad[..., 0] for p in pp]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,h,w", LOSS_SHAPES, ids=["x".join(map(str, s)) for s in LOSS_SHAPES])
def test_keypoint_loss_past_the_block_cap(cuda, dtype, B, h, w):
    """mpn_keypoint_loss against the float64 oracle with autograd. Cap: 768 blocks x 256 px = 196 608 px per grid stride.
      3 x 384 x 384 = 442 368 px: 3 iterations (2.25 strides; the remainder is a whole 192 blocks, as the plan fixes it)
      2 x 264 x 400 = 211 200 px: 2 iterations (the remainder is a whole 57 blocks)
      3 x 264 x 328 = 259 776 px: 2 iterations, the last ends inside a block (246 blocks and 192 px)
      2 x 16 x 24: the 3-block case of test_ops_fwd_gpu.py, here against float64
    num_boxes differs per image and includes 0, one image has loss_mask == 0 everywhere, logits of +-30, +-40, +-100 sit on
    positive and negative labels (the float64 oracle is finite there, value and gradient). Tolerances of
    test_keypoint_loss_and_gradients: rtol 2e-5 on the eight losses, assert_close(f32, scale = max |grad|) on the gradients
    (measured on these inputs: the kernel's losses lie within 9e-8 relative of the float64 oracle at every shape, the f32 torch
    oracle's within 1.7e-7 - the bounds of the f32 comparison hold against float64 unchanged).
    Every output is preset to NaN (an element no iteration writes fails), and a second call is bit-identical."""
    ops = _ops()
    small = B * h * w <= CAPS["loss"][0]
    if not small:
        _iterations(B * h * w, "loss", partial=(B, h, w) == (3, 264, 328))
        assert _lib().mpn_keypoint_loss_num_parts(B, h, w) == 768           # the cap guard
    logits, lab, ps = _loss_inputs(B, h, w, dtype)
    want, want_dl, want_daux = _loss_reference(logits, lab, ps)
    assert np.isfinite(want).all() and bool(torch.isfinite(want_dl).all())
    dlab = {k: dev(v) for k, v in lab.items()}
    dlogits, dps = dev(logits), [dev(p, dtype) for p in ps]
    runs = []
    for _ in range(2):
        dl = torch.full((B, h, w, 18), NAN, device="cuda")
        daux = [torch.full((B, h >> k, w >> k), NAN, device="cuda") for k in range(4)]
        out = ops.keypoint_loss(dlogits, dlab, dps, dl, daux).clone()
        runs.append((out, dl, daux))
    (out, dl, daux), (out2, dl2, daux2) = runs
    got = out.cpu().numpy().astype(np.float64)
    print(f"keypoint loss {B}x{h}x{w} {IDS[DTYPES.index(dtype)]}: |got / want - 1| of the eight losses "
          f"{np.array2string(np.abs(got / want - 1), precision=2)}")
    np.testing.assert_allclose(got[:7], want[:7], rtol=2e-5)
    np.testing.assert_allclose(got[7], want[7], rtol=2e-5)
    assert_close(dl, want_dl, torch.float32, scale=float(want_dl.abs().max()))
    for k in range(4):
        assert_close(daux[k], want_daux[k], torch.float32, scale=float(want_daux[k].abs().max()) or 1.0)
    assert torch.equal(out, out2) and torch.equal(dl, dl2) and all(torch.equal(a, b) for a, b in zip(daux, daux2))


# --------------------------------------------------------------------------------------------------------------- 2. Adam
ADAM_STRIDE = CAPS["adam"][0]                                        # 2 097 152 float4 = 8 388 608 floats
ADAM_SIZES = [4 * (2 * ADAM_STRIDE + 3 * 512 + 100), 4 * (ADAM_STRIDE + 357)]


def _adam_inputs(n):
    """f32 CPU tensors p, g, m, v: gradients that clip at +200 and -200 after grad_scale = 0.5 (std 150, and +-1e4 planted),
    and entries with g = m = v = 0, at the start, on both sides of every grid-stride boundary and inside the last piece.
    m starts with the sign of g: the kernel rounds (1 - beta1) to f32 as TF does (2.4e-7 relative), and where
    beta1 m and (1 - beta1) g cancel, that rounding of a term of up to 20 stands against an m near 0 - no tolerance relative to
    m covers it. test_adam_matches_tf_semantics, whose tolerances these are, starts from m = 0 and cannot cancel either."""
    gen = _gen(n % 1000003)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 300.0
    m = torch.randn(n, generator=gen).abs() * 0.1
    v = torch.rand(n, generator=gen) * 1e-2
    S = 4 * ADAM_STRIDE
    marks = [0, 1029, n - 4 * 50, n - 4] + [k * S + d for k in range(1, n // S + 1) for d in (-5, 0, 7)]
    for i in marks:                                                  # four entries each: +clip, -clip, g = m = v = 0, g = 0 alone
        g[i], g[i + 1], g[i + 2], g[i + 3] = 1e4, -1e4, 0.0, 0.0
        m[i + 2] = v[i + 2] = 0.0
    m = torch.where(g < 0, -m, m)
    return p, g, m, v


@pytest.mark.parametrize("n", ADAM_SIZES, ids=["3-iterations-second-piece-out-of-range", "2-iterations-second-piece-partly-in-range"])
def test_adam_past_the_block_cap(cuda, n):
    """mpn_adam_prepare + mpn_adam_step for three steps against oracle.network.adam_step / cosine_decay in float64.
    Cap: 4096 blocks x 512 float4 = 2 097 152 float4 (8 388 608 floats) per grid stride.
      n = 4 (2 * 2 097 152 + 3 * 512 + 100) = 16 783 760: 3 iterations; the last block of the last one holds 100 <= 256 float4,
          its second unrolled piece is wholly out of range (the clamped load) and the first is cut by the guarded store
      n = 4 (2 097 152 + 357) = 8 390 036: 2 iterations; 357 > 256, the second piece is partly in range
    Gradients clip on both sides, grad_scale = 0.5, entries with g = 0 and v = 0. Tolerances of test_adam_matches_tf_semantics:
    p and m at rtol 1e-5 / atol 1e-7, v at rtol 1e-4 ((1 - beta2) is rounded in f32, as in TF)."""
    ops = _ops()
    n4 = n // 4
    assert _iterations(n4, "adam") == (3 if n == ADAM_SIZES[0] else 2)
    assert (n4 % 512 <= 256) == (n == ADAM_SIZES[0])
    p, g, m, v = _adam_inputs(n)
    dp, dg, dm, dv = dev(p), dev(g), dev(m), dev(v)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    hyper = torch.zeros(4, device="cuda")
    p64, m64, v64 = p.double().numpy(), m.double().numpy(), v.double().numpy()
    g64 = g.double().numpy() * 0.5
    assert (g64 > 200).any() and (g64 < -200).any() and ((g64 == 0) & (v64 == 0)).any()
    for it in range(3):
        ops.adam_prepare(step, hyper, 3e-4, 200000)
        ops.adam_step(dp, dg, dm, dv, hyper, grad_scale=0.5)
        lr = onet.cosine_decay(3e-4, it, 200000)
        onet.adam_step(p64, g64, m64, v64, lr, it + 1)
        assert int(step.item()) == it + 1
        np.testing.assert_allclose(float(hyper[1]), lr, rtol=1e-6)
        _assert_allclose_on_device(dp, p64, 1e-5, 1e-7, f"p after step {it + 1}")
        _assert_allclose_on_device(dm, m64, 1e-5, 1e-7, f"m after step {it + 1}")
        _assert_allclose_on_device(dv, v64, 1e-4, 0.0, f"v after step {it + 1}")
    assert torch.equal(dg.cpu(), g)                                   # the gradients are read only


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_adam_step_cast_past_the_block_cap(cuda, dtype):
    """mpn_adam_step_cast at n = 16 783 760 (3 iterations of 2 097 152 float4, see test_adam_past_the_block_cap): bit-equal to
    mpn_adam_step, the ranges equal to `.to(dtype)` of the updated arena, guard elements untouched. The ranges: one across the
    first grid-stride boundary, one across the second, one that ends with the arena inside the last, cut piece, one at 0."""
    ops = _ops()
    n = ADAM_SIZES[0]
    _iterations(n // 4, "adam")
    S = 4 * ADAM_STRIDE
    gen = _gen(5)
    p0 = dev(torch.randn(n, generator=gen))
    g = dev(torch.randn(n, generator=gen) * 0.01)
    m0 = dev(torch.randn(n, generator=gen) * 0.01)
    v0 = dev(torch.rand(n, generator=gen) * 1e-4)
    hyper = dev(np.array([1e-3, 1e-3, 0, 0], np.float32))
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    ops.adam_step(p1, g, m1, v1, hyper, grad_scale=0.5, clip=float("inf"))
    ranges = [(0, 1024), (S - 4 * 300, 4 * 1000), (2 * S - 4 * 256, 4 * 700), (n - 4 * 150, 4 * 150)]
    dsts = [torch.full((c + 8,), 7.0, dtype=dtype, device="cuda") for _, c in ranges]      # 8 guard elements behind each
    jobs = ops.AdamCastJobs([(o, c, d[:c]) for (o, c), d in zip(ranges, dsts)])
    p2, m2, v2 = p0.clone(), m0.clone(), v0.clone()
    ops.adam_step_cast(p2, g, m2, v2, hyper, jobs, grad_scale=0.5, clip=float("inf"))
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    for a, b in ((0, S), (S, 2 * S), (2 * S, n)):                      # each iteration's span moved (not skipped by both kernels):
        assert float((v0[a:b] == v2[a:b]).float().mean()) < 1e-2       # v = beta2 v + (1 - beta2) g^2 stands still only by rounding
    for (o, c), d in zip(ranges, dsts):
        assert torch.equal(d[:c], p2[o:o + c].to(dtype))
        assert bool((d[c:] == 7.0).all())


@pytest.mark.parametrize("gs", [199999, 200000, 200005], ids=["last-decay-step", "at-decay-steps", "past-decay-steps"])
def test_adam_prepare_at_the_end_of_the_decay(cuda, gs):
    """mpn_adam_prepare with the step preset to decay_steps - 1, decay_steps and decay_steps + 5: lr = the oracle's cosine_decay
    (3e-8 from decay_steps on), lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) in float64, both at rtol 1e-6."""
    ops = _ops()
    step = torch.full((1,), gs, dtype=torch.int64, device="cuda")
    hyper = torch.zeros(4, device="cuda")
    ops.adam_prepare(step, hyper, 3e-4, 200000)
    lr, t = onet.cosine_decay(3e-4, gs, 200000), gs + 1
    if gs >= 200000:
        assert math.isclose(lr, 3e-8, rel_tol=1e-12)
    assert int(step.item()) == t
    np.testing.assert_allclose(float(hyper[1]), lr, rtol=1e-6)
    np.testing.assert_allclose(float(hyper[0]), lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------- 3. reductions, exact
@pytest.mark.parametrize("rows,n", [(9, 2097152 + 4000), (101, 102400)], ids=["9-rows-past-the-cap", "101-rows-in-10-uneven-slices"])
def test_reduce_partials_exact_under_grid_stride_and_in_slices(cuda, rows, n):
    """mpn_reduce_partials on small integers, by equality (tests/exact_ref.py), plain / accumulate / scale.
      9 rows of 2 101 152 floats = 525 288 float4: bx is capped at 2048 blocks = 524 288 float4 per grid stride, 2 iterations
          (the last: 3 blocks and 232 float4); 1024 / bx = 0 slices, so MODE 0 runs under the grid stride
      101 rows of 102 400 floats: bx = 100, nslices = 10: MODE 1 over row ranges of 10, ..., 10, 11 rows, then MODE 2"""
    ops = _ops()
    if rows == 9:
        assert _iterations(n // 4, "reduce") == 2
    else:
        bx = -(-(n // 4) // 256)
        assert bx == 100 and min(1024 // bx, 16, rows // 8) == 10 and rows % 10 != 0
    rs = np.random.RandomState(rows)
    part = E.int_tensor(rs, (rows, n), -100, 100)
    want = part.double().sum(0)
    assert float(part.abs().double().sum(0).max()) * 4 + 1000 < E.EXACT_LIMIT
    dpart = part.cuda()
    out = torch.full((n + 8,), NAN, device="cuda")
    ops.reduce_partials(dpart.clone(), rows, n, out[:n])                 # (pass 1 of the sliced path folds sums INTO the slab)
    E.assert_exact(out[:n], want)
    assert bool(torch.isnan(out[n:]).all())
    out0 = E.int_tensor(rs, (n,), -1000, 1000)
    for scale in (0.5, 4.0):
        acc = out0.cuda()
        ops.reduce_partials(dpart.clone(), rows, n, acc, accumulate=True, scale=scale)
        E.assert_exact(acc, out0.double() + scale * want)
    acc = out0.cuda()
    ops.reduce_partials(dpart.clone(), rows, n, acc, accumulate=False, scale=0.25)
    E.assert_exact(acc, 0.25 * want)


def test_axpy_exact_past_the_block_cap(cuda):
    """mpn_axpy at n = 2 * 524 288 + 12 345 = 1 060 921: the cap is 2048 blocks x 256 = 524 288 floats per grid stride, so 3
    iterations, the last of 48 blocks and 57 floats. Integer data and a = 0.25: y + a x is exact in f32 - equality with numpy."""
    ops = _ops()
    n = 2 * 524288 + 12345
    assert _iterations(n, "axpy") == 3
    rs = np.random.RandomState(21)
    x, y = rs.randint(-1000, 1001, n).astype(np.float32), rs.randint(-1000, 1001, n).astype(np.float32)
    want = y.astype(np.float64) + 0.25 * x.astype(np.float64)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    dx = dev(x)
    buf = torch.full((n + 8,), NAN, device="cuda")
    buf[:n] = dev(y)
    ops.axpy(0.25, dx, buf[:n])
    np.testing.assert_array_equal(buf[:n].cpu().numpy(), want.astype(np.float32))
    assert bool(torch.isnan(buf[n:]).all()) and np.array_equal(dx.cpu().numpy(), x)


# ------------------------------------------------------------------------------------------------ 4. weight-decay sums
L2_SIZES = [1, 16384, 16385, 50000]


def _l2_tensors():
    rs = np.random.RandomState(31)
    sizes = L2_SIZES + [int(s) for s in rs.randint(1, 40000, size=96)]
    ws = [(rs.randn(n) * 0.1).astype(np.float32) for n in sizes]
    ws[0][0] = 30.0            # the one-element tensor and the 16 385th element (a block of its own) carry weight in the sum:
    ws[2][16384] = 25.0        # dropping either moves the result by 1e-2 relative
    return sizes, ws


def test_l2_loss_batch_and_single_tensor_sums(cuda):
    """First operator-level test of mpn_l2_loss_batched (ops.L2LossBatch) and mpn_l2_loss_accumulate. 100 tensors = two launches
    (96 + 4 jobs at kL2Max = 96) of 16 384-element blocks; sizes 1, 16 384 (one block), 16 385 (a second block of ONE
    element), 50 000 (4 blocks; 49 iterations of the single-block kernel's 1024 threads) and 96 ragged ones. The kernels
    accumulate in f64 and round once: acc + scale * sum w^2 / 2 in float64 at rtol 1e-6, acc preset to a nonzero value; the
    batch equals the sum of the single-tensor calls at the same tolerance; a repeat run is bit-identical."""
    ops = _ops()
    sizes, ws = _l2_tensors()
    assert len(ws) == 100 > L2_MAX_TENSORS and all(s in sizes for s in (1, L2_CHUNK, L2_CHUNK + 1))
    scale = float(np.float32(5e-5))                                       # (the C ABI takes the scale as f32)
    each = np.array([scale * 0.5 * float((w.astype(np.float64) ** 2).sum()) for w in ws])
    dws = [dev(w) for w in ws]
    batch = ops.L2LossBatch(dws)
    results = []
    for _ in range(2):
        acc = torch.full((1,), 0.75, device="cuda")
        batch.run(scale, acc)
        results.append(acc)
    np.testing.assert_allclose(float(results[0]), 0.75 + each.sum(), rtol=1e-6)
    assert torch.equal(results[0], results[1])
    # single tensors, each into an accumulator of its own: from zero (their sum = the batch) ...
    accs = torch.zeros(len(ws), device="cuda")
    for t, w in enumerate(dws):
        ops.l2_loss_accumulate(w, scale, accs[t:t + 1])
    np.testing.assert_allclose(accs.cpu().numpy().astype(np.float64), each, rtol=1e-6)
    np.testing.assert_allclose(float(results[0]), 0.75 + float(accs.double().sum()), rtol=1e-6)
    # ... and on top of a preset value
    pre = torch.full((len(L2_SIZES),), 0.75, device="cuda")
    for t in range(len(L2_SIZES)):
        ops.l2_loss_accumulate(dws[t], scale, pre[t:t + 1])
    np.testing.assert_allclose(pre.cpu().numpy().astype(np.float64), 0.75 + each[:len(L2_SIZES)], rtol=1e-6)
    for w, d in zip(ws, dws):
        assert np.array_equal(d.cpu().numpy(), w)


# ----------------------------------------------------------------------------------------------- 5. batch-norm streams
BN_FWD_CASES = [(70001, 64, torch.float32, 2), (140001, 64, torch.bfloat16, 2), (180001, 24, torch.float32, 1),
                (360001, 24, torch.bfloat16, 2), (140001, 64, torch.float32, 1)]


@pytest.mark.parametrize("M,C,dtype,act", BN_FWD_CASES, ids=[f"{M}x{C}-{IDS[DTYPES.index(dt)]}" for M, C, dt, _ in BN_FWD_CASES])
def test_bn_stats_finalize_apply_past_the_caps(cuda, M, C, dtype, act):
    """The statement and tolerances of test_ops_fwd_gpu.py::test_bn_stats_finalize_apply at row counts past the caps.
    bn_act_apply: 4096 blocks x 256 = 1 048 576 vectors per grid stride.
       70 001 x 64 f32  = 1 120 016 vectors (16 per row): 2 iterations        140 001 x 64 bf16 = 1 120 008 (8 per row): 2
      180 001 x 24 f32  = 1 080 006 (6 per row; 1 048 576 % 6 != 0: a thread's channels change with the iteration): 2
      360 001 x 24 bf16 = 1 080 003 (3 per row): 2                           140 001 x 64 f32  = 2 240 016: 3 (first, middle, cut)
    bn_stats: 2048 blocks of 128 rows = 262 144 rows; 360 001 rows is past it: the block count is AT the cap and a block walks
    176 rows (more than the 128 of every other test); 180 001 rows: 1407 blocks of 128."""
    ops = _ops()
    ve = 4 if dtype == torch.float32 else 8
    assert _iterations(M * (C // ve), "bn_act_apply") == (3 if (M, C, dtype) == (140001, 64, torch.float32) else 2)
    nblocks = _lib().mpn_bn_stats_num_parts(M)
    if M > CAPS["bn_stats"][0]:
        assert nblocks == 2048 and -(-M // nblocks) > 128               # the cap guard
    rs = np.random.RandomState(C)
    x = (torch.randn((1, 1, M, C), generator=_gen(M)) * 2 + 0.7).to(dtype).float()
    g, b = rs.rand(C).astype(np.float32) + 0.5, rs.randn(C).astype(np.float32)
    mm, mv = rs.randn(C).astype(np.float32), rs.rand(C).astype(np.float32) + 0.5
    bn = ops.BNState(dev(g), dev(b), dev(mm), dev(mv), act)
    dx = dev(x, dtype)
    part, nparts = ops.bn_stats(dx)
    assert nparts == nblocks
    ops.bn_finalize(bn, part, nparts, M, training=True)
    xd = x.double().reshape(M, C)
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    np.testing.assert_allclose(bn.mean.cpu().numpy(), mean.numpy(), atol=2e-6 * 10)
    np.testing.assert_allclose(bn.invstd.cpu().numpy(), (1 / torch.sqrt(var + 1e-3)).numpy(), rtol=2e-5)
    np.testing.assert_allclose(bn.moving_mean.cpu().numpy(), mm * 0.95 + mean.numpy() * 0.05, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bn.moving_var.cpu().numpy(), mv * 0.95 + var.numpy() * M / (M - 1) * 0.05, rtol=1e-5)
    y = torch.full((M * C + 64,), NAN, dtype=dtype, device="cuda")
    ops.bn_act_apply(dx, bn.affine, out=y[:M * C].view(1, 1, M, C))
    want = act_ref((xd - mean) / torch.sqrt(var + 1e-3) * torch.tensor(g).double() + torch.tensor(b).double(), act)
    assert_close(y[:M * C].reshape(M, C), want, dtype)
    assert bool(torch.isnan(y[M * C:]).all())


def test_bn_backward_apply_past_the_block_cap(cuda):
    """mpn_bn_bwd_apply through ops.bn_backward (reduce, finalize, apply): f32, C = 8, M = 8 388 608 + 4 097 rows = 16 785 410
    vectors. Cap: kApplyBlocks = 16 384 blocks x 1024 vectors = 16 777 216 per grid stride: 2 iterations, the second of 8 whole
    blocks and one that holds 2 vectors (three of its four pieces wholly out of range). ReLU6 and add_ch0.
    Reference: the batch-norm backward in float64 written out as chunked torch arithmetic on the device (sums, then
    dx = scale (g - sum g / M - xhat sum(g xhat) / M), + add_ch0 on channel 0); tolerance of test_bn_backward:
    assert_close(f32, scale = max |dx|), rtol / atol 2e-3 on dgamma / dbeta.
    x takes the nine values -4 .. 4, so that x * scale + shift takes nine values per channel; the test asserts that none lies
    within 5e-3 of ReLU6's thresholds 0 and 6 - with continuous x some of 67 M elements fall within f32 rounding of one, where
    the kernel's f32 mask and the float64 one legitimately differ."""
    ops = _ops()
    C, M, act = 8, 8388608 + 4097, 2
    assert _iterations(M * (C // 4), "bn_bwd_apply") == 2
    gen = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randint(-4, 5, (1, 1, M, C), generator=gen, device="cuda").float()
    dA0 = torch.randn((1, 1, M, C), generator=gen, device="cuda")
    a0 = torch.randn(M, generator=gen, device="cuda")
    gamma = torch.tensor([1.5, 2.0, 2.5, 3.0, 1.75, 2.25, 2.75, 3.25], dtype=torch.float64, device="cuda")
    beta = torch.tensor([0.3, -0.7, 1.1, 2.3, -1.9, 0.55, 3.1, -0.2], dtype=torch.float64, device="cuda")
    bn = ops.BNState(gamma.float(), beta.float(), torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), act)
    bn.dgamma, bn.dbeta = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    part, nparts = ops.bn_stats(x)
    assert nparts == 2048
    ops.bn_finalize(bn, part, nparts, M)
    x2, d2 = x.view(M, C), dA0.view(M, C)
    chunks = [(r, min(r + (1 << 20), M)) for r in range(0, M, 1 << 20)]
    zero = lambda: torch.zeros(C, dtype=torch.float64, device="cuda")
    s, q = zero(), zero()
    for r0, r1 in chunks:
        xd = x2[r0:r1].double()
        s += xd.sum(0)
        q += (xd * xd).sum(0)
    mean = s / M
    invstd = 1.0 / torch.sqrt(q / M - mean * mean + 1e-3)
    scale = gamma * invstd
    shift = beta - mean * scale
    levels = torch.arange(-4, 5, dtype=torch.float64, device="cuda")[:, None] * scale + shift
    assert float(torch.minimum(levels.abs(), (levels - 6).abs()).min()) > 5e-3
    assert bool((levels < 0).any()) and bool((levels > 6).any())
    np.testing.assert_allclose(bn.mean.cpu().numpy(), mean.cpu().numpy(), atol=2e-5)
    np.testing.assert_allclose(bn.invstd.cpu().numpy(), invstd.cpu().numpy(), rtol=2e-5)

    def masked(r0, r1):
        xd = x2[r0:r1].double()
        pre = xd * scale + shift
        g = torch.where((pre > 0) & (pre < 6), d2[r0:r1].double(), torch.zeros((), dtype=torch.float64, device="cuda"))
        return g, (xd - mean) * invstd

    s1, s2 = zero(), zero()
    for r0, r1 in chunks:
        g, xhat = masked(r0, r1)
        s1 += g.sum(0)
        s2 += (g * xhat).sum(0)
    dA = torch.full((M * C + 64,), NAN, device="cuda")
    dA[:M * C] = dA0.view(-1)
    part2 = torch.empty(nparts * 2 * C, device="cuda")
    ops.bn_backward(bn, dA[:M * C].view(1, 1, M, C), x, part2, add_ch0=a0)
    got = dA[:M * C].view(M, C)
    rtol, atol = tol(torch.float32)
    excess, biggest = 0.0, 0.0                                        # assert_close's statement, chunk by chunk
    for r0, r1 in chunks:
        g, xhat = masked(r0, r1)
        want = scale * (g - s1 / M - xhat * s2 / M)
        want[:, 0] += a0[r0:r1].double()
        err = torch.nan_to_num((got[r0:r1].double() - want).abs(), nan=float("inf"))
        excess = max(excess, float((err - rtol * want.abs()).max()))
        biggest = max(biggest, float(want.abs().max()))
    assert excess <= atol * biggest, f"|err| - {rtol:g} |want| reaches {excess:.3e}; allowed {atol:g} * max |want| = {atol * biggest:.3e}"
    assert bool(torch.isnan(dA[M * C:]).all()) and torch.equal(d2, dA0.view(M, C))
    np.testing.assert_allclose(bn.dgamma.cpu().numpy(), s2.cpu().numpy(), rtol=2e-3, atol=2e-3 * float(s2.abs().max()))
    np.testing.assert_allclose(bn.dbeta.cpu().numpy(), s1.cpu().numpy(), rtol=2e-3, atol=2e-3 * float(s1.abs().max()))


# ------------------------------------------------------------------------------------------------- 6. pyramid helpers
@pytest.mark.parametrize("h,w", [(260, 256), (259, 257)], ids=["260x256", "259x257"])
def test_sumpool2x2_past_the_block_cap(cuda, h, w):
    """mpn_sumpool2x2, plain and accumulate, f32, against avg_pool2d * 4 in float64. Cap: 8192 blocks x 256 = 2 097 152 vectors.
      dst 1 x 260 x 256 x 128 = 2 129 920 vectors: 2 iterations (the remainder is a whole 128 blocks, as the plan fixes it)
      dst 1 x 259 x 257 x 128 = 2 130 016 vectors: 2 iterations, the last of 128 blocks and 96 vectors; odd width"""
    ops = _ops()
    C, dtype = 128, torch.float32
    assert _iterations(h * w * (C // 4), "pool", partial=(h, w) != (260, 256)) == 2
    gen = _gen(h)
    src = torch.randn((1, 2 * h, 2 * w, C), generator=gen)
    dst0 = torch.randn((1, h, w, C), generator=gen)
    want = nhwc(F.avg_pool2d(nchw(src.double()), 2) * 4)
    dsrc = dev(src, dtype)
    assert_close(ops.sumpool2x2(dsrc), want, dtype)
    d = dev(dst0, dtype)
    ops.sumpool2x2(dsrc, d, accumulate=True)
    assert_close(d, want + dst0.double(), dtype)
    assert torch.equal(dsrc.cpu(), src)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_inplace_past_the_block_cap(cuda, dtype):
    """mpn_add_inplace at 2 097 152 + 1003 vectors (f32: 8 392 620 elements, bf16: 16 785 240). Cap: 8192 blocks x 256 =
    2 097 152 vectors: 2 iterations, the second of 3 blocks and 235 vectors."""
    ops = _ops()
    nvec = CAPS["pool"][0] + 1003
    assert _iterations(nvec, "pool") == 2
    n = nvec * (4 if dtype == torch.float32 else 8)
    gen = _gen(n % 9973)
    a, b = torch.randn(n, generator=gen).to(dtype), torch.randn(n, generator=gen).to(dtype)
    buf = torch.full((n + 64,), NAN, dtype=dtype, device="cuda")
    buf[:n] = a.cuda()
    db = b.cuda()
    ops.add_inplace(buf[:n], db)
    assert_close(buf[:n], a.double() + b.double(), dtype)
    assert bool(torch.isnan(buf[n:]).all()) and torch.equal(db.cpu(), b)


X1_CASES = [(torch.float32, 364, 364), (torch.float32, 363, 365), (torch.bfloat16, 520, 512), (torch.bfloat16, 521, 511)]


@pytest.mark.parametrize("dtype,h,w", X1_CASES, ids=[f"{IDS[DTYPES.index(dt)]}-{h}x{w}" for dt, h, w in X1_CASES])
def test_bilinear_x1_slice_kernels_past_the_block_cap(cuda, dtype, h, w):
    """mpn_bilinear_up_fwd / _bwd at upsample 1 (slice_affine_store_kernel, slice_copy_kernel): C = 128 into / out of channels
    16 .. 143 of a 160-channel tensor. Cap: 4096 blocks x 256 threads x 4 vectors (one grid width, 1 048 576, apart) =
    4 194 304 vectors per iteration.
      f32  1 x 364 x 364 = 4 239 872 vectors, bf16 1 x 520 x 512 = 4 259 840: 2 iterations; in the second only the first of a
          thread's four vectors is in range (three clamped loads), over a whole 178 / 256 blocks, as the plan fixes them
      f32  1 x 363 x 365 = 4 239 840, bf16 1 x 521 x 511 = 4 259 696: the same, and the last block is cut (224 / 112 vectors)
    Forward: act(x * scale + shift) in float64 inside the slice, zeros outside it. Backward: the gradient IS the slice."""
    ops = _ops()
    C, ctot, off = 128, 160, 16
    ve = 4 if dtype == torch.float32 else 8
    assert _iterations(h * w * (C // ve), "slice", partial=(h, w) in ((363, 365), (521, 511))) == 2
    gen = _gen(h)
    x = torch.randn((1, h, w, C), generator=gen).to(dtype)
    sc, sh = 0.5 + torch.rand(C, generator=gen), torch.randn(C, generator=gen) * 0.5
    want = torch.relu(x.double() * sc.double() + sh.double())
    out = torch.zeros((1, h, w, ctot), dtype=dtype, device="cuda")
    ops.bilinear_up_fwd(x.cuda(), 1, out, off, ops.Affine(dev(sc), dev(sh), 1))
    assert_close(out[..., off:off + C], want, dtype)
    assert float(out[..., :off].abs().max()) == 0 and float(out[..., off + C:].abs().max()) == 0
    dy = torch.randn((1, h, w, ctot), generator=torch.Generator(device="cuda").manual_seed(w), device="cuda").to(dtype)
    n = h * w * C
    buf = torch.full((n + 64,), NAN, dtype=dtype, device="cuda")
    got = ops.bilinear_up_bwd(dy, 1, off, C, out=buf[:n].view(1, h, w, C))
    assert torch.equal(got, dy[..., off:off + C])
    assert bool(torch.isnan(buf[n:]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("u", [1, 2, 4, 8])
@pytest.mark.parametrize("N,h,w,C", [(1, 4, 5, 24), (1, 3, 37, 64), (1, 2, 260, 8)], ids=["24ch", "wide-64ch", "rows-wider-than-a-block"])
def test_bilinear_forward_on_ragged_maps(cuda, dtype, u, N, h, w, C):
    """Forward shapes test_bilinear_into_concat_slice (2 x 6 x 10 x 128 only) lacks, on the ragged maps of test_bilinear_backward:
    C = 24 (6 / 3 vectors per pixel, 256 % that != 0: upsample 1 falls back from the slice kernel to the general one),
    a 37-wide map of 64 channels (a block row cut inside a pixel row) and a 260-wide one of 8 channels (several blocks per
    row), each into a slice at channel 16 of C + 32, against the oracle's legacy resize in float64."""
    ops = _ops()
    rs = np.random.RandomState(u + C)
    x = rnd(rs.randn(N, h, w, C), dtype)
    sc = torch.tensor(0.5 + rs.rand(C), dtype=torch.float32)
    sh = torch.tensor(rs.randn(C) * 0.5, dtype=torch.float32)
    a = torch.relu(x.double() * sc.double() + sh.double())
    want = nhwc(onet.resize_bilinear_legacy(nchw(a), h * u, w * u))
    out = torch.zeros((N, h * u, w * u, C + 32), dtype=dtype, device="cuda")
    ops.bilinear_up_fwd(dev(x, dtype), u, out, 16, ops.Affine(dev(sc), dev(sh), 1))
    assert_close(out[..., 16:16 + C], want, dtype)
    assert float(out[..., :16].abs().max()) == 0 and float(out[..., 16 + C:].abs().max()) == 0


# ------------------------------------------------------------------------- 6b. stride-2 depthwise data gradient, gather form
DW_S2_CASES = [(torch.float32, 593, 24), (torch.bfloat16, 513, 64)]


@pytest.mark.parametrize("dtype,H,C", DW_S2_CASES, ids=[f"{IDS[DTYPES.index(dt)]}-{H}x{H}x{C}" for dt, H, C in DW_S2_CASES])
def test_dwconv_stride2_gather_data_gradient_past_the_block_cap(cuda, dtype, H, C):
    """mpn_dwconv_bwd_data at stride 2 on an odd map (dwconv_dgrad_s2_kernel, the gather form that odd H / W or C / 4 not a
    power of two fall back to; csrc/dwconv.hip caps it at 8192 blocks x 256 = 2 097 152 vectors - the cap table's "pool" row has
    the same figures), against autograd through the oracle's depthwise conv in float64, tolerance of test_dwconv_backward.
      f32  1 x 593 x 593 x 24 = 2 109 894 vectors (6 per pixel): 2 iterations, the last of 49 blocks and 198 vectors
      bf16 1 x 513 x 513 x 64 = 2 105 352 vectors (8 per pixel): 2 iterations, the last of 32 blocks and 8 vectors"""
    ops = _ops()
    ve = 4 if dtype == torch.float32 else 8
    assert _iterations(H * H * (C // ve), "pool") == 2
    gen = _gen(H)
    w = torch.randn((3, 3, C, 1), generator=gen) / 3
    a = torch.zeros((1, C, H, H), dtype=torch.float64, requires_grad=True)
    out = onet.depthwise_conv2d_tf_same(a, w.double(), 2)
    dy = torch.randn(tuple(nhwc(out).shape), generator=gen).to(dtype)
    out.backward(nchw(dy.double()))
    n = H * H * C
    buf = torch.full((n + 64,), NAN, dtype=dtype, device="cuda")
    da = ops.dwconv_bwd_data(dy.cuda(), dev(w), (H, H), 2, out=buf[:n].view(1, H, H, C))
    assert_close(da, nhwc(a.grad), dtype, 9)
    assert bool(torch.isnan(buf[n:]).all())


# --------------------------------------------------------------------------------------------------------- 7. PRN crops
def test_crops_past_the_block_cap(cuda):
    """KeypointAssigner.crops (mpn_prn_crop): 130 boxes on a 3 x 64 x 48 map = 130 x 56 x 36 x 17 = 4 455 360 elements. Cap:
    16 384 blocks x 256 = 4 194 304 elements per grid stride: 2 iterations, the second of 1019 blocks and 192 elements (crops
    122 .. 129). With the edge boxes of test_minmax_and_crops_match_the_restatement, some of them among the last crops:
    whole image, zero height, padding index -1, boxes that stick out of the image. Bit-identical to the restatement."""
    from multiposenet_amd.prn_inference import KeypointAssigner
    b, h, w, n = 3, 64, 48, 130
    assert _iterations(n * 56 * 36 * 17, "crop") == 2
    first_late = CAPS["crop"][0] // (56 * 36 * 17)                        # the first crop the second iteration touches: 122
    rs = np.random.RandomState(130)
    hm = 1.0 / (1.0 + np.exp(-(rs.randn(b, h, w, 17) * 1.5 - 3.0)))
    hm[0, :, :, 3] = 0.1 * hm[0, :, :, 3]                                 # a channel under the 0.2 threshold: masked
    hm = hm.astype(np.float32)
    y1, x1 = rs.rand(n) * 0.6 - 0.05, rs.rand(n) * 0.6 - 0.05             # some boxes stick out of the image (extrapolation)
    boxes = np.stack([y1, x1, y1 + 0.1 + rs.rand(n) * 0.5, x1 + 0.05 + rs.rand(n) * 0.5], 1).astype(np.float32)
    ind = rs.randint(0, b, n).astype(np.int32)
    for base in (0, first_late + 1):
        boxes[base + 1] = [0.0, 0.0, 1.0, 1.0]                            # the whole image
        boxes[base + 2] = [0.25, 0.25, 0.25, 0.75]                        # zero height: every row samples the same line
        ind[base + 4] = -1                                                # padding slot -> zero crop
        ind[base + 5] = 0                                                 # (an image with the masked channel)
    assert ((boxes[first_late:, :2] < 0).any() or (boxes[first_late:, 2:] > 1).any())
    got = KeypointAssigner(None).crops(torch.tensor(hm).cuda(), torch.tensor(boxes).cuda(), torch.tensor(ind).cuda()).cpu().numpy()
    norm, _, _ = oprn.normalize_heatmaps(hm)
    want = oprn.crop_and_resize(norm, boxes, ind, (56, 36))
    assert got.shape == (n, 56, 36, 17)
    assert np.all(got[4] == 0) and np.all(got[first_late + 5] == 0)
    assert np.all(got[ind == 0][..., 3] == 0)
    np.testing.assert_array_equal(got, want)
