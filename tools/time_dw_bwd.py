"""Depthwise backward, cold (rotating tensor sets), at the backbone's layer shapes (batch 32 @ 512 x 512):
    python tools/time_dw_bwd.py           stride 1: the fused walk (mpn_dwconv_bwd_fused) against the separate weight-gradient and
                                          data-gradient (+ reduction) launches
    python tools/time_dw_bwd.py --apply   all 13 layers: the batch-norm backward apply launch + the fused walk against the walk that
                                          applies on load (mpn_dwconv_bwd_fused_apply / _s2_apply), each timed three times"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiposenet_amd import ops
dt, B = torch.bfloat16, 32
st = torch.cuda.current_stream()


def apply_on_load():
    # (blocks, input rows, channels, stride) of Conv2d_i_depthwise; the stride-2 layers that feed an FPN lateral add its gradient
    layers = [("dw1", 256, 32, 1, False), ("dw2", 256, 64, 2, False), ("dw3", 128, 128, 1, False), ("dw4", 128, 128, 2, True),
              ("dw5", 64, 256, 1, False), ("dw6", 64, 256, 2, True), ("dw7-11", 32, 512, 1, False), ("dw12", 32, 512, 2, True),
              ("dw13", 16, 1024, 1, False)]
    count = {"dw7-11": 5}
    total = [0.0, 0.0]
    for name, H, C, s, add in layers:
        O = H // s
        byt_in, byt_out = B * H * H * C * 2, B * O * O * C * 2
        nset = max(2, min(10, int(1.6e9 // (2 * byt_in + 2 * byt_out + (byt_in if add else 0)))))
        mk = lambda n: [torch.randn(B, n, n, C, device="cuda").to(dt) for _ in range(nset)]
        xs, ys, gs = mk(H), mk(O), mk(O)
        adds = mk(H) if add else [None] * nset
        outs = [torch.empty(B, H, H, C, device="cuda", dtype=dt) for _ in range(nset)]
        w = torch.randn(3, 3, C, device="cuda") / 3
        one = lambda: torch.rand(C, device="cuda") + 0.5

        def mkbn():
            bn = ops.BNState(one(), one(), one(), one(), 2)
            bn.scale.copy_(one() * 0.8); bn.invstd.copy_(one()); bn.shift.copy_(torch.randn(C, device="cuda") * 0.5)
            bn.mean.copy_(torch.randn(C, device="cuda") * 0.3); bn.k1.copy_(torch.randn(C, device="cuda") * 0.05); bn.k2.copy_(torch.randn(C, device="cuda") * 0.05)
            return bn
        bn, ap = mkbn(), mkbn()
        rows = ops.dwconv_wgrad_num_parts(B, H, H, C, s, dt)
        wpart, sp = torch.empty(rows * 9 * C, device="cuda"), torch.empty(rows * 2 * C, device="cuda")

        def timed(fn):
            for i in range(nset):
                fn(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            it = 3 * nset
            e0.record(st)
            for i in range(it):
                fn(i)
            e1.record(st)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / it
        walk = lambda i, **kw: ops.dwconv_bwd_fused(xs[i % nset], gs[i % nset], w, bn, None, out=outs[i % nset], wpart=wpart, bn_part=sp,
                                                    reduce=False, stride=s, addend=adds[i % nset], **kw)

        def pair(i):
            ops.bn_bwd_apply(ap, gs[i % nset], ys[i % nset])
            walk(i)
        # alternating, three times each: the spread of the pair is the bar a folded walk has to clear
        # (one round untimed first: the first layer otherwise pays for the clocks coming up)
        tp, tf = [], []
        timed(pair); timed(lambda i: walk(i, apply_bn=ap, y_raw=ys[i % nset]))
        for _ in range(3):
            tp.append(timed(pair))
            tf.append(timed(lambda i: walk(i, apply_bn=ap, y_raw=ys[i % nset])))
        tw = timed(walk)
        spread = max(tp) - min(tp)
        gain = min(tp) - max(tf)
        n = count.get(name, 1)
        total[0] += n * sorted(tp)[1]; total[1] += n * sorted(tf)[1]
        print(f"{name:7s} {C:5d} ch @{H:3d} s{s}{' +add' if add else '     '}: apply + walk {min(tp):6.1f} .. {max(tp):6.1f} us (walk alone {tw:6.1f})   "
              f"folded {min(tf):6.1f} .. {max(tf):6.1f} us   worst-case gain {gain:6.1f} us, spread of the pair {spread:4.1f} us -> "
              f"{'FOLD' if gain > spread else 'keep the pass'}", flush=True)
        del xs, ys, gs, adds, outs
        torch.cuda.empty_cache()
    print(f"13 layers (medians): apply + walk {total[0]:7.1f} us, folded {total[1]:7.1f} us")


if "--apply" in sys.argv:
    apply_on_load()
    sys.exit(0)
for name, H, C in [("dw1", 256, 32), ("dw3", 128, 128), ("dw5", 64, 256), ("dw7-11", 32, 512), ("dw13", 16, 1024)]:
    byt = B * H * H * C * 2
    nset = max(2, min(10, int(1.6e9 // (3 * byt))))
    xs = [torch.randn(B, H, H, C, device="cuda").to(dt) for _ in range(nset)]
    dys = [torch.randn(B, H, H, C, device="cuda").to(dt) for _ in range(nset)]
    outs = [torch.empty(B, H, H, C, device="cuda", dtype=dt) for _ in range(nset)]
    w = torch.randn(3, 3, C, device="cuda") / 3
    one = lambda: torch.rand(C, device="cuda") + 0.5
    bn = ops.BNState(one(), one(), one(), one(), 2)
    bn.scale.copy_(one()); bn.invstd.copy_(one()); bn.shift.copy_(torch.randn(C, device="cuda") * 0.5); bn.mean.copy_(torch.randn(C, device="cuda") * 0.3)
    rows = ops.dwconv_wgrad_num_parts(B, H, H, C, 1, dt)
    wpart = torch.empty(rows * 9 * C, device="cuda"); sp = torch.empty(max(rows, ops.dwconv_bwd_data_bn_num_parts(B, H, H, C, 1, dt)) * 2 * C, device="cuda")
    dw = torch.zeros(3, 3, C, device="cuda")

    def timed(fn):
        for i in range(nset):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        it = 3 * nset
        e0.record(st)
        for i in range(it):
            fn(i)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / it
    fused = timed(lambda i: ops.dwconv_bwd_fused(xs[i % nset], dys[i % nset], w, bn, dw, out=outs[i % nset], wpart=wpart, bn_part=sp, reduce=False))
    wg = timed(lambda i: ops.dwconv_bwd_weight(xs[i % nset], dys[i % nset], 1, bn.affine, dw, wpart, reduce=False))
    dg = timed(lambda i: ops.dwconv_bwd_data(dys[i % nset], w, (H, H), 1, out=outs[i % nset], bn=bn, x_bn=xs[i % nset], part=sp))
    print(f"{name:7s} {C:5d} ch @{H:3d}: fused {fused:6.1f} us = {3 * byt / fused / 1e6:5.2f} TB/s of its 3 passes ({3 * byt / fused / 8e6:.3f} of 8 TB/s)   "
          f"separate: weight {wg:6.1f} + data {dg:6.1f} = {wg + dg:6.1f} us", flush=True)
    del xs, dys, outs
    torch.cuda.empty_cache()
