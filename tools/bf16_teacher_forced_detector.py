"""The bf16 build's detector-head BACKWARD pass at the emulating oracle's forward state (teacher forcing): the port of
tools/bf16_teacher_forced.py to PersonDetectorNet (person_detector_model.py:8-81, retinanet.py:169-217, box_predictor.py:93-121).

Why not a plain comparison of step gradients: round 5's last scratch run did exactly that - the bf16 build's step against the f32 oracle
at random initialisation on one 128 x 256 batch - and read "all rel-L2 0.31, every *_for_level_7 / p7 / pre_p7_bn tensor 1.04-1.28":
the forward perturbation of bf16 storage shifts batch statistics taken over 2 x 1 x 2 = 4 pixels (level 7) and flips ReLU masks, and
the backward pass amplifies it - the same ill-conditioning tools/bf16_grad_bound.py measured on the keypoint net (the f64 oracle's OWN
gradient moves 0.93 under bf16 storage). Here the perturbation is taken out: the bf16 build runs its forward pass (sizing every buffer),
then every tensor its backward pass reads - the backbone features, the FPN sums, p3..p7, both stride-2 patch tensors, every tower
layer's raw output, the raw box / class outputs, and the batch statistics / affines of all 46 batch-norm layers of the head - is
OVERWRITTEN with the emulating oracle's (exactly representable) values; the build's matching, loss gradient and backward pass run from
there. What remains is the arithmetic of the backward kernels: bf16 gradient storage, f32 accumulation order, the fused reductions.

python tools/bf16_teacher_forced_detector.py [train steps] [batch] [height] [width]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from oracle import network as onet
from oracle import retinanet as R
from multiposenet_amd import ops
from multiposenet_amd.retinanet import LEVELS, NETS, PersonDetectorNet, generate_anchors

BN_EPS = 1e-3
HP = {"initial_learning_rate": 1e-3, "num_steps": 150000, "weight_decay": 0.0, "localization_loss_weight": 1.0,
      "classification_loss_weight": 2.0, "gamma": 2.0, "alpha": 0.25, "depth_multiplier": 1.0}


def groundtruth(rs, B, maxn=5):
    boxes = np.zeros((B, maxn, 4), np.float32)
    for b in range(B):
        for n in range(maxn):
            cy, cx = rs.rand(2)
            h, w = 0.1 + 0.5 * rs.rand(2)
            boxes[b, n] = [max(cy - h / 2, 0), max(cx - w / 2, 0), min(cy + h / 2, 1), min(cx + w / 2, 1)]
    return boxes, rs.randint(1, maxn + 1, B).astype(np.int32)


def trained_variables(steps, B, H, W, seed=5, pool=3):
    """the f32 build, `steps` steps over a small pool of batches: head variables that have left their initialisation (the backbone is
    frozen: its seeded initial values with randomised batch-norm statistics, as the detector tests use)"""
    bb = onet.randomize_bn(onet.init_params(seed), seed + 1)
    hp = R.init_head_params(seed + 2)
    net = PersonDetectorNet(backbone_values=bb, head_values=hp, dtype=torch.float32)
    rs = np.random.RandomState(seed)
    batches = []
    for _ in range(pool):
        img = torch.tensor(rs.rand(B, H, W, 3).astype(np.float32)).cuda()
        bx, nb = groundtruth(rs, B)
        batches.append((img, {"boxes": torch.tensor(bx).cuda(), "num_boxes": torch.tensor(nb).cuda()}))
    first = last = None
    for i in range(steps):
        l = net.train_step(batches[i % pool][0], batches[i % pool][1], HP)
        first = float(l[3]) if i == 0 else first
        last = float(l[3])
    head = {k: v for k, v in net.state_dict().items() if k in hp}
    return bb, head, first, last


def run(steps=40, B=2, H=256, W=384, seed=9, dtype=torch.bfloat16, verbose=True, boxes=None, num=None):
    """boxes ([B, N, 4] normalised (ymin, xmin, ymax, xmax)) and num ([B]): the held-out batch's boxes instead of random ones, to
    choose which levels get a matched anchor; the training pool keeps its random boxes."""
    bb, hp, first, last = trained_variables(steps, B, H, W)
    rs = np.random.RandomState(seed)
    img = rs.rand(B, H, W, 3).astype(np.float32)                       # a batch the variables have not seen
    assert (boxes is None) == (num is None)
    if boxes is None:
        boxes, num = groundtruth(rs, B)
    else:
        boxes, num = np.asarray(boxes, np.float32), np.asarray(num, np.int32)
        assert boxes.shape[0] == B and boxes.shape[2] == 4 and num.shape == (B,) and int(num.max()) <= boxes.shape[1]
    anchors, _ = generate_anchors(H, W)
    tg = np.zeros((B, anchors.shape[0], 4), np.float32); mt = np.zeros((B, anchors.shape[0]), np.int32)
    for b in range(B):
        tg[b], mt[b] = R.get_training_targets(anchors, boxes[b, :num[b]])
    # ---- the emulating oracle: forward with every stored tensor tapped, backward
    em = torch.bfloat16 if dtype == torch.bfloat16 else None
    frozen = lambda k: k.endswith("moving_mean") or k.endswith("moving_variance")
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=not frozen(k)) for k, v in hp.items()}
    bb64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in bb.items()}
    taps = {}
    ctx = onet.storage_emulation(em) if em is not None else None
    if ctx:
        ctx.__enter__()
    try:
        feats64 = onet.mobilenet_v1(torch.tensor(img, dtype=torch.float64), bb64, False, 1.0)
        enc, cls, _ = R.head_forward(feats64, p64, True, taps=taps)
        total, ls = R.total_loss_fn(enc, cls, torch.tensor(tg, dtype=torch.float64), torch.tensor(mt), HP, None)
        total.backward()
    finally:
        if ctx:
            ctx.__exit__(None, None, None)
    want = {k: p64[k].grad.numpy() for k in hp if not frozen(k)}
    # ---- the build: forward (buffers, targets), then the oracle's forward state in its place
    net = PersonDetectorNet(backbone_values=bb, head_values=hp, dtype=dtype)
    b = net.forward(torch.tensor(img).cuda(), True)
    net.create_targets({"boxes": torch.tensor(boxes).cuda(), "num_boxes": torch.tensor(num).cuda()})
    assert np.array_equal(b["matches"].cpu().numpy(), mt)

    def nhwc(t):
        return t.detach().permute(0, 2, 3, 1).contiguous()

    def put(dst, src_nhwc):
        assert tuple(dst.shape) == tuple(src_nhwc.shape), (dst.shape, src_nhwc.shape)
        dst.copy_(src_nhwc.to(dst.dtype).cuda())

    def put_bn(bn, name, raw_nchw):
        x = raw_nchw.detach()
        mean, var = x.mean(dim=(0, 2, 3)), x.var(dim=(0, 2, 3), unbiased=False)
        invstd = torch.rsqrt(var + BN_EPS)
        scale = p64[name + "/gamma"].detach() * invstd
        for dst, src in ((bn.mean, mean), (bn.invstd, invstd), (bn.scale, scale), (bn.shift, p64[name + "/beta"].detach() - mean * scale)):
            dst.copy_(src.float().cuda())

    # the frozen backbone's features: the oracle's ACTIVATED c3..c5 as the raw tensors, under an identity affine (ReLU6 of a value in
    # [0, 6] is the value)
    dev = net.device
    feats = {}
    for l in (3, 4, 5):
        c = nhwc(feats64[f"c{l}"]).to(dtype).cuda()
        feats[f"c{l}"] = (c, ops.Affine(torch.ones(c.shape[3], device=dev), torch.zeros(c.shape[3], device=dev), ops.ACT_RELU6))
    net._last = (b, feats, net._last[2])
    for l in (3, 4, 5):
        put(b["x"][l], nhwc(taps[f"x{l}"]))
    for l in LEVELS:
        put(b["p"][l], nhwc(taps[f"p{l}"])); put_bn(net.p_bn[l], f"p{l}_batch_norm", taps[f"p{l}"])
    put_bn(net.pre_p7_bn, "fpn/pre_p7_bn", taps["p6"])
    ops.patchify3x3s2(feats["c5"][0], b["patches6"], feats["c5"][1])          # (gathers of forced tensors: fpn.py:43-45)
    ops.patchify3x3s2(b["p"][6], b["patches7"], net.pre_p7_bn.affine)
    for net_name, out_name, _ in NETS:
        for l in LEVELS:
            for i in range(4):
                t = taps[f"{net_name}/conv{i}/l{l}"]
                put(b["t"][net_name][i][l], nhwc(t))                       # (layer 0: a channel slice of the merged tensor)
                put_bn(net.tower_bn[net_name][i][l], f"{net_name}/batch_norm_{i}_for_level_{l}", t)
            o = nhwc(taps[f"{net_name}/out/l{l}"])
            dst = b["out"][net_name][l]
            dst.zero_()
            put(dst[..., :o.shape[3]], o)                                  # (class_net: 6 of 8 stored channels)
    losses = net.compute_losses(HP)
    net.backward(0.0)
    got = {k: net.grads[k].cpu().numpy().astype(np.float64) for k in want}
    rel = lambda a, c: float(np.linalg.norm(a - c) / (np.linalg.norm(c) + 1e-300))
    cos = lambda a, c: float(a.ravel() @ c.ravel() / (np.linalg.norm(a) * np.linalg.norm(c) + 1e-300))
    rows = [(k, want[k].size, float(np.linalg.norm(want[k])), rel(got[k], want[k]), cos(got[k], want[k])) for k in sorted(want)]
    cat = lambda g: np.concatenate([g[k].ravel() for k in sorted(want)])
    out = {"rows": rows, "all_rel": rel(cat(got), cat(want)), "all_cos": cos(cat(got), cat(want)), "loss": float(losses[3]),
           "oracle_loss": float(total.detach()), "train_first": first, "train_last": last, "got": got, "want": want}
    if verbose:
        print(f"head variables after {steps} steps (total loss {first} -> {last}); batch of {B} @ {H}x{W}; teacher-forced backward of the "
              f"{'bf16' if dtype == torch.bfloat16 else 'f32'} build vs the {'emulating ' if em else ''}oracle: total loss {out['loss']:.5f} vs "
              f"{out['oracle_loss']:.5f}; ALL gradients rel-L2 {out['all_rel']:.4f}, cosine {out['all_cos']:.6f}")
        print("%-50s %9s %10s %8s %9s" % ("tensor", "size", "|g|", "rel-L2", "cosine"))
        for r in rows:
            print("%-50s %9d %10.3e %8.4f %9.6f" % r)
        worst = sorted(rows, key=lambda r: -r[3])[:8]
        print("worst eight:", [(r[0], round(r[3], 4)) for r in worst])
    return out


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:] if not x.startswith("--")][:4]
    run(*a)
    if "--f32" in sys.argv:
        run(*a, dtype=torch.float32)
