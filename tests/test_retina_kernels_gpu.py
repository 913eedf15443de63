"""GPU: the three detector-head kernels of csrc/retina.hip one entry point at a time - mpn_retina_loss (+ _finalize) per anchor,
mpn_retina_match on its ignore / forced-match branches, mpn_retina_nms on ties and at the LDS boundary - and the variants of
mpn_patchify3x3s2, each against oracle/retinanet.py (or a plain torch restatement) on a few hundred anchors: the entry points
take the level shapes and the anchor array as arguments, so every branch is reached in milliseconds. Every property a case
is built to reach is asserted on the ORACLE's side first: a case that stops reaching its branch fails instead of passing
vacuously."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import retinanet as R
from util import act_ref, dev, level_tensors, rnd

pytestmark = pytest.mark.gpu
PA, IA = ctypes.c_void_p * 5, ctypes.c_int * 5
SENTINEL = 7.0


def _L():
    from multiposenet_amd import _lib
    return _lib


def _ptrs(ts):
    return PA(*[_L().ptr(t) for t in ts])


def _hw(shapes):
    return IA(*[s[0] for s in shapes]), IA(*[s[1] for s in shapes])


def _flatten(levels, ch):
    """per-level [B,h,w,8 or 24] device tensors -> [B,A] (ch = 1: channels 0..5 of the 8) or [B,A,4] in anchor order, float64"""
    B = levels[0].shape[0]
    if ch == 1:
        return torch.cat([t.float().cpu()[..., :6].reshape(B, -1) for t in levels], dim=1).double().numpy()
    return torch.cat([t.float().cpu().reshape(B, -1, 4) for t in levels], dim=1).double().numpy()


# =============================================================================================== 1. mpn_retina_loss
LOSS_SHAPES = [(5, 7), (3, 4), (2, 2), (1, 3), (1, 1)]     # A = 330: two blocks per image, level boundaries at 210, 282, 306, 324
LOSS_A, LOSS_B = 330, 2
LW, CW, REG = 1.5, 2.0, 0.125
PLANTED = [0.0, 15.0, -15.0, 30.0, -30.0, 88.0, -88.0]     # all exactly representable in bf16


@functools.lru_cache(maxsize=None)
def _loss_inputs(planted, all_negative):
    """Seeded inputs of one loss case (float32 numpy, shared by the dtypes; nobody writes to them)."""
    assert sum(h * w * 6 for h, w in LOSS_SHAPES) == LOSS_A
    rs = np.random.RandomState(41 + 2 * planted + all_negative)
    enc = (rs.randn(LOSS_B, LOSS_A, 4) * 1.5).astype(np.float32)
    logit = (rs.randn(LOSS_B, LOSS_A) * 2.0).astype(np.float32)
    targets = rs.randn(LOSS_B, LOSS_A, 4).astype(np.float32)          # (non-zero on unmatched anchors too: the mask must hold)
    u = rs.rand(LOSS_B, LOSS_A)
    matches = np.where(u < 0.15, -2, np.where(u < 0.6, -1, rs.randint(0, 5, (LOSS_B, LOSS_A)))).astype(np.int32)
    if all_negative:
        matches = np.where(u < 0.3, -2, -1).astype(np.int32)
    for b in range(LOSS_B):                                           # every kind of anchor on both sides of every level boundary
        for i, edge in enumerate((210, 282, 306, 324)):
            matches[b, edge - 1], matches[b, edge] = ((-1, -2), (-2, -1))[(i + b) % 2] if all_negative else ((0, -1), (-2, 3))[(i + b) % 2]
    if planted:
        for kind in (0, -1, -2):
            for b in range(LOSS_B):
                idx = np.flatnonzero((matches[b] >= 0) if kind == 0 else (matches[b] == kind))
                if all_negative and kind == 0:
                    continue
                idx = rs.choice(idx, len(PLANTED), replace=False)
                logit[b, idx] = PLANTED
    bias_c = (rs.randn(6) * 0.3).astype(np.float32)
    bias_b = (rs.randn(24) * 0.2).astype(np.float32)
    return enc, logit, targets, matches, bias_c, bias_b


def _loss_reference(enc, logit, targets, matches, bias_c, bias_b, gamma, alpha, dt):
    """R.losses_fn in `dt` on (stored inputs + f32 bias) and autograd of LW * loc + CW * cls w.r.t. both. In float32 the sum
    input + bias is an f32 addition, as in the kernel; in float64 it is exact."""
    k_of = np.arange(enc.shape[1]) % 6          # anchor a of a location = channel k (the level offsets are multiples of 6)
    if dt == torch.float64:
        e = torch.tensor(enc, dtype=dt) + torch.tensor(bias_b.reshape(6, 4)[k_of], dtype=dt)
        x = torch.tensor(logit, dtype=dt) + torch.tensor(bias_c[k_of], dtype=dt)
    else:
        e, x = torch.tensor(enc + bias_b.reshape(6, 4)[k_of][None]), torch.tensor(logit + bias_c[k_of][None])
    e.requires_grad_(True); x.requires_grad_(True)
    ls = R.losses_fn(e, x, torch.tensor(targets, dtype=dt), torch.tensor(matches), gamma, alpha)
    (LW * ls["localization_loss"] + CW * ls["classification_loss"]).backward()
    return {"loc": float(ls["localization_loss"].detach()), "cls": float(ls["classification_loss"].detach()),
            "dcls": x.grad.double().numpy(), "dbox": e.grad.double().numpy()}


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _loss_call(lg, bx, dlg, dbx, dtype, d, gamma, alpha, with_grad):
    """One mpn_retina_loss + reduce + finalize over sentinel-filled outputs. Returns (part [rows,32], losses[4], dbias_cls, dbias_box)."""
    L = _L()
    from multiposenet_amd import ops
    rows = L.lib().mpn_retina_loss_num_parts(LOSS_B, LOSS_A)
    assert rows == LOSS_B * 2
    part = torch.full((rows, 32), SENTINEL, device="cuda")
    for t in dlg + dbx:
        t.fill_(SENTINEL)
    hs, ws = _hw(LOSS_SHAPES)
    L.call("mpn_retina_loss", _ptrs(lg), _ptrs(bx), _ptrs(dlg) if with_grad else None, _ptrs(dbx) if with_grad else None, hs, ws,
           L.dtype_code(dtype), L.ptr(d["bias_c"]), L.ptr(d["bias_b"]), L.ptr(d["matches"]), L.ptr(d["targets"]), L.ptr(d["nm"]),
           LOSS_B, gamma, alpha, LW, CW, L.ptr(part), L.stream_ptr())
    sums = torch.full((32,), SENTINEL, device="cuda")
    ops.reduce_partials(part, rows, 32, sums)
    losses = torch.tensor([SENTINEL, SENTINEL, REG, SENTINEL], device="cuda")
    dbc, dbb = torch.full((6,), SENTINEL, device="cuda"), torch.full((24,), SENTINEL, device="cuda")
    L.call("mpn_retina_loss_finalize", L.ptr(sums), L.ptr(d["nm"]), LW, CW, L.ptr(losses), L.ptr(dbc) if with_grad else None,
           L.ptr(dbb) if with_grad else None, L.stream_ptr())
    return part.cpu(), losses.cpu(), dbc.cpu(), dbb.cpu()


LOSS_CASES = {                       # name: (gamma, alpha, planted saturated logits, every anchor unmatched)
    "gamma2-planted": (2.0, 0.25, True, False),
    "gamma1.5-planted": (1.5, 0.25, True, False),
    "gamma0-alpha0.5": (0.0, 0.5, False, False),      # (autograd of pow(0, gamma < 1) is inf / NaN: no saturated logits here)
    "nothing-matched": (2.0, 0.25, True, True),
}


@pytest.mark.parametrize("case", list(LOSS_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_loss_per_anchor(cuda, dtype, case):
    """mpn_retina_loss + mpn_retina_loss_finalize against R.losses_fn in float64 (autograd of LW * loc + CW * cls), anchor by anchor
    over 5 levels x 2 images (A = 330; level boundaries 210 / 282 / 306 / 324, none block-aligned), random biases, matches from
    {-2, -1, 0..4}, logits planted at 0, +-15, +-30, +-88 on matched, unmatched and ignored anchors; bf16: the reference reads
    the bf16-rounded tensors, so there is no input-rounding term.

    Tolerances come from the reference's own float32 error, measured in the test on the same inputs: losses_fn in float32 on
    the CPU against float64, max |delta| / max |reference| per tensor. Measured on these inputs (four cases, both dtypes):
    dlogits 9.8e-8 (gamma 0) .. 1.23e-6 (gamma 2, planted logits), dboxes 1.1e-7 .. 1.3e-7, the two losses 3.4e-9 .. 7.7e-8. The
    kernel gets 8x that (device expf / log1pf / powf are not correctly rounded and the closed-form derivative is not autograd's
    chain) with a floor of 2^-22 of the tensor's largest value: dlogits within 7.8e-7 .. 9.8e-6 of the largest gradient, dboxes
    within 9.1e-7 .. 1.04e-6, the losses within 2.4e-7 (the floor) .. 6.2e-7. bf16 outputs add one rounding, 2^-8 of the element.

    Exact: padding channels 6, 7 of dlogits are 0 (sentinel gone); dcls == 0 on ignored anchors; dboxes == 0 on unmatched ones;
    the evaluation call (no gradient buffers) gives bit-identical loss sums and leaves part[:, 2:] zero. The bias gradients are
    the sums of the kernel's OWN stored gradients (float64 sum of the outputs, f32 accumulation error n * 2^-24 * sum|g| only)."""
    gamma, alpha, planted, all_negative = LOSS_CASES[case]
    enc, logit, targets, matches, bias_c, bias_b = _loss_inputs(planted, all_negative)
    enc_r, logit_r = rnd(enc, dtype).numpy(), rnd(logit, dtype).numpy()
    nm = int((matches >= 0).sum())
    assert (nm == 0) == all_negative and (matches == -2).any() and (matches == -1).any()
    want = _loss_reference(enc_r, logit_r, targets, matches, bias_c, bias_b, gamma, alpha, torch.float64)
    f32 = _loss_reference(enc_r, logit_r, targets, matches, bias_c, bias_b, gamma, alpha, torch.float32)
    norm = max(nm, 1)
    assert all(np.isfinite(v).all() for v in want.values()) and np.abs(want["dcls"]).max() > 0
    if all_negative:
        assert want["loc"] == 0.0 and not want["dbox"].any()
    else:
        assert np.abs(want["dbox"]).max() > 0
    measured = {k: _rel(np.asarray(f32[k]), np.asarray(want[k])) if np.any(want[k]) else 0.0 for k in want}
    allow = {k: max(8.0 * v, 2.0 ** -22) for k, v in measured.items()}
    print(f"\n[{case} {dtype}] float32 restatement vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in measured.items()))
    assert max(measured.values()) < 1e-5            # (the restatement itself is sound on these inputs)

    bx, lg = level_tensors(enc, logit, LOSS_SHAPES, dtype)
    dlg, dbx = [torch.empty_like(t) for t in lg], [torch.empty_like(t) for t in bx]
    d = {"bias_c": dev(bias_c), "bias_b": dev(bias_b), "matches": dev(matches), "targets": dev(targets),
         "nm": torch.tensor([nm], dtype=torch.int32, device="cuda")}
    part, losses, dbc, dbb = _loss_call(lg, bx, dlg, dbx, dtype, d, gamma, alpha, True)
    got_dcls, got_dbox = _flatten(dlg, 1), _flatten(dbx, 4)
    pad = torch.cat([t.float().cpu()[..., 6:].reshape(-1) for t in dlg]).numpy()
    sums = part.double().sum(0).numpy()
    losses = losses.double().numpy()
    print(f"[{case} {dtype}] kernel vs float64: dcls {_rel(got_dcls, want['dcls']):.2e} dbox "
          f"{_rel(got_dbox, want['dbox']) if want['dbox'].any() else 0.0:.2e} cls {abs(sums[0] / norm - want['cls']) / want['cls']:.2e} "
          f"loc {abs(sums[1] / norm - want['loc']) / max(want['loc'], 1e-300):.2e}")

    # ---- exact conditions
    assert np.isfinite(got_dcls).all() and np.isfinite(got_dbox).all() and np.isfinite(part.numpy()).all()
    assert not pad.any(), "padding channels 6, 7 of dlogits"
    assert not got_dcls[matches == -2].any(), "ignored anchors carry a classification gradient"
    assert not got_dbox[matches < 0].any(), "unmatched anchors carry a box gradient"
    # ---- the loss sums and the four losses
    np.testing.assert_allclose(sums[0] / norm, want["cls"], rtol=allow["cls"], atol=0)
    np.testing.assert_allclose(sums[1] / norm, want["loc"], rtol=allow["loc"], atol=0)
    np.testing.assert_allclose(losses[1], want["cls"], rtol=allow["cls"], atol=0)
    np.testing.assert_allclose(losses[0], want["loc"], rtol=allow["loc"], atol=0)
    assert losses[2] == REG
    total = LW * want["loc"] + CW * want["cls"] + REG
    np.testing.assert_allclose(losses[3], total, rtol=max(allow["cls"], allow["loc"]) + 2.0 ** -22, atol=0)
    if all_negative:
        assert losses[0] == 0.0 and sums[1] == 0.0          # and the normaliser was 1: losses[1] above is the plain sum
    # ---- gradients, element by element
    out_round = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    for name, got, ref in (("dcls", got_dcls, want["dcls"]), ("dbox", got_dbox, want["dbox"])):
        bound = allow[name] * np.abs(ref).max() + out_round * np.abs(ref)
        err = np.abs(got - ref)
        worst = np.unravel_index(int((err - bound).argmax()), err.shape)
        assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} elements off, worst at (image, anchor..) {worst}: " \
                                     f"{got[worst]!r} vs {ref[worst]!r} (bound {bound[worst]:.3e})"
    # ---- bias gradients = sums of the stored gradients
    k_of = np.arange(LOSS_A) % 6
    n_terms = LOSS_B * LOSS_A // 6
    for k in range(6):
        g = got_dcls[:, k_of == k]
        assert g.size == n_terms
        assert abs(float(dbc[k]) - g.sum()) <= n_terms * 2.0 ** -24 * np.abs(g).sum() + 1e-45, f"class bias gradient {k}"
        for j in range(4):
            g = got_dbox[:, k_of == k, j]
            assert abs(float(dbb[k * 4 + j]) - g.sum()) <= n_terms * 2.0 ** -24 * np.abs(g).sum() + 1e-45, f"box bias gradient {k},{j}"
    assert np.abs(dbc.numpy()).max() > 0

    # ---- evaluation call: the same loss sums bit for bit, no gradient columns, buffers untouched
    part_e, losses_e, dbc_e, dbb_e = _loss_call(lg, bx, dlg, dbx, dtype, d, gamma, alpha, False)
    assert torch.equal(part_e[:, :2], part[:, :2]) and not part_e[:, 2:].any()
    assert np.array_equal(losses_e.double().numpy(), losses)
    assert all(bool((t == SENTINEL).all()) for t in dlg + dbx) and bool((dbc_e == SENTINEL).all()) and bool((dbb_e == SENTINEL).all())


# =============================================================================================== 2. mpn_retina_match
def _match_case(anchors, boxes, num, pos_thr, neg_thr):
    """mpn_retina_match twice on one (uninitialised) workspace against R.get_training_targets image by image: matches identical,
    targets to float32 rounding of logf, the matched-anchor count. Returns the oracle's matches [B,A]."""
    anchors, boxes, num = np.ascontiguousarray(anchors, np.float32), np.ascontiguousarray(boxes, np.float32), np.asarray(num, np.int32)
    B, maxn = boxes.shape[:2]
    A = anchors.shape[0]
    want_m, want_t = np.zeros((B, A), np.int32), np.zeros((B, A, 4), np.float32)
    for b in range(B):
        want_t[b], want_m[b] = R.get_training_targets(anchors, boxes[b, :num[b]], pos_thr, neg_thr)
    _match_device(anchors, boxes, num, pos_thr, neg_thr, want_m, want_t)
    return want_m


def _match_device(anchors, boxes, num, pos_thr, neg_thr, want_m, want_t):
    L = _L()
    (B, maxn), A = boxes.shape[:2], anchors.shape[0]
    d_an, d_bx, d_nb = dev(anchors), dev(boxes), dev(num)
    matches = torch.full((B, A), 99, dtype=torch.int32, device="cuda")
    targets = torch.full((B, A, 4), SENTINEL, device="cuda")
    nm = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lib().mpn_retina_match_workspace_bytes(B, maxn), dtype=torch.uint8, device="cuda")
    for rep in range(2):                                   # twice: the keys and the counter reset themselves
        L.call("mpn_retina_match", L.ptr(d_an), L.ptr(d_bx), L.ptr(d_nb), B, A, maxn, pos_thr, neg_thr, L.ptr(matches), L.ptr(targets),
               L.ptr(nm), L.ptr(ws), ws.numel(), L.stream_ptr())
        got_m, got_t = matches.cpu().numpy(), targets.cpu().numpy()
        for b in range(B):
            diff = np.flatnonzero(got_m[b] != want_m[b])
            assert diff.size == 0, f"call {rep} image {b}: anchors {diff[:8]} got {got_m[b][diff[:8]]} want {want_m[b][diff[:8]]}"
        np.testing.assert_allclose(got_t, want_t, rtol=2e-6, atol=2e-6)
        assert int(nm.item()) == int((want_m >= 0).sum())


def _anchors_64x96():
    anchors, _ = R.generate_anchors(64, 96)
    assert anchors.shape == (774, 4)                       # four blocks, the last partly live
    return anchors


def test_match_distinct_thresholds_reach_the_ignore_branch(cuda):
    """Thresholds 0.5 / 0.4 (the reference project's own defaults): anchors whose best IoU lies in [0.4, 0.5) become -2. Three
    images: three boxes, none, and fewer boxes than max_boxes (the unused slot holds a box that would match everything)."""
    anchors = _anchors_64x96()
    gt = np.array([[.1, .1, .6, .5], [.3, .4, .9, .95], [0, 0, .3, .2]], np.float32)
    boxes = np.zeros((3, 3, 4), np.float32)
    boxes[0] = gt
    boxes[1] = gt                                          # num_boxes = 0: must not be read as boxes
    boxes[2, :2], boxes[2, 2] = gt[:2], [0, 0, 1, 1]
    want = _match_case(anchors, boxes, [3, 0, 2], 0.5, 0.4)
    for b in (0, 2):
        assert (want[b] == -2).any() and (want[b] == -1).any() and (want[b] >= 0).any()
    assert (want[0] == -2).sum() >= 20 and (want[1] == -1).all() and want[2].max() == 1
    # the same boxes at equal thresholds: no -2 anywhere (the other side of the branch)
    assert (_match_case(anchors, boxes, [3, 0, 2], 0.5, 0.5) >= -1).all()


def _crowd(seed, B, n):
    rs = np.random.RandomState(seed)
    boxes = np.zeros((B, n, 4), np.float32)
    for b in range(B):
        cy, cx = rs.rand(n), rs.rand(n)
        h, w = 0.05 + 0.5 * rs.rand(n), 0.05 + 0.5 * rs.rand(n)
        h[:40], w[:40] = 0.01, 0.01                        # tiny boxes: best IoU below the 0.05 rule
        boxes[b] = np.stack([np.maximum(cy - h / 2, 0), np.maximum(cx - w / 2, 0), np.minimum(cy + h / 2, 1), np.minimum(cx + w / 2, 1)], 1)
    return boxes


def test_match_more_boxes_than_threads_and_forced_collisions(cuda):
    """300 boxes per image (match_forced_kernel's loop strides past its 256 threads), 40 of them tiny: many boxes force the same
    anchor, and some anchors' smallest forcing box is below the 0.05 rule while a later one passes it - the anchor then takes
    the SMALLEST index all the same. Two images with different box counts."""
    anchors = _anchors_64x96()
    boxes, num = _crowd(1, 2, 300), [300, 270]
    for b in range(2):                                     # preconditions, from the oracle's own pieces
        sim = R.iou(boxes[b, :num[b]], anchors)
        forced, okay = sim.argmax(axis=1), sim.max(axis=1) >= np.float32(0.05)
        ids, counts = np.unique(forced, return_counts=True)
        mixed = [a for a in ids[counts > 1] if not okay[forced == a][0] and okay[forced == a].any()]
        late = [a for a in ids if np.flatnonzero(forced == a)[0] >= 256 and okay[forced == a].any()]
        assert num[b] > 256 and counts.max() >= 3 and (~okay).sum() >= 20 and len(mixed) >= 1 and (b == 1 or len(late) >= 1), \
            (counts.max(), int((~okay).sum()), len(mixed), len(late))
    want = _match_case(anchors, boxes, num, 0.5, 0.4)
    assert (want == -2).any() and want.max() >= 256


def test_match_box_without_any_overlap_forces_anchor_zero(cuda):
    """A groundtruth box with IoU 0 against every anchor (zero area here): argmax of its all-zero row is 0, so in the reference
    (training_target_creation.py:101-121) it forces ANCHOR 0 - never passing the 0.05 rule itself, but taking part in the
    smallest-index rule. With a second box whose best anchor is anchor 0, anchor 0 gets the zero-area box when that one comes
    first, the real box when it comes second; alone, the zero-area box forces nothing."""
    anchors = _anchors_64x96()
    zero, real = np.array([0.5, 0.5, 0.5, 0.7], np.float32), np.clip(anchors[0], 0, 1)
    sim = R.iou(np.stack([zero, real]), anchors)
    assert not sim[0].any() and sim[1].argmax() == 0 and sim[1, 0] >= 0.05
    boxes = np.zeros((3, 2, 4), np.float32)
    boxes[0], boxes[1], boxes[2, 0] = [zero, real], [real, zero], zero
    for pos_thr, neg_thr in ((0.5, 0.5), (0.5, 0.4)):
        want = _match_case(anchors, boxes, [2, 2, 1], pos_thr, neg_thr)
        assert want[0, 0] == 0 and want[1, 0] == 0 and (want[2] == -1).all()


def test_match_fewer_anchors_than_a_wave(cuda):
    """A hand-made 3 x 4 grid of 12 anchors (less than one wave: 52 idle lanes take part in the key reduction), max_boxes = 1:
    one image whose box has a positive, ignored and negative anchors, one whose box reaches no threshold and is force-matched."""
    anchors = np.array([[0.05 + 0.22 * r, 0.05 + 0.22 * c, 0.35 + 0.22 * r, 0.35 + 0.22 * c] for r in range(3) for c in range(4)], np.float32)
    boxes = np.array([[[0.05, 0.10, 0.35, 0.50]], [[0.60, 0.60, 0.75, 0.75]]], np.float32)
    want = _match_case(anchors, boxes, [1, 1], 0.5, 0.4)
    assert (want[0] == 0).any() and (want[0] == -2).any() and (want[0] == -1).any()
    sim1 = R.iou(boxes[1], anchors)[0]
    assert 0.05 <= sim1.max() < 0.4 and (want[1] == 0).sum() == 1 and want[1, sim1.argmax()] == 0


# =============================================================================================== 3. mpn_retina_nms
NMS_SHAPES = [(24, 30), (4, 5), (2, 2), (1, 2), (1, 1)]
NMS_A = 4482
NMS_DEAD = (5, 606, 2402, 4331, 4463, 4481)             # anchors wholly outside the unit square (k = 5, 0, 2, 5, 5, 5): clip to zero area


@functools.lru_cache(maxsize=None)
def _nms_anchors():
    assert sum(h * w * 6 for h, w in NMS_SHAPES) == NMS_A
    rs = np.random.RandomState(5)
    c, s = 0.1 + 0.8 * rs.rand(NMS_A, 2), 0.03 + 0.12 * rs.rand(NMS_A, 2)
    anchors = np.concatenate([c - s / 2, c + s / 2], axis=1).astype(np.float32)
    assert anchors.min() > 0 and anchors.max() < 1
    anchors[list(NMS_DEAD)] += 2.0
    return anchors


def _nms_biases(rs):
    """Biases on a 1/8 grid: bf16 logit + bias is then exact in f32, so two anchors score equal iff their sums are equal and
    unequal scores are never one rounding apart (which device expf and numpy's could order differently)."""
    return (rs.randint(-4, 5, 6) / 8.0).astype(np.float32), (rs.randint(-4, 5, 24) / 16.0).astype(np.float32)


def _oracle_selection(enc, logit, anchors, thr, iou_thr, md):
    """Anchor indices get_predictions selects for ONE image, in order (its own steps, keeping the indices)."""
    f = np.float32
    scores = (f(1.0) / (f(1.0) + np.exp(-logit.astype(f)))).astype(f)
    conf = np.flatnonzero(scores >= f(thr))
    boxes = np.clip(R.decode(enc[conf], anchors[conf]), f(0.0), f(1.0))
    return conf[R.non_max_suppression(boxes, scores[conf], md, iou_thr, thr)], scores, conf


def _nms_case(enc, logit, bias_c, bias_b, dtype, thr, iou_thr, md):
    """mpn_retina_nms over sentinel-filled outputs against R.get_predictions on (stored inputs + bias): the same detections in
    the same order, out_num exact, zero padding exact, the overflow word clear. Returns the oracle's (boxes, scores, num) and
    its inputs (enc + bias, logit + bias)."""
    anchors = _nms_anchors()
    B = enc.shape[0]
    k_of = np.arange(NMS_A) % 6
    enc_r, logit_r = rnd(enc, dtype).numpy(), rnd(logit, dtype).numpy()
    e_in, x_in = enc_r + bias_b.reshape(6, 4)[k_of][None], logit_r + bias_c[k_of][None]
    wb, wsc, wn = R.get_predictions(e_in, x_in, anchors, thr, iou_thr, md)
    ob, osc, on = _nms_device(enc, logit, bias_c, bias_b, dtype, thr, iou_thr, md)
    np.testing.assert_array_equal(on, wn)
    np.testing.assert_allclose(osc, wsc, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ob, wb, rtol=1e-4, atol=1e-5)
    for b in range(B):
        assert not ob[b, wn[b]:].any() and not osc[b, wn[b]:].any(), "padding behind the detections"
    return (wb, wsc, wn), (e_in, x_in)


def _nms_device(enc, logit, bias_c, bias_b, dtype, thr, iou_thr, md):
    L = _L()
    anchors, B = _nms_anchors(), enc.shape[0]
    bx, lg = level_tensors(enc, logit, NMS_SHAPES, dtype)
    d_bc, d_bb, d_an = dev(bias_c), dev(bias_b), dev(anchors)
    ob, osc = torch.full((B, md, 4), SENTINEL, device="cuda"), torch.full((B, md), SENTINEL, device="cuda")
    on = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lib().mpn_retina_nms_workspace_bytes(B, NMS_A), dtype=torch.uint8, device="cuda")
    hs, ws_ = _hw(NMS_SHAPES)
    L.call("mpn_retina_nms", _ptrs(lg), _ptrs(bx), hs, ws_, L.dtype_code(dtype), L.ptr(d_bc), L.ptr(d_bb), L.ptr(d_an), B, thr, iou_thr, md,
           L.ptr(ob), L.ptr(osc), L.ptr(on), L.ptr(ws), ws.numel(), L.stream_ptr())
    off = L.lib().mpn_retina_nms_overflow_offset(B, NMS_A)
    assert int(ws[off:off + 4].view(torch.int32).item()) == 0, "overflow word"
    return ob.cpu().numpy(), osc.cpu().numpy(), on.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _nms_random(seed, B, mean):
    rs = np.random.RandomState(seed)
    enc = (rs.randn(B, NMS_A, 4) * 0.5).astype(np.float32)
    logit = (rs.randn(B, NMS_A) * 1.5 + mean).astype(np.float32)
    bias_c, bias_b = _nms_biases(rs)
    return enc, logit, bias_c, bias_b


@pytest.mark.parametrize("md", [25, 1])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f32-quantised"])
def test_nms_ties_in_anchor_order(cuda, kind, md):
    """Three images, the middle one with nothing above the threshold. bf16 logits (and f32 logits rounded to integers: 60
    distinct scores over some 4000 candidates) make equal scores the normal case: among equal scores the smaller anchor index is selected first (the ~anchor half of the selection
    key). max_detections = 1 as well."""
    enc, logit, bias_c, bias_b = _nms_random(23, 3, -0.5)
    dtype = torch.bfloat16 if kind == "bf16" else torch.float32
    logit = logit.copy()
    logit[2] -= 3.0                                        # image 0: more than 4096 candidates (workspace walk); image 2: fewer (LDS)
    if kind == "f32-quantised":
        logit = np.round(logit).astype(np.float32)
    logit[1] = -9.0
    logit[0::2, 100] = logit[0::2, 3004] = 6.0             # (the same channel) the best score of images 0 and 2 is itself a tie
    (wb, wsc, wn), (e_in, x_in) = _nms_case(enc, logit, bias_c, bias_b, dtype, 0.05, 0.5, md)
    assert wn[0] == md and wn[1] == 0 and wn[2] == md
    for b in (0, 2):
        sel, scores, conf = _oracle_selection(e_in[b], x_in[b], _nms_anchors(), 0.05, 0.5, md)
        assert (len(conf) > 4096) == (b == 0)
        assert sel[0] == 100 and scores[3004] == scores[100] == scores[conf].max()
        if md > 1:
            tied = [i for i in range(1, len(sel)) if scores[sel[i]] == scores[sel[i - 1]]]
            assert len(tied) >= (1 if kind == "f32" else 2) and all(sel[i] > sel[i - 1] for i in tied), "selected detections sharing a score"
        if kind != "f32":
            assert len(np.unique(scores[conf])) < len(conf) // 2             # ties are the normal case


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_nms_at_the_lds_boundary(cuda, dtype):
    """Exactly 4096 candidates (the most the selection holds in LDS) in image 0, exactly 4097 (the first count it walks in the
    workspace) in image 1; every other logit is -9."""
    rs = np.random.RandomState(29)
    enc = (rs.randn(2, NMS_A, 4) * 0.5).astype(np.float32)
    bias_c, bias_b = _nms_biases(rs)
    logit = np.full((2, NMS_A), -9.0, np.float32)
    for b, n in enumerate((4096, 4097)):
        idx = rs.choice(NMS_A, n, replace=False)
        logit[b, idx] = np.maximum(rs.randn(n) * 1.5 + 1.0, -1.0)
    (wb, wsc, wn), (e_in, x_in) = _nms_case(enc, logit, bias_c, bias_b, dtype, 0.05, 0.5, 25)
    for b, n in enumerate((4096, 4097)):
        sel, scores, conf = _oracle_selection(e_in[b], x_in[b], _nms_anchors(), 0.05, 0.5, 25)
        assert len(conf) == n and (scores[conf] > np.float32(0.05)).all(), len(conf)
    assert (wn == 25).all()


def test_nms_zero_area_boxes_neither_suppress_nor_are_suppressed(cuda):
    """Three anchors outside the unit square (their boxes clip to zero area: IoU 0 with everything, nms_iou's early return) carry
    the highest, equal logits: all three are selected first, in anchor order, positive-area boxes follow, and one positive-area
    box - a copy of a better one - is suppressed."""
    enc, logit, bias_c, bias_b = _nms_random(31, 1, -4.0)
    enc, logit = enc.copy(), logit.copy()
    dead = [a for a in NMS_DEAD if a % 6 == 5][:3]                       # the same channel: equal logits give equal scores
    logit[0, dead] = 7.0
    anchors = _nms_anchors()
    twin_a, twin_b = 1200, 1206                                          # (same channel) two predictions of the same box
    shift = (anchors[twin_a, :2] + anchors[twin_a, 2:]) / 2 - (anchors[twin_b, :2] + anchors[twin_b, 2:]) / 2
    size_b = anchors[twin_b, 2:] - anchors[twin_b, :2]
    enc[0, twin_a] = 0.0
    enc[0, twin_b] = np.concatenate([10 * shift / size_b, 5 * np.log((anchors[twin_a, 2:] - anchors[twin_a, :2]) / size_b)])
    logit[0, twin_a], logit[0, twin_b] = 5.0, 4.75
    md = 8
    (wb, wsc, wn), (e_in, x_in) = _nms_case(enc, logit, bias_c, bias_b, torch.float32, 0.05, 0.5, md)
    sel, scores, conf = _oracle_selection(e_in[0], x_in[0], anchors, 0.05, 0.5, md)
    area = (wb[0, :, 2] - wb[0, :, 0]) * (wb[0, :, 3] - wb[0, :, 1])
    assert wn[0] == md and list(sel[:3]) == dead and not area[:3].any() and (area[3:] > 0).all()
    assert sel[3] == twin_a and twin_b not in sel and scores[twin_b] > scores[sel[-1]]    # suppressed, not merely out-ranked


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_nms_fewer_survivors_than_max_detections(cuda, dtype):
    """A dozen candidates per image, max_detections = 25: the rows behind the survivors are exactly 0 (no sentinel left)."""
    rs = np.random.RandomState(37)
    enc = (rs.randn(2, NMS_A, 4) * 0.5).astype(np.float32)
    bias_c, bias_b = _nms_biases(rs)
    logit = np.full((2, NMS_A), -9.0, np.float32)
    for b, n in enumerate((12, 1)):
        logit[b, rs.choice(NMS_A, n, replace=False)] = (rs.randn(n) + 1.0).astype(np.float32)
    (wb, wsc, wn), _ = _nms_case(enc, logit, bias_c, bias_b, dtype, 0.05, 0.5, 25)
    assert 3 <= wn[0] <= 12 and wn[1] == 1


# =============================================================================================== 4. mpn_patchify3x3s2
@pytest.mark.parametrize("mode", ["affine", "affine-relu", "affine-relu6", "plain"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_patchify_gathers_exactly(cuda, dtype, mode):
    """mpn_patchify3x3s2 alone against pad + unfold of the activated tensor, by equality: inputs on a 1/4 grid, scales from
    {1/2, 3/4, 1, 3/2}, shifts on a 1/8 grid make the affine exact in f32 however it is contracted, so the kernel only moves,
    clamps and (bf16) rounds values. Every activation, and the path without an affine (scale == NULL)."""
    from multiposenet_amd import ops
    L = _L()
    N, H, W, C = 2, 7, 11, 32
    rs = np.random.RandomState(43)
    x = rnd(rs.randint(-40, 41, (N, H, W, C)) / 4.0, dtype)            # (7 significant bits at most: exact in bf16)
    sc = torch.tensor(rs.choice([0.5, 0.75, 1.0, 1.5], C), dtype=torch.float32)
    sh = torch.tensor(rs.randint(-8, 9, C) / 8.0, dtype=torch.float32)
    act = {"affine": L.ACT_NONE, "affine-relu": L.ACT_RELU, "affine-relu6": L.ACT_RELU6, "plain": L.ACT_NONE}[mode]
    if mode == "plain":
        a, affine = x, None
    else:
        pre = x * sc + sh
        assert torch.equal(pre.double(), x.double() * sc.double() + sh.double())       # exact: no rounding to disagree about
        assert float(pre.max()) > 6.0 and float(pre.min()) < 0.0
        a, affine = rnd(act_ref(pre, act), dtype), ops.Affine(dev(sc), dev(sh), act)
    OH, OW = (H + 1) // 2, (W + 1) // 2
    cols = F.unfold(F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1)), kernel_size=3, stride=2)        # [N, C*9, OH*OW], (c, tap) order
    want = cols.view(N, C, 9, OH, OW).permute(0, 3, 4, 2, 1).reshape(N, OH, OW, 9 * C)
    out = torch.full((N, OH, OW, 9 * C), SENTINEL, device="cuda", dtype=dtype)
    ops.patchify3x3s2(dev(x, dtype), out, affine)
    got = out.float().cpu()
    assert (want == 0).any() and want.abs().max() > 6.0 - (mode == "affine-relu6")
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"
