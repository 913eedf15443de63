"""CPU: the host half of the person-detector input pipeline - descriptor layout against the built library, invariants
and frequencies of the sampler (multiposenet_amd/detector/input_pipeline/detector_augment.py), and the independence of the
batches from the decode thread count."""
import math

import numpy as np
import pytest

import detector_augment_ref as ref
from multiposenet_amd.detector.input_pipeline import detector_augment as da
from multiposenet_amd.detector.input_pipeline import keypoint_augment as ka

F = np.float32


def _example(rng, people=None):
    h, w = int(rng.integers(200, 481)), int(rng.integers(240, 641))
    p = int(rng.integers(1, 6)) if people is None else people
    bh, bw = rng.uniform(0.1, 0.8, p) * h, rng.uniform(0.05, 0.5, p) * w
    y0, x0 = rng.uniform(0, 1, p) * (h - bh), rng.uniform(0, 1, p) * (w - bw)
    return h, w, np.stack([y0, x0, y0 + bh, x0 + bw], 1).astype(F)


def test_descriptor_layout_matches_the_library():
    from multiposenet_amd import _lib
    lib = _lib.lib()
    assert da.DESC_DTYPE.itemsize == lib.mpn_detector_augment_desc_bytes() == 112
    assert hasattr(lib, "mpn_detector_augment")
    assert lib.mpn_version() == 600                      # additive symbols: the ABI revision stays
    assert (da.COLOR, da.GRAYSCALE, da.PIXEL_SCALE, da.FLIP, da.EVAL, da.PAD) == \
           (ref.COLOR, ref.GRAYSCALE, ref.PIXEL_SCALE, ref.FLIP, ref.EVAL, ref.PAD) == (2, 4, 8, 16, 32, 64)
    assert da.DESC_DTYPE.fields["scale_y"][1] == 56 and da.DESC_DTYPE.fields["flags"][1] == 96


@pytest.mark.parametrize("size", [(640, 640), (256, 384)])
def test_sampler_invariants(size):
    H, W = size
    rng = np.random.default_rng(3)
    cropped = padded = emptied = 0
    for _ in range(400):
        h, w, boxes = _example(rng)
        d, out = da.sample_training(rng, h, w, boxes, size)
        da.check_descriptors(d, h * w * 3, H, W)
        cy, cx, ch, cw = (int(d[k]) for k in ("crop_y", "crop_x", "crop_h", "crop_w"))
        assert 0 <= cy and 0 <= cx and cy + ch <= h and cx + cw <= w and ch >= 1 and cw >= 1
        if (ch, cw) != (h, w):                             # a crop was found: inside the sampler's ranges
            cropped += 1
            lo, hi = da.CROP_ARGS["area_range"]
            assert F(lo) * F(w) * F(h) <= ch * cw <= F(hi) * F(w) * F(h)
            a0, a1 = da.CROP_ARGS["aspect_ratio_range"]
            assert (a0 * ch - 0.5) <= cw <= (a1 * ch + 0.5)           # w = rint(h * aspect)
        assert d["scale_y"] == F(ch) / F(H) and d["scale_x"] == F(cw) / F(W)
        assert (int(d["valid_h"]), int(d["valid_w"])) == (H, W)
        if d["flags"] & da.PAD:
            padded += 1
            py, px, ph, pw = (int(d[k]) for k in ("pad_y", "pad_x", "pad_h", "pad_w"))
            assert 0 <= py and py + ph <= H - 1 and 0 <= px and px + pw <= W - 1       # offsets are < H - sh
            assert 0.5 * H - 1 <= ph < 0.9 * H and 0.5 * W - 1 <= pw < 0.9 * W
            assert d["pad_scale_y"] == F(H) / F(ph) and d["pad_scale_x"] == F(W) / F(pw)
        if d["flags"] & da.PIXEL_SCALE:
            assert (d["minval"], d["maxval"]) == (F(0.8), F(1.2))
        assert not d["flags"] & (da.EVAL | ka.ROTATE)
        assert out.dtype == F and out.ndim == 2 and out.shape[1] == 4 and len(out) <= len(boxes)
        emptied += len(out) == 0
        assert np.all(out >= 0) and np.all(out <= 1)
        assert np.all(out[:, 0] <= out[:, 2]) and np.all(out[:, 1] <= out[:, 3])
    assert cropped > 200 and padded > 10
    print(f"{size}: cropped {cropped}, padded {padded}, images left without boxes {emptied}")


def test_pad_moves_boxes_by_the_drawn_scale_and_offsets():
    rng = np.random.default_rng(5)
    boxes = np.array([[0.1, 0.2, 0.6, 0.9], [0, 0, 1, 1]], F)
    for _ in range(50):
        state = rng.bit_generator.state
        out, scale, (oy, ox, sh, sw) = da.random_pad(rng, boxes, 256, 384)
        assert scale.dtype == F and 0.5 <= scale < 0.9 and (sh, sw) == (int(scale * F(256)), int(scale * F(384)))
        assert 0 <= oy < 256 - sh and 0 <= ox < 384 - sw
        t = np.array([oy / 256, ox / 384, oy / 256, ox / 384]).astype(F)
        np.testing.assert_array_equal(out, boxes * scale + t)           # the reference's scale, not sh / H
        rng.bit_generator.state = state
        np.testing.assert_array_equal(da.random_pad(rng, boxes, 256, 384)[0], out)


def test_jitter_is_bounded_by_a_hundredth_of_the_box_side():
    rng = np.random.default_rng(6)
    for _ in range(200):
        _, _, boxes = _example(rng)
        boxes = da.normalise(boxes, 480, 640)
        off = da.jitter_offsets(rng, boxes)
        bh, bw = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        side = np.stack([bh, bw, bh, bw], 1)
        assert off.dtype == F and off.shape == boxes.shape
        assert np.all(np.abs(off) <= F(0.01) * side * (1 + 1e-6))
    assert np.abs(off).max() > 0


def test_flip_is_an_involution():
    rng = np.random.default_rng(7)
    boxes = np.sort(rng.random((50, 2, 2), dtype=F), axis=1).reshape(50, 4)
    # xmin' = 1 - xmax is exact to a rounding of the difference; on a grid of 2^-12 the round trip is exact
    boxes = np.round(boxes * 4096) / F(4096)
    once = da.flip_left_right(boxes)
    np.testing.assert_array_equal(once[:, [0, 2]], boxes[:, [0, 2]])
    np.testing.assert_array_equal(once[:, 1], F(1) - boxes[:, 3])
    np.testing.assert_array_equal(da.flip_left_right(once), boxes)
    assert np.all(once[:, 1] <= once[:, 3])


def test_evaluation_sizes_and_boxes():
    rng = np.random.default_rng(8)
    for _ in range(300):
        h, w, boxes = _example(rng)
        d, out, (hp, wp) = da.sample_evaluation(h, w, boxes, 640)
        new_h, new_w, want_h, want_w = ka.evaluation_size(h, w, 640)
        assert (hp, wp) == (want_h, want_w) and hp % 128 == 0 and wp % 128 == 0 and min(new_h, new_w) == 640
        assert (int(d["valid_h"]), int(d["valid_w"])) == (new_h, new_w) and d["flags"] == da.EVAL
        assert (int(d["crop_y"]), int(d["crop_x"]), int(d["crop_h"]), int(d["crop_w"])) == (0, 0, h, w)
        assert d["scale_y"] == F(h) / F(new_h) and d["scale_x"] == F(w) / F(new_w)
        da.check_descriptors(d, h * w * 3, hp, wp)
        s = np.array([new_h / hp, new_w / wp, new_h / hp, new_w / wp]).astype(F)
        np.testing.assert_array_equal(out, (boxes / np.array([h, w, h, w], F)).astype(F) * s)
        assert np.all(out >= 0) and np.all(out <= 1)


def test_decision_frequencies_follow_the_reference():
    """Each decision is one Bernoulli draw per image: over n images the count lies within 4 standard deviations of
    n p (a fair sampler leaves that band about once in 16 000 tries per decision).
    The crop decision is read from its outcome: the one box, 20 pixels in the middle of a 300 x 300 image, lies inside
    every window of >= 75 % of the area and aspect 0.85..1.15 (such a window is at least 242 x 205), so every valid attempt
    wins and the crop differs from the whole image whenever it was drawn (an attempt that IS the whole image needs
    h = w = 300, about 1 in 10 000)."""
    n = 5000
    rng = np.random.default_rng(9)
    boxes = np.array([[140, 140, 160, 160]], F)
    counts = dict.fromkeys(("crop", "pad", "color", "gray", "scale", "flip"), 0)
    for _ in range(n):
        d, _ = da.sample_training(rng, 300, 300, boxes, (256, 256))
        f = int(d["flags"])
        counts["crop"] += (int(d["crop_h"]), int(d["crop_w"])) != (300, 300)
        counts["pad"] += bool(f & da.PAD)
        counts["color"] += bool(f & da.COLOR)
        counts["gray"] += bool(f & da.GRAYSCALE)
        counts["scale"] += bool(f & da.PIXEL_SCALE)
        counts["flip"] += bool(f & da.FLIP)
    want = {"crop": 0.9, "pad": 0.1, "color": 0.33, "gray": 0.033, "scale": 0.1, "flip": 0.5}   # person_detector_pipeline.py:109-116
    for k, p in want.items():
        bound = 4 * math.sqrt(n * p * (1 - p))
        print(f"{k}: {counts[k]} of {n}, expected {n * p:.0f} +- {bound:.0f}")
        assert abs(counts[k] - n * p) <= bound, k


class _Host:
    """The host half of DetectorPipeline without a device: records -> decode pool -> sample."""

    def __init__(self, examples, threads, seed):
        from multiposenet_amd.detector.input_pipeline.person_detector_pipeline import DetectorPipeline
        self.p = DetectorPipeline(examples, True, {"batch_size": 4, "image_size": (256, 384), "shuffle_buffer_size": 5},
                                  device="cpu", num_threads=threads, seed=seed)

    def batches(self, n):
        from concurrent.futures import ThreadPoolExecutor
        p = self.p
        shuffle_rng, rng = p.generators()
        records = p._records(shuffle_rng)
        out = []
        with ThreadPoolExecutor(max_workers=p.num_threads) as pool:
            for _ in range(n):
                ex = [f.result() for f in [pool.submit(p._decode, next(records)) for _ in range(p.batch_size)]]
                out.append(p.sample(rng, ex))
        return out


def test_batches_do_not_depend_on_the_thread_count():
    rng = np.random.default_rng(11)
    examples = []
    for _ in range(13):
        h, w, boxes = _example(rng)
        examples.append({"image": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "boxes": boxes})
    a, b, c = _Host(examples, 1, 4).batches(6), _Host(examples, 8, 4).batches(6), _Host(examples, 8, 5).batches(6)
    for (da_, ba, sa, na), (db, bb, sb, nb) in zip(a, b):
        assert da_.tobytes() == db.tobytes() and sa == sb == (384, 256) and na == nb
        assert len(ba) == len(bb) and all(np.array_equal(x, y) for x, y in zip(ba, bb))
    assert any(x[0].tobytes() != y[0].tobytes() for x, y in zip(a, c))      # another seed: other decisions
    assert _Host(examples, 1, 4).p.num_examples == 13
