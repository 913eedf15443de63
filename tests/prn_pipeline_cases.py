"""Hand-made input tables for `mpn_prn_examples`, and the conditions that keep a bit-for-bit comparison on them from being
vacuous (checked on the CPU with the restatement alone, and again next to the GPU comparison)."""
import numpy as np

import prn_pipeline_ref as ref
from oracle.heatmap_creation import get_heatmaps, person_sigmas

F = np.float32
DESC = np.dtype([("image", "<i4"), ("person", "<i4"), ("flip", "<i4"), ("reserved", "<i4")])


def _person(rng, box, height, width, visible):
    ymin, xmin, ymax, xmax = box
    y = np.clip(rng.uniform(ymin, ymax, 17), 0, height - 1).astype(np.int32)
    x = np.clip(rng.uniform(xmin, xmax, 17), 0, width - 1).astype(np.int32)
    v = np.where(visible, rng.integers(1, 3, 17), 0).astype(np.int32)
    return np.stack([y, x, v], 1)


def handmade_tables():
    """Three images of ragged sizes: 203x157 (neither a multiple of 4; a box partly outside, two persons whose blobs overlap,
    one person without a visible keypoint), 480x640 with 70 small persons (sigma clipped to 1; crosses the 60-person culling
    chunk) and 641x702 with a box large enough for sigma clipped to 4. Flips alternate."""
    rng = np.random.default_rng(7)
    images = []
    # image 0
    h, w = 203, 157
    boxes = np.array([[-20.5, -10.25, 100, 90], [20, 30, 150.5, 120], [60, 40, 180, 150.75]], F)
    a = _person(rng, boxes[0], h, w, np.ones(17, bool))
    b = _person(rng, boxes[1], h, w, rng.random(17) < 0.7)
    b[3] = a[3] + np.array([2, -3, 0])      # part 3 of both: centres < 1 map pixel apart
    b[3, 2] = a[3, 2] = 2
    c = _person(rng, boxes[2], h, w, np.zeros(17, bool))
    images.append((np.stack([a, b, c]), boxes, h, w))
    # image 1
    h, w = 480, 640
    bx, kp = [], []
    for _ in range(70):
        bh, bw = rng.uniform(40, 120), rng.uniform(30, 110)
        y0, x0 = rng.uniform(0, h - bh), rng.uniform(0, w - bw)
        bx.append((y0, x0, y0 + bh, x0 + bw))
        kp.append(_person(rng, bx[-1], h, w, rng.random(17) < 0.6))
    images.append((np.stack(kp), np.array(bx, F), h, w))
    # image 2
    h, w = 641, 702
    boxes = np.array([[10, 20, 630, 690], [300, 100, 500.5, 260.25]], F)
    images.append((np.stack([_person(rng, boxes[0], h, w, rng.random(17) < 0.8),
                             _person(rng, boxes[1], h, w, rng.random(17) < 0.5)]), boxes, h, w))
    first = np.cumsum([0] + [len(i[1]) for i in images])
    ex = [(0, 0), (0, 1), (0, 2), (0, 0), (2, 0), (2, 1), (2, 0)]
    ex += [(1, int(k)) for k in [0, 5, 17, 33, 59, 60, 61, 65, 69, 42, 69]]
    descs = np.zeros(len(ex), DESC)
    for n, (r, k) in enumerate(ex):
        descs[n] = (r, first[r] + k, n % 2, 0)
    descs[3]["flip"] = 1                      # person 0 of image 0 both ways (example 0 unflipped)
    return {"keypoints": np.concatenate([i[0] for i in images]).astype(np.int32),
            "boxes": np.concatenate([i[1] for i in images]).astype(F),
            "first_person": first.astype(np.int32),
            "width": np.array([i[3] for i in images], np.int32), "height": np.array([i[2] for i in images], np.int32),
            "examples": descs}


def random_tables(seed, images=9, n=32):
    """Toy-shard-like annotations: random sizes, 1-4 persons per image, random boxes, visibilities and flips."""
    rng = np.random.default_rng(seed)
    kps, bxs, hs, ws = [], [], [], []
    for _ in range(images):
        h, w = int(rng.integers(200, 481)), int(rng.integers(240, 641))
        p = int(rng.integers(1, 5))
        bx = []
        for _ in range(p):
            bh, bw = rng.uniform(0.2, 0.8) * h, rng.uniform(0.1, 0.5) * w
            y0, x0 = rng.uniform(0, h - bh), rng.uniform(0, w - bw)
            bx.append((y0, x0, y0 + bh, x0 + bw))
        kps.append(np.stack([_person(rng, b, h, w, rng.random(17) < 0.66) for b in bx]))
        bxs.append(np.array(bx, F))
        hs.append(h)
        ws.append(w)
    first = np.cumsum([0] + [len(b) for b in bxs])
    descs = np.zeros(n, DESC)
    for i in range(n):
        r = int(rng.integers(images))
        descs[i] = (r, first[r] + int(rng.integers(len(bxs[r]))), int(rng.random() < 0.5), 0)
    return {"keypoints": np.concatenate(kps).astype(np.int32), "boxes": np.concatenate(bxs).astype(F),
            "first_person": first.astype(np.int32), "width": np.array(ws, np.int32), "height": np.array(hs, np.int32),
            "examples": descs}


def visible_count(tables):
    kp = tables["keypoints"]
    return int(sum((kp[int(e["person"]), :, 2] > 0).sum() for e in tables["examples"]))


def check_batch(tables, crops, labels):
    """Every batch: some crop element is nonzero and the labels hold one 1.0 per visible keypoint."""
    assert np.count_nonzero(crops) > 0
    assert float(labels.sum()) == visible_count(tables)
    assert set(np.unique(labels)) <= {0.0, 1.0}


def check_handmade(tables, crops, labels):
    """The conditions on the hand-made inputs, from the restatement's outputs `crops`, `labels`."""
    kp, bx, fp = tables["keypoints"], tables["boxes"], tables["first_person"]
    hs, ws, ex = tables["height"], tables["width"], tables["examples"]
    check_batch(tables, crops, labels)
    assert len(set(zip(hs.tolist(), ws.tolist()))) > 1 and any(h % 4 and w % 4 for h, w in zip(hs, ws))     # ragged
    counts = np.diff(fp)
    big = int(np.argmax(counts))
    assert counts[big] > 60                                                     # crosses the culling chunk
    assert any(e["image"] == big and e["person"] - fp[big] >= 60 for e in ex)
    # a box partly outside its image: the rows above the image are the extrapolation value, the rest is not
    n0 = next(n for n, e in enumerate(ex) if bx[e["person"], 0] < 0 and not e["flip"])
    assert not crops[n0, 0].any() and crops[n0].any()
    # a person without a visible keypoint: all labels zero
    assert any((kp[e["person"], :, 2] <= 0).all() and not labels[n].any() for n, e in enumerate(ex))
    # two persons whose blobs overlap in one channel
    a, b = int(fp[0]), int(fp[0]) + 1
    one = get_heatmaps(kp[a:a + 1], bx[a:a + 1], int(ws[0]), int(hs[0]), ref.DOWNSAMPLE)
    two = get_heatmaps(kp[b:b + 1], bx[b:b + 1], int(ws[0]), int(hs[0]), ref.DOWNSAMPLE)
    assert ((one > 0) & (two > 0)).any()
    assert any(e["flip"] for e in ex) and not all(e["flip"] for e in ex)
    sig = person_sigmas(bx[sorted({int(e["person"]) for e in ex})])
    assert (sig == F(1)).any() and (sig == F(4)).any()                          # both clip ends
