"""The cases of the COCO mask tests: groups of (h, w, annotations) items with what tests/coco_mask_ref.py makes of them
(computed once per session and shared), and a toy COCO data set written to a directory."""
import functools
import json
import os

import numpy as np

import coco_mask_ref as ref

# (h, w): 1 x 1; sides that are no multiple of 4; h no multiple of 32 (columns straddle bitmap words); mh * mw * 2 bits no
# multiple of 8 (5 x 7 -> 2 x 2 x 2 = 8 is, 37 x 53 -> 10 x 14 x 2 = 280 is, 33 x 257 -> 9 x 65 x 2 = 1170 is not,
# 1 x 1 -> 2 is not)
SIZES = [(1, 1), (4, 4), (5, 7), (37, 53), (64, 48), (130, 70), (33, 257)]


def shapes(h, w):
    """name -> flat polygon, scaled to an h x w image."""
    return {
        'triangle': [0.1 * w, 0.1 * h, 0.9 * w, 0.25 * h, 0.4 * w, 0.9 * h],
        'concave': [0.1 * w, 0.1 * h, 0.9 * w, 0.1 * h, 0.9 * w, 0.9 * h, 0.5 * w, 0.35 * h, 0.1 * w, 0.9 * h],
        'self_intersecting': [0.1 * w, 0.1 * h, 0.9 * w, 0.9 * h, 0.9 * w, 0.1 * h, 0.1 * w, 0.9 * h],
        'sliver': [0.2 * w, 0.3 * h, 0.8 * w, 0.3 * h + 0.3, 0.5 * w, 0.3 * h + 0.1],
        'two_points': [0.2 * w, 0.2 * h, 0.7 * w, 0.8 * h],
        'axis_aligned': [float(min(1, w - 1)), float(min(1, h - 1)), float(w), float(min(1, h - 1)), float(w), float(max(h - 1, 1)),
                         float(min(1, w - 1)), float(max(h - 1, 1))],
        'fractions': [0.5, 0.5, w - 0.5, 1.1, w - 1.1, h - 0.5, int(w / 2) + 0.1, int(h / 2) + 0.5, 1.5, h - 0.1],
        'outside': [-0.5 * w, -0.3 * h, 1.6 * w, 0.4 * h, 0.5 * w, 1.7 * h, -0.2 * w, 0.8 * h],
        'touches_bottom': [0.2 * w, 0.5 * h, 0.8 * w, 0.4 * h, 0.9 * w, float(h), 0.5 * w, h + 0.4 * h, 0.1 * w, float(h)],
    }


def _ann(segmentation, dropped=False):
    return {'segmentation': segmentation, 'dropped': dropped}


def _blob(h, w, rng):
    """A crowd region: a uint8 [h, w] mask of a few rectangles."""
    m = np.zeros((h, w), np.uint8)
    for _ in range(3):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[y0:y0 + int(rng.integers(1, h // 2 + 2)), x0:x0 + int(rng.integers(1, w // 2 + 2))] = 1
    return m


def _random_polygon(h, w, rng, lo=3, hi=40, spread=0.3):
    k = int(rng.integers(lo, hi + 1))
    x = rng.uniform(-spread * w, (1 + spread) * w, k)
    y = rng.uniform(-spread * h, (1 + spread) * h, k)
    snap = rng.integers(0, 3, k)                     # a third of the vertices on .5, a third on .1 fractions
    x = np.where(snap == 1, np.floor(x) + 0.5, np.where(snap == 2, np.floor(x) + 0.1, x))
    y = np.where(snap == 1, np.floor(y) + 0.5, np.where(snap == 2, np.floor(y) + 0.1, y))
    return np.stack([x, y], 1).reshape(-1).tolist()


def _person(h, w, rng):
    """A person-sized star-shaped polygon somewhere in the image."""
    k = int(rng.integers(8, 21))
    cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(20, 90)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * rng.uniform(0.4, 1.0, k)
    return np.stack([cx + rad * np.cos(ang), cy + 1.5 * rad * np.sin(ang)], 1).round(2).reshape(-1).tolist()


def _items(group):
    rng = np.random.default_rng(0)
    items = []
    if group == 'shapes':                            # every shape at every size: kept, with the next shape dropped
        for h, w in SIZES:
            polys = list(shapes(h, w).values())
            for i, p in enumerate(polys):
                items.append((h, w, [_ann([p]), _ann([polys[(i + 1) % len(polys)]], True)]))
    elif group == 'combinations':
        for h, w in [(64, 48), (130, 70)]:
            a = [0.1 * w, 0.1 * h, 0.6 * w, 0.1 * h, 0.6 * w, 0.6 * h, 0.1 * w, 0.6 * h]
            b = [0.4 * w, 0.4 * h, 0.9 * w, 0.4 * h, 0.9 * w, 0.9 * h, 0.4 * w, 0.9 * h]
            blob = _blob(h, w, rng)
            runs = ref.rle_encode(blob)
            items += [
                (h, w, [_ann([a, b])]),                                             # a union, not an XOR; no dropped person
                (h, w, [_ann([a]), _ann([b], True)]),                               # a dropped person over a kept one
                (h, w, [_ann([a, b], True), _ann([b, shapes(h, w)['triangle']])]),
                (h, w, [_ann([a]), _ann({'counts': runs, 'size': [h, w]}, True)]),  # a crowd region: run lengths ...
                (h, w, [_ann([a]), _ann({'counts': ref.rle_to_string(runs), 'size': [h, w]}, True)]),   # ... and the string
                (h, w, [_ann({'counts': [0, 5, h * w - 5], 'size': [h, w]}), _ann({'counts': [h * w - 1, 1], 'size': [h, w]}, True)]),
                (h, w, []),                                                         # no person at all
                (h, w, [_ann([]), _ann([], True)]),                                 # persons without a polygon
            ]
    elif group == 'coco':                            # one COCO-sized image (w 640, h 427) with 20 persons
        h, w = 427, 640
        anns = [_ann([_person(h, w, rng)] + ([_person(h, w, rng)] if i % 5 == 0 else []), dropped=i % 3 == 0) for i in range(19)]
        anns.append(_ann({'counts': ref.rle_to_string(ref.rle_encode(_blob(h, w, rng))), 'size': [h, w]}, True))
        items.append((h, w, anns))
    elif group == 'random':
        for h, w in [(37, 53), (64, 48), (130, 70), (33, 257), (5, 7), (96, 96)] * 2:
            items.append((h, w, [_ann([_random_polygon(h, w, rng)]), _ann([_random_polygon(h, w, rng), _random_polygon(h, w, rng, hi=8)], True)]))
    elif group == 'ragged':                          # nine images of nine sizes
        for i, (h, w) in enumerate(SIZES + [(96, 100), (17, 300)]):
            items.append((h, w, [_ann([_random_polygon(h, w, rng, hi=12)], dropped=bool(i % 2)), _ann([shapes(h, w)['concave']])]))
    elif group == 'paths':                           # what the issue's sizes do not reach inside the kernel
        ring = np.linspace(0, 2 * np.pi, 300, endpoint=False)

        def star(h, w):                              # 300 vertices: more than one group of 256 edges
            rad = (0.25 + 0.2 * (np.arange(300) % 2)) * min(h, w)
            return np.stack([0.5 * w + rad * np.cos(ring), 0.5 * h + rad * np.sin(ring)], 1).round(3).reshape(-1).tolist()
        # h = 1000: 32 words per column, 248 columns per 32 KB chunk - polygons over two chunks, one with crossings at y == h
        items.append((1000, 300, [_ann([[5.0, 100.0, 295.0, 50.0, 290.0, 1000.0, 150.0, 1200.0, 10.0, 1000.0]]),
                                  _ann([star(1000, 300), [0.0, 990.0, 300.0, 990.0, 300.0, 1000.0, 0.0, 1000.0]], True)]))
        noise = (rng.random((130, 70)) < 0.5).astype(np.uint8)         # a run-length code of thousands of runs
        items.append((130, 70, [_ann([star(130, 70)]), _ann({'counts': ref.rle_encode(noise), 'size': [130, 70]}, True)]))
        items.append((1024, 1024, [_ann([[-500.0, 20.0, 1500.0, 400.0, 512.5, 1900.0]]),     # the largest image there is
                                   _ann([[1000.0, 1000.0, 1024.0, 1000.0, 1024.0, 1024.0, 1000.0, 1024.0]], True)]))
    else:
        raise KeyError(group)
    return items


@functools.lru_cache(maxsize=None)
def group(name):
    """-> (items, packed list, full list) of the group, from the transcription. Shared: do not write to the arrays."""
    items = _items(name)
    packed, full = ref.rasterize(items, return_full=True)
    for a in packed + full:
        a.setflags(write=False)
    return items, packed, full


# ---------------------------------------------------------------- a toy data set
def _keypoints(x0, y0, labelled=17):
    out = []
    for k in range(17):
        out += [x0 + 2 * (k % 5), y0 + 3 * (k // 5), 2] if k < labelled else [0, 0, 0]
    return out


def _person_ann(image_id, bbox, labelled=17, kp_at=None):
    x, y, bw, bh = bbox
    kx, ky = kp_at if kp_at else (int(x) + 1, int(y) + 1)
    return {'image_id': image_id, 'category_id': 1, 'iscrowd': 0, 'bbox': list(bbox), 'area': float(bw * bh) / 2,
            'num_keypoints': labelled, 'keypoints': _keypoints(kx, ky, labelled),
            'segmentation': [[x, y, x + bw, y, x + bw, y + bh, x, y + bh]]}


def toy_dataset(root):
    """Writes images and person_keypoints_toy.json under `root`; returns (json path, images dir). Six images with persons:
    a.jpg (a good person, a person with one labelled keypoint, a person with a 4-pixel box, a box hanging over the edge),
    b.jpg (only dropped persons), c.png (not a JPEG), d.jpg (grayscale), e.jpg and f.jpg (one good person each)."""
    from PIL import Image
    images_dir = os.path.join(str(root), "images")
    os.makedirs(images_dir, exist_ok=True)
    rng = np.random.default_rng(3)
    sizes = {'a.jpg': (48, 64), 'b.jpg': (40, 40), 'c.png': (32, 32), 'd.jpg': (37, 53), 'e.jpg': (64, 48), 'f.jpg': (33, 70)}
    for name, (h, w) in sizes.items():
        if name == 'd.jpg':
            Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8), 'L').save(os.path.join(images_dir, name), format='jpeg')
        else:
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 'RGB').save(
                os.path.join(images_dir, name), format='png' if name.endswith('.png') else 'jpeg')
    ids = {name: i + 1 for i, name in enumerate(sizes)}
    anns = [_person_ann(1, (5.5, 6.25, 30.0, 35.0)),
            _person_ann(1, (20.0, 10.0, 20.0, 20.0), labelled=1),
            _person_ann(1, (40.0, 30.0, 4.0, 12.0)),
            _person_ann(1, (50.0, 38.0, 30.0, 30.0), kp_at=(60, 44)),           # clipped to (38, 50, 48, 64); keypoints past the edge
            _person_ann(2, (5.0, 5.0, 20.0, 20.0), labelled=0),
            _person_ann(2, (10.0, 10.0, 3.0, 3.0)),
            _person_ann(3, (5.0, 5.0, 20.0, 20.0)),
            _person_ann(4, (10.0, 8.0, 30.0, 20.0)),
            _person_ann(5, (4.0, 4.0, 40.0, 50.0)),
            _person_ann(6, (30.0, 3.0, 25.0, 25.0)),
            {'image_id': 6, 'category_id': 1, 'iscrowd': 1, 'bbox': [0.0, 0.0, 10.0, 10.0], 'area': 50.0, 'num_keypoints': 0,
             'keypoints': [0] * 51, 'segmentation': {'counts': [0, 396, 33 * 70 - 396], 'size': [33, 70]}}]
    for i, a in enumerate(anns):
        a['id'] = 100 + i
    coco = {'images': [{'id': ids[n], 'file_name': n, 'height': h, 'width': w} for n, (h, w) in sizes.items()]
            + [{'id': 99, 'file_name': 'nobody.jpg', 'height': 10, 'width': 10}],
            'annotations': anns, 'categories': [{'id': 1, 'name': 'person'}]}
    path = os.path.join(str(root), "person_keypoints_toy.json")
    with open(path, "w") as f:
        json.dump(coco, f)
    return path, images_dir
