"""What the masks of COCO keypoint records cost: `CocoMaskRasterizer` (mpn_coco_masks, csrc/coco_masks.hip) on a batch of
synthetic COCO-sized images, `write_shards` end to end on a directory of synthetic JPEGs, and the same masks from the
plain-loop numpy transcription (tests/coco_mask_ref.py) on one thread - what the reference's script pays per image.

    timeout -k 10 400 python tools/bench_coco_masks.py [--batch 64] [--persons 4] [--images 256] [--rounds 5]
                                                       [--out profiles/coco_masks.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

  device_ms_per_batch     HIP events around back-to-back mpn_coco_masks calls on uploaded tables (three launches each)
  rasterize_ms_per_batch  wall clock of `rasterize`: tables built on the host, one copy up, the call, packed bits back
  write_shards            wall images/s over `--images` JPEGs in a temporary directory (read on the thread pool, rules,
                          rasterise, encode, frame, write)
  host                    tests/coco_mask_ref.py on `--host-images` of the same images, one thread; the tool stops if its packed
                          masks differ from the device's
A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coco_mask_ref as ref  # noqa: E402
from multiposenet_amd import coco_records as cr  # noqa: E402
from tools.bench_predict_images import events_ms  # noqa: E402

SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (375, 500), (333, 500)]      # (h, w): COCO's common ones


def person_polygon(h, w, rng):
    k = int(rng.integers(10, 40))
    cx, cy, r = rng.uniform(0.1 * w, 0.9 * w), rng.uniform(0.1 * h, 0.9 * h), rng.uniform(15, 110)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * rng.uniform(0.5, 1.0, k)
    x = np.clip(cx + rad * np.cos(ang), 0, w)
    y = np.clip(cy + 1.6 * rad * np.sin(ang), 0, h)
    return np.stack([x, y], 1).round(2)


def synthetic_annotations(h, w, persons, rng, image_id):
    anns = []
    for _ in range(persons):
        p = person_polygon(h, w, rng)
        x0, y0, x1, y1 = p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()
        labelled = int(rng.choice([0, 1, 9, 17], p=[0.15, 0.05, 0.3, 0.5]))
        kp = []
        for j in range(17):
            kp += [int(rng.uniform(x0, x1)), int(rng.uniform(y0, y1)), 2] if j < labelled else [0, 0, 0]
        anns.append({'image_id': image_id, 'category_id': 1, 'iscrowd': 0, 'bbox': [float(x0), float(y0), float(x1 - x0), float(y1 - y0)],
                     'area': float((x1 - x0) * (y1 - y0) / 2), 'num_keypoints': labelled, 'keypoints': kp,
                     'segmentation': [p.reshape(-1).tolist()]})
    return anns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--persons", type=int, default=4, help="persons per image (COCO train2017: about 260 k on 64 k images)")
    ap.add_argument("--images", type=int, default=256, help="images of the write_shards leg")
    ap.add_argument("--host-images", type=int, default=8, help="images the numpy transcription is timed on")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "coco_masks.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coco_masks: no GPU (a measurement path does not fall back)")
    rng = np.random.default_rng(0)
    items = []
    for i in range(args.batch):
        h, w = SIZES[i % len(SIZES)]
        items.append((h, w, cr.apply_record_rules(synthetic_annotations(h, w, args.persons, rng, i), h, w)))
    rasterizer = cr.CocoMaskRasterizer(args.batch)
    got = rasterizer.rasterize(items)                                              # warm-up: buffers, tap tables
    t0 = time.perf_counter()
    want = ref.rasterize(items[:args.host_images])
    host_ms = (time.perf_counter() - t0) * 1e3 / max(args.host_images, 1)
    if not all(np.array_equal(a, b) for a, b in zip(got, want)):
        raise SystemExit("bench_coco_masks: the device's packed masks differ from the transcription's")
    batch = cr._Batch(items, False)
    rasterizer.upload(batch)
    device_ms = [events_ms(lambda: rasterizer.launch(batch), 20) for _ in range(args.rounds)]
    wall_ms = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rasterizer.rasterize(items)
        wall_ms.append((time.perf_counter() - t0) * 1e3)

    from PIL import Image
    shard_rates = []
    with tempfile.TemporaryDirectory() as tmp:
        images_dir = os.path.join(tmp, "images")
        os.makedirs(images_dir)
        coco = {'images': [], 'annotations': [], 'categories': [{'id': 1, 'name': 'person'}]}
        for i in range(args.images):
            h, w = SIZES[i % len(SIZES)]
            yy, xx = np.arange(h) // 8, np.arange(w) // 8
            pixels = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)[yy][:, xx]
            Image.fromarray(np.ascontiguousarray(pixels)).save(os.path.join(images_dir, f"{i:06d}.jpg"), quality=90)
            coco['images'].append({'id': i, 'file_name': f"{i:06d}.jpg", 'height': h, 'width': w})
            coco['annotations'] += synthetic_annotations(h, w, args.persons, rng, i)
        path = os.path.join(tmp, "person_keypoints_synthetic.json")
        with open(path, "w") as f:
            json.dump(coco, f)
        report = None
        for r in range(args.rounds):
            t0 = time.perf_counter()
            report = cr.write_shards(path, images_dir, os.path.join(tmp, f"out{r}"), 4, seed=0, batch=args.batch)
            shard_rates.append(report['images'] / (time.perf_counter() - t0))

    def spread(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "persons_per_image": args.persons, "sizes": SIZES,
              "parts_per_batch": batch.num_parts, "vertices_per_batch": batch.num_xy // 2,
              "tables_h2d_bytes_per_batch": batch.nbytes, "packed_d2h_bytes_per_batch": batch.packed_bytes,
              "device_ms_per_batch": spread(device_ms), "rasterize_ms_per_batch": spread(wall_ms),
              "rasterize_images_per_s": args.batch / (statistics.median(wall_ms) * 1e-3),
              "write_shards": {"images": args.images, "report": report, "images_per_s": spread(shard_rates)},
              "host": {"what": "tests/coco_mask_ref.py rasterize (plain-loop numpy transcription, one thread)",
                       "images": args.host_images, "ms_per_image": host_ms},
              "device_speedup_over_host_masks": host_ms * args.batch / statistics.median(wall_ms)}
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
