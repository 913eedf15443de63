"""Writes a few TFRecord shards of COCO-shaped keypoint records from a seed - smoke data for
`python -m multiposenet_amd.train_keypoints --train-dataset OUT --val-dataset OUT` without COCO.

    python tools/make_toy_tfrecords.py OUT [--shards 2] [--records 16] [--seed 0]

Each record follows the contract of the reference's data/create_tfrecords.py:89-94: a JPEG `image` of random size,
`num_persons`, absolute `boxes` (ymin, xmin, ymax, xmax), `keypoints` (y, x, v) and the np.packbits `masks` of
[ceil(H/4), ceil(W/4), 2]. Needs PIL for the JPEG encoding.
"""
import argparse
import io
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiposenet_amd.detector.input_pipeline.tfrecord import encode_example, frame_record  # noqa: E402


def toy_example(rng):
    from PIL import Image
    h, w = int(rng.integers(200, 481)), int(rng.integers(240, 641))
    yy, xx = np.mgrid[0:h, 0:w]
    image = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) % 256)], 2).astype(np.uint8)
    image = np.clip(image.astype(np.int16) + rng.integers(-20, 21, image.shape), 0, 255).astype(np.uint8)
    p = int(rng.integers(1, 5))
    boxes, kps = [], []
    mh, mw = math.ceil(h / 4), math.ceil(w / 4)
    seg = np.zeros((mh, mw), bool)
    for _ in range(p):
        bh, bw = rng.uniform(0.2, 0.8) * h, rng.uniform(0.1, 0.5) * w
        y0, x0 = rng.uniform(0, h - bh), rng.uniform(0, w - bw)
        boxes.append((y0, x0, y0 + bh, x0 + bw))
        y = np.clip(rng.uniform(y0, y0 + bh, 17), 0, h - 1).astype(np.int64)
        x = np.clip(rng.uniform(x0, x0 + bw, 17), 0, w - 1).astype(np.int64)
        v = rng.integers(0, 3, 17)
        kps.append(np.stack([y, x, v], 1))
        seg[int(y0) // 4:int(y0 + bh) // 4 + 1, int(x0) // 4:int(x0 + bw) // 4 + 1] = True
        image[int(y0):int(y0 + bh), int(x0):int(x0 + bw)] //= 2
    loss = rng.random((mh, mw)) < 0.97
    masks = np.packbits(np.stack([loss, seg], 2).astype(np.uint8) > 0)
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format="JPEG", quality=90)
    return encode_example({"image": buf.getvalue(), "num_persons": np.array([p], np.int64),
                           "boxes": np.array(boxes, np.float32).reshape(-1),
                           "keypoints": np.stack(kps).astype(np.int64).reshape(-1),
                           "masks": masks.tobytes()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--shards", type=int, default=2)
    ap.add_argument("--records", type=int, default=16, help="records per shard")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    rng = np.random.default_rng(args.seed)
    for s in range(args.shards):
        path = os.path.join(args.out, f"shard-{s:04d}.tfrecords")
        with open(path, "wb") as f:
            for _ in range(args.records):
                f.write(frame_record(toy_example(rng)))
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
