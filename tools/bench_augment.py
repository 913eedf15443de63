"""Cost of the keypoint input pipeline's augmentation: device time of one `mpn_keypoint_augment` launch and the host rates.

    python tools/bench_augment.py [--batch 32] [--size 512] [--iters 200]

Prints one JSON line: the kernel's device time per batch (HIP events after warm-up) of `batch` 640x480 sources to
size x size, the bytes it must move (f32 images + masks written, uint8 sources + packed masks read once) and that
over 6.3 TB/s (the rate a float4 copy reaches on the MI355X); the host ms per batch for sampling + descriptor packing
(no decode) and, with PIL present, for JPEG decode of the batch on NUM_PARALLEL_CALLS threads.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from multiposenet_amd import _lib
    from multiposenet_amd.detector.constants import NUM_PARALLEL_CALLS
    from multiposenet_amd.detector.input_pipeline import keypoint_augment as ka
    from multiposenet_amd.detector.input_pipeline.keypoints_detector_pipeline import KeypointPipeline
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    B, S = args.batch, args.size
    assert torch.cuda.is_available(), "bench_augment measures on the GPU"
    rng = np.random.default_rng(0)
    h, w = 480, 640
    exs = []
    for _ in range(B):
        boxes = np.array([[100, 150, 400, 330], [50, 350, 300, 520]], np.float32)
        kp = np.stack([rng.integers(60, 420, (2, 17)), rng.integers(160, 500, (2, 17)), np.full((2, 17), 2)], 2)
        mh, mw = ka.mask_size(h, w)
        exs.append({"image": rng.integers(0, 256, (h, w, 3)).astype(np.uint8), "boxes": boxes,
                    "keypoints": kp.astype(np.int32), "masks": np.packbits(rng.integers(0, 2, (mh, mw, 2)).astype(np.uint8))})
    pipe = KeypointPipeline(exs, True, {"batch_size": B, "image_size": (S, S)})
    # host: sampling + packing into one staging buffer (what a batch costs the main thread besides decode)
    host_ms = []
    src = np.empty(B * (h * w * 3 + 16), np.uint8)
    for i in range(20):
        t0 = time.perf_counter()
        descs, people, size, so, mo = pipe.sample(rng, exs)
        for d, ex in zip(descs, exs):
            o = int(d["src_offset"])
            src[o:o + ex["image"].size] = ex["image"].reshape(-1)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    host = float(np.median(host_ms[5:]))
    # device: one launch on fixed descriptors
    msk = np.concatenate([np.pad(e["masks"], (0, (-e["masks"].size) % 16)) for e in exs])
    dev = "cuda"
    s_d = torch.from_numpy(src[:so]).to(dev)
    m_d = torch.from_numpy(msk).to(dev)
    d_d = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
    img = torch.empty((B, S, S, 3), device=dev)
    lm = torch.empty((B, S // 4, S // 4), device=dev)
    sm = torch.empty_like(lm)

    def launch():
        _lib.call("mpn_keypoint_augment", _lib.ptr(s_d), _lib.ptr(m_d), _lib.ptr(d_d), B, S, S, _lib.ptr(img),
                  _lib.ptr(lm), _lib.ptr(sm), _lib.stream_ptr())
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    kernel_us = e0.elapsed_time(e1) * 1e3 / args.iters
    nbytes = img.numel() * 4 + 2 * lm.numel() * 4 + so + msk.size
    out = {"metric": "keypoint_augment", "batch": B, "out": [S, S], "src": [h, w],
           "kernel_us": round(kernel_us, 2), "bytes": int(nbytes),
           "frac_of_6p3TBps": round(nbytes / (kernel_us * 1e-6) / 6.3e12, 3),
           "host_sample_pack_ms_per_batch": round(host, 2),
           "host_sample_pack_images_per_s": round(B / host * 1e3, 1)}
    try:
        from PIL import Image
        jpgs = []
        for e in exs:
            buf = io.BytesIO()
            Image.fromarray(e["image"]).save(buf, format="JPEG", quality=90)
            jpgs.append(buf.getvalue())
        from multiposenet_amd.detector.input_pipeline.tfrecord import decode_jpeg
        with ThreadPoolExecutor(NUM_PARALLEL_CALLS) as pool:
            list(pool.map(decode_jpeg, jpgs))
            t0 = time.perf_counter()
            for _ in range(5):
                list(pool.map(decode_jpeg, jpgs))
            dec = (time.perf_counter() - t0) / 5 * 1e3
        out["host_decode_ms_per_batch"] = round(dec, 2)
        out["host_decode_images_per_s"] = round(B / dec * 1e3, 1)
        out["decode_threads"] = NUM_PARALLEL_CALLS
        out["note"] = "decode of random-noise JPEGs (a worst case for the entropy decoder)"
    except ImportError:
        out["host_decode_ms_per_batch"] = None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
