"""Cost of the person detector's input pipeline: device time of one `mpn_detector_augment` launch beside the keypoint
kernel's, the host rates, and the pipeline's end-to-end rate.

    python tools/bench_detector_pipeline.py [--batch 32] [--iters 200] [--repeats 2]

Prints one JSON line. For each output size (512 x 512, the keypoint pipeline's, and 640 x 640, the detector's own) and the
same `batch` 640x480 sources: the device time per batch (HIP events over `iters` launches after warm-up) of
  keypoint      `mpn_keypoint_augment` on sampled descriptors (the yardstick),
  detector      `mpn_detector_augment` on sampled descriptors with MPN_AUGMENT_PAD cleared (at most 4 source reads per pixel),
  detector_pad  the same descriptors with MPN_AUGMENT_PAD set on every image (the 16-tap composition),
measured in that order, alternating, `repeats` times in one process (the spread between repeats is the noise to hold a
difference against). Then the bytes the detector kernel must move (f32 images written, uint8 sources read once) over its
time beside 6.3 TB/s (the rate a float4 copy reaches on the MI355X), the host ms per batch for sampling + packing, with PIL
the JPEG decode of the batch on NUM_PARALLEL_CALLS threads, and the images/s of `DetectorPipeline` (batch 16, 640 x 640,
in-memory sources) beside what the detector's train step consumes (16 images per 5.6 ms).
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
    from multiposenet_amd.detector.input_pipeline import DetectorPipeline, KeypointPipeline
    from multiposenet_amd.detector.input_pipeline import detector_augment as da
    from multiposenet_amd.detector.input_pipeline import keypoint_augment as ka
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    B = args.batch
    assert torch.cuda.is_available(), "bench_detector_pipeline measures on the GPU"
    rng = np.random.default_rng(0)
    h, w = 480, 640
    mh, mw = ka.mask_size(h, w)
    exs = []
    for _ in range(B):
        kp = np.stack([rng.integers(60, 420, (2, 17)), rng.integers(160, 500, (2, 17)), np.full((2, 17), 2)], 2)
        exs.append({"image": rng.integers(0, 256, (h, w, 3)).astype(np.uint8),
                    "boxes": np.array([[100, 150, 400, 330], [50, 350, 300, 520]], np.float32), "keypoints": kp.astype(np.int32),
                    "masks": np.packbits(rng.integers(0, 2, (mh, mw, 2)).astype(np.uint8))})
    dev = "cuda"

    def timed(launch):
        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    out = {"metric": "detector_augment", "batch": B, "src": [h, w], "iters": args.iters, "sizes": {}}
    for S in (512, 640):
        kpipe = KeypointPipeline(exs, True, {"batch_size": B, "image_size": (S, S)})
        dpipe = DetectorPipeline(exs, True, {"batch_size": B, "image_size": (S, S)})
        kdescs, _, _, kso, _ = kpipe.sample(np.random.default_rng(1), exs)
        host_ms = []
        src = np.zeros(B * (h * w * 3 + 16), np.uint8)
        srng = np.random.default_rng(1)
        for _ in range(20):      # host: sampling + packing into one staging buffer (a batch's cost besides decode)
            t0 = time.perf_counter()
            descs, boxes, _, so = dpipe.sample(srng, exs)
            for d, ex in zip(descs, exs):
                o = int(d["src_offset"])
                src[o:o + ex["image"].size] = ex["image"].reshape(-1)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert so == kso
        da.check_descriptors(descs, so, S, S)
        plain, padded = descs.copy(), descs.copy()
        plain["flags"] &= ~da.PAD
        prng = np.random.default_rng(2)
        for d in padded:
            _, _, (oy, ox, sh, sw) = da.random_pad(prng, np.zeros((0, 4), np.float32), S, S)
            d["pad_y"], d["pad_x"], d["pad_h"], d["pad_w"] = oy, ox, sh, sw
            d["pad_scale_y"], d["pad_scale_x"] = np.float32(S) / np.float32(sh), np.float32(S) / np.float32(sw)
            d["flags"] |= da.PAD
        da.check_descriptors(padded, so, S, S)
        msk = np.concatenate([np.pad(e["masks"], (0, (-e["masks"].size) % 16)) for e in exs])
        s_d, m_d = torch.from_numpy(src[:so].copy()).to(dev), torch.from_numpy(msk).to(dev)
        k_d = torch.from_numpy(kdescs.view(np.uint8).copy()).to(dev)
        p_d = torch.from_numpy(plain.view(np.uint8).copy()).to(dev)
        q_d = torch.from_numpy(padded.view(np.uint8).copy()).to(dev)
        img = torch.empty((B, S, S, 3), device=dev)
        lm = torch.empty((B, S // 4, S // 4), device=dev)
        sm = torch.empty_like(lm)

        def keypoint():
            _lib.call("mpn_keypoint_augment", _lib.ptr(s_d), _lib.ptr(m_d), _lib.ptr(k_d), B, S, S, _lib.ptr(img),
                      _lib.ptr(lm), _lib.ptr(sm), _lib.stream_ptr())

        def detector(d_d):
            return lambda: _lib.call("mpn_detector_augment", _lib.ptr(s_d), _lib.ptr(d_d), B, S, S, _lib.ptr(img),
                                     _lib.stream_ptr())
        legs = {"keypoint": keypoint, "detector": detector(p_d), "detector_pad": detector(q_d)}
        us = {k: [] for k in legs}
        for _ in range(args.repeats):
            for k, fn in legs.items():
                us[k].append(round(timed(fn), 2))
        nbytes = img.numel() * 4 + so
        best = min(us["detector"])
        out["sizes"][str(S)] = {
            "kernel_us": us, "bytes": int(nbytes), "frac_of_6p3TBps": round(nbytes / (best * 1e-6) / 6.3e12, 3),
            "keypoint_rotated_images": int(sum(bool(f & ka.ROTATE) for f in kdescs["flags"])),
            "host_sample_pack_ms_per_batch": round(float(np.median(host_ms[5:])), 2)}
    try:
        from PIL import Image
        from multiposenet_amd.detector.input_pipeline.tfrecord import decode_jpeg
        jpgs = []
        for e in exs:
            buf = io.BytesIO()
            Image.fromarray(e["image"]).save(buf, format="JPEG", quality=90)
            jpgs.append(buf.getvalue())
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
    # the pipeline end to end on in-memory sources (no decode): sampling, packing, copy, kernel
    it = DetectorPipeline(exs, True, {"batch_size": 16, "image_size": (640, 640)}).batches()
    for _ in range(5):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 30
    for _ in range(n):
        next(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["pipeline_images_per_s_in_memory"] = round(16 * n / dt, 1)
    out["detector_step_images_per_s"] = round(16 / 5.6e-3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
