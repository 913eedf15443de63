"""Cost of the JPEG decode, host stage and device stage, beside Pillow's: writes profiles/jpeg_decode.json and prints it.

    python tools/bench_jpeg_decode.py [--batch 32] [--iters 200] [--out profiles/jpeg_decode.json]

640x480 4:2:0 quality-90 JPEGs of two kinds: 'photo' (the photograph-like content of tools/make_toy_tfrecords.py) and
'noise' (uniform random bytes, the worst case for an entropy decoder, which DESIGN.md sections 9 and 11 used).
  host        per-image ms of `mpn_jpeg_entropy_decode` (the host stage of decode='device') against Pillow's full decode,
              same process, same bytes, the two legs alternating, on 1 thread and on 12 (section 9's count);
  device      us per batch of `mpn_jpeg_decode` by HIP events (`iters` launches after 20 warm-up) beside the bytes it must move
              (int16 coefficients read, uint8 planes written and read, RGB written) over 6.3 TB/s;
  end to end  images/s of `KeypointPipeline` (batch 32, 512 x 512) on in-memory records that hold JPEG bytes, decode='host'
              and decode='device', beside what the keypoint step consumes.
Without a GPU only the host part is measured ("device": null, "pipeline": null).
"""
import argparse
import ctypes
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640
THREADS = 12
KEYPOINT_STEP_IMAGES_PER_S = 4300.0


def make_jpegs(kind, count, rng):
    from PIL import Image
    out = []
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(count):
        if kind == 'noise':
            im = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        else:
            im = np.stack([(xx * 255 // W), (yy * 255 // H), ((xx + yy) % 256)], 2).astype(np.int16)
            im = np.clip(im + rng.integers(-20, 21, im.shape), 0, 255).astype(np.uint8)
            y0, x0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
            im[y0:y0 + H // 3, x0:x0 + W // 3] //= 2
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format="JPEG", quality=90, subsampling=2)
        out.append(buf.getvalue())
    return out


def host_legs(jpegs, threads, rounds=3):
    from multiposenet_amd.inference import jpeg as J
    legs = {"entropy_decode": J.entropy_decode, "pillow": J.pillow_decode}
    ms = {k: [] for k in legs}
    with ThreadPoolExecutor(threads) as pool:
        for fn in legs.values():
            list(pool.map(fn, jpegs))
        for _ in range(rounds):
            for k, fn in legs.items():                      # alternating
                t0 = time.perf_counter()
                list(pool.map(fn, jpegs))
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"batch_ms": [round(v, 2) for v in vs], "ms_per_image": round(min(vs) / len(jpegs), 3),
                "images_per_s": round(len(jpegs) / min(vs) * 1e3, 1)} for k, vs in ms.items()}


def device_leg(jpegs, iters):
    import torch
    from multiposenet_amd import _lib
    from multiposenet_amd.inference import jpeg as J
    entries = [J.entropy_decode(j) for j in jpegs]
    offsets = [i * ((H * W * 3 + 15) // 16 * 16) for i in range(len(entries))]
    sources = torch.zeros(offsets[-1] + H * W * 3 + 16, dtype=torch.uint8, device="cuda")
    dec = J.JpegBatchDecoder("cuda:0")
    dec.decode(entries, sources, offsets)                   # stages coefficients and descriptors on the device
    torch.cuda.synchronize()
    _, _, lay = dec.plan(entries, offsets)
    base = dec._buf['dev'].data_ptr()

    def launch():
        _lib.call("mpn_jpeg_decode", ctypes.c_void_p(base + lay['coef_base']), lay['coef_bytes'], ctypes.c_void_p(base), len(entries),
                  _lib.ptr(sources), sources.numel(), _lib.ptr(dec._buf['work']), dec._buf['work'].numel(), _lib.stream_ptr())
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    nbytes = lay['coef_bytes'] + 2 * lay['work_bytes'] + len(entries) * H * W * 3
    return {"batch_us": round(us, 2), "images_per_s": round(len(entries) / us * 1e6, 1), "bytes": int(nbytes),
            "frac_of_6p3TBps": round(nbytes / (us * 1e-6) / 6.3e12, 4), "h2d_bytes": int(lay['stage_bytes'])}


def pipeline_leg(jpegs, mode, batch):
    import torch
    from multiposenet_amd.detector.input_pipeline import KeypointPipeline
    from multiposenet_amd.detector.input_pipeline import keypoint_augment as ka
    rng = np.random.default_rng(3)
    mh, mw = ka.mask_size(H, W)
    exs = []
    for j in jpegs:
        kp = np.stack([rng.integers(60, 420, (2, 17)), rng.integers(160, 500, (2, 17)), np.full((2, 17), 2)], 2)
        exs.append({"image": j, "boxes": np.array([[100, 150, 400, 330], [50, 350, 300, 520]], np.float32),
                    "keypoints": kp.astype(np.int32), "masks": np.packbits(rng.integers(0, 2, (mh, mw, 2)).astype(np.uint8))})
    it = KeypointPipeline(exs, True, {"batch_size": batch, "image_size": (512, 512)}, num_threads=THREADS, decode=mode).batches()
    for _ in range(4):
        next(it)
    torch.cuda.synchronize()
    n = 20
    t0 = time.perf_counter()
    for _ in range(n):
        next(it)
    torch.cuda.synchronize()
    return round(batch * n / (time.perf_counter() - t0), 1)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.json"))
    args = ap.parse_args()
    gpu = torch.cuda.is_available()
    out = {"metric": "jpeg_decode", "src": [H, W], "sampling": "4:2:0", "quality": 90, "batch": args.batch,
           "cpus": len(os.sched_getaffinity(0)), "gpu": gpu, "kinds": {}}
    rng = np.random.default_rng(0)
    for kind in ("photo", "noise"):
        jpegs = make_jpegs(kind, args.batch, rng)
        res = {"jpeg_bytes_per_image": int(np.mean([len(j) for j in jpegs])),
               "host": {f"threads_{t}": host_legs(jpegs, t) for t in (1, THREADS)},
               "device": device_leg(jpegs, args.iters) if gpu else None,
               "pipeline_images_per_s": {m: pipeline_leg(jpegs, m, args.batch) for m in ("host", "device")} if gpu else None}
        out["kinds"][kind] = res
    out["keypoint_step_images_per_s"] = KEYPOINT_STEP_IMAGES_PER_S
    text = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
