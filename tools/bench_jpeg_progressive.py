"""Cost of the multi-scan JPEG host stage and of the four-component device stage: writes profiles/jpeg_progressive.json and
prints it.

    python tools/bench_jpeg_progressive.py [--batch 32] [--iters 200] [--out profiles/jpeg_progressive.json]

  host    per-image ms of `mpn_jpeg_scans_decode` (what decode='device' runs on the pool for a progressive file) against
          Pillow's full decode, same process, same bytes, the two legs alternating, on 1 thread and on 12: the images of a
          toy shard (tools/make_toy_tfrecords.py), re-encoded as progressive JPEGs at quality 85;
  device  us per batch of `mpn_jpeg_decode` by HIP events (`iters` launches after 20 warm-up) for a batch of 640x480 Adobe
          CMYK frames (four planes), beside the bytes it must move over 6.3 TB/s.
Without a GPU only the host part is measured ("device": null).
"""
import argparse
import ctypes
import importlib.util
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


def toy_progressive(count):
    """The images of `count` toy records, re-encoded as progressive JPEGs."""
    from PIL import Image
    from multiposenet_amd.detector.input_pipeline.tfrecord import parse_example
    spec = importlib.util.spec_from_file_location("make_toy_tfrecords", os.path.join(ROOT, "tools", "make_toy_tfrecords.py"))
    toy = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(toy)
    rng = np.random.default_rng(11)
    out = []
    for _ in range(count):
        image = bytes(parse_example(toy.toy_example(rng))["image"][0])
        buf = io.BytesIO()
        Image.open(io.BytesIO(image)).save(buf, format="JPEG", quality=85, progressive=True)
        out.append(buf.getvalue())
    return out


def cmyk_frames(count):
    from PIL import Image
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(count):
        im = np.stack([(xx * 255 // W), (yy * 255 // H), ((xx + yy) % 256)], 2).astype(np.int16)
        im = np.clip(im + rng.integers(-20, 21, im.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(im).convert("CMYK").save(buf, format="JPEG", quality=90)
        out.append(buf.getvalue())
    return out


def host_legs(jpegs, threads, rounds=3):
    from multiposenet_amd.inference import jpeg as J
    legs = {"scans_decode": J.scans_decode, "pillow": J.pillow_decode}
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
    entries = [J.scans_decode(j) for j in jpegs]
    assert all(int(e.desc[0]['components']) == 4 for e in entries)
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


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_progressive.json"))
    args = ap.parse_args()
    gpu = torch.cuda.is_available()
    jpegs = toy_progressive(args.batch)
    out = {"metric": "jpeg_progressive", "batch": args.batch, "cpus": len(os.sched_getaffinity(0)), "gpu": gpu,
           "progressive": {"quality": 85, "jpeg_bytes_per_image": int(np.mean([len(j) for j in jpegs])),
                           "host": {f"threads_{t}": host_legs(jpegs, t) for t in (1, THREADS)}},
           "cmyk": {"src": [H, W], "quality": 90, "device": device_leg(cmyk_frames(args.batch), args.iters) if gpu else None}}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
