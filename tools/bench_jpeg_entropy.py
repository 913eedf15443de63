"""Cost of the JPEG entropy stage on the device beside the host's: writes profiles/jpeg_entropy.json and prints it.

    python tools/bench_jpeg_entropy.py [--batch 32] [--iters 200] [--out profiles/jpeg_entropy.json]

Batches of in-memory 640x480 4:2:0 quality-90 JPEGs, 'photo' and 'noise' (tools/bench_jpeg_decode.py makes them).
  device      us per batch of `mpn_jpeg_entropy_decode_device` by HIP events (`iters` launches after 20 warm-up), the passes
              its records report and the images that would take the fallback;
  host        `mpn_jpeg_entropy_decode` on 1 and 12 threads in the same run, the legs alternating with the device leg's rounds;
  upload      bytes staged per batch in both modes (files and header descriptors against coefficients and descriptors);
  end to end  images/s of `KeypointPipeline` (batch 32, 512 x 512) with decode='host', decode='device' and
              decode='device', entropy='device'.
Needs a GPU. No threshold is applied: the file is what a later change of the default is argued from.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_jpeg_decode as D  # noqa: E402


def host_ms(jpegs, pool):
    from multiposenet_amd.inference import jpeg as J
    t0 = time.perf_counter()
    list(pool.map(J.entropy_decode, jpegs))
    return (time.perf_counter() - t0) * 1e3


def device_us(jpegs, iters, rounds):
    """Stages the batch once. Returns (one_round, decoder, fallbacks, staging layout): one_round() times `iters / rounds`
    launches of the entropy call between two events and returns the us per launch."""
    import torch
    from multiposenet_amd.inference import jpeg as J
    scans = [J.scan_prepare(j) for j in jpegs]
    offsets = [i * ((D.H * D.W * 3 + 15) // 16 * 16) for i in range(len(scans))]
    sources = torch.zeros(offsets[-1] + D.H * D.W * 3 + 16, dtype=torch.uint8, device="cuda")
    dec = J.JpegBatchDecoder("cuda:0")
    bad = dec.decode_scans(scans, sources, offsets, torch.cuda.current_stream())     # stages files and descriptors
    lay, launch = dec.scan_layout, dec.entropy_launch
    for _ in range(20):
        launch()
    torch.cuda.synchronize()

    def one_round():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters // rounds):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (iters // rounds)
    return one_round, dec, len(bad), lay


def pipeline_leg(jpegs, batch, **modes):
    import torch
    from multiposenet_amd.detector.input_pipeline import KeypointPipeline
    from multiposenet_amd.detector.input_pipeline import keypoint_augment as ka
    rng = np.random.default_rng(3)
    mh, mw = ka.mask_size(D.H, D.W)
    exs = []
    for j in jpegs:
        kp = np.stack([rng.integers(60, 420, (2, 17)), rng.integers(160, 500, (2, 17)), np.full((2, 17), 2)], 2)
        exs.append({"image": j, "boxes": np.array([[100, 150, 400, 330], [50, 350, 300, 520]], np.float32),
                    "keypoints": kp.astype(np.int32), "masks": np.packbits(rng.integers(0, 2, (mh, mw, 2)).astype(np.uint8))})
    it = KeypointPipeline(exs, True, {"batch_size": batch, "image_size": (512, 512)}, num_threads=D.THREADS, **modes).batches()
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
    from multiposenet_amd.inference import jpeg as J
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_entropy.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_entropy: needs a GPU")
    out = {"metric": "jpeg_entropy", "src": [D.H, D.W], "sampling": "4:2:0", "quality": 90, "batch": args.batch,
           "iters": args.iters, "max_passes": J.MAX_PASSES, "cpus": len(os.sched_getaffinity(0)), "kinds": {}}
    rng = np.random.default_rng(0)
    rounds = 4
    for kind in ("photo", "noise"):
        jpegs = D.make_jpegs(kind, args.batch, rng)
        one_round, dec, fallbacks, lay = device_us(jpegs, args.iters, rounds)
        us, ms = [], {1: [], D.THREADS: []}
        with ThreadPoolExecutor(1) as p1, ThreadPoolExecutor(D.THREADS) as pn:
            host_ms(jpegs, p1), host_ms(jpegs, pn)
            for _ in range(rounds):                             # the legs alternate
                us.append(one_round())
                ms[1].append(host_ms(jpegs, p1))
                ms[D.THREADS].append(host_ms(jpegs, pn))
        entries = [J.entropy_decode(j) for j in jpegs]
        _, _, host_lay = J.JpegBatchDecoder.plan(entries, [0] * len(entries))
        out["kinds"][kind] = {
            "jpeg_bytes_per_image": int(np.mean([len(j) for j in jpegs])),
            "device": {"batch_us_rounds": [round(v, 2) for v in us], "batch_us": round(min(us), 2),
                       "images_per_s": round(args.batch / min(us) * 1e6, 1), "passes": dec.records['passes'].tolist(),
                       "fallbacks": fallbacks},
            "host": {f"threads_{t}": {"batch_ms_rounds": [round(v, 2) for v in vs], "ms_per_image": round(min(vs) / args.batch, 3),
                                      "images_per_s": round(args.batch / min(vs) * 1e3, 1)} for t, vs in ms.items()},
            "upload_bytes_per_batch": {"entropy_host": int(host_lay['stage_bytes']), "entropy_device": int(lay['stage_bytes'])},
            "pipeline_images_per_s": {"host": pipeline_leg(jpegs, args.batch, decode='host'),
                                      "device": pipeline_leg(jpegs, args.batch, decode='device'),
                                      "device_entropy_device": pipeline_leg(jpegs, args.batch, decode='device', entropy='device')}}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
