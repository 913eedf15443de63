"""Annotated frames as JPEG files: `Detector.predict_images(annotate='jpeg')` (draw and encode on the device, inside the
captured graph; only compressed bytes cross PCIe) against what it replaces - `predict_images(annotate=True)` followed by
Pillow's encoder on the host, on 1 and on 12 threads - same process, same GPU; and the device time of the two encode calls.

    timeout -k 10 900 python tools/bench_jpeg_encode.py [--batch 16] [--source 1080 1920] [--size 640] [--quality 75]
                                                        [--subsampling 4:2:0] [--batches 4] [--rounds 5] [--replays 50]
                                                        [--out profiles/jpeg_encode.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Setup as tools/bench_draw.py: bf16, 25 persons per image (the lively head), frames made as tools/bench_predict_images.py
makes them. Legs, numpy in / bytes out, wall clock:
  A1 annotate_then_pillow_1_thread    annotate=True, then `Image.fromarray(frame[..., :3]).save(buf, "JPEG", ...)` per frame.
  A12 annotate_then_pillow_12_threads the same with the frames of a batch spread over a pool of 12 threads.
  B  annotate_jpeg                    annotate='jpeg'.
All are warmed up, then ALTERNATE over `--rounds` rounds of `--batches` batches; the figure of a leg is its median round.
Device time (HIP events, warm, `--replays` launches back to back) of mpn_jpeg_forward and of mpn_jpeg_entropy_encode on the
graph's own buffers. Bytes copied device-to-host per frame: the RGBA frame in A, the record of the streams plus the
compressed bytes in B. The files of B are compared with those of A. A run without a GPU fails; nothing here falls back.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiposenet_amd import _lib  # noqa: E402
from multiposenet_amd.inference import jpeg as J  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--subsampling", default="4:2:0", choices=sorted(J.SAMPLING))
    ap.add_argument("--batches", type=int, default=4, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "jpeg_encode.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode: no GPU (a measurement path does not fall back)")
    import PIL
    from PIL import Image
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr, q, sub = args.batch, args.size, args.threshold, args.quality, args.subsampling
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    pillow_sub = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}[sub]

    def host_encode(frame):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame[..., :3])).save(buf, "JPEG", quality=q, subsampling=pillow_sub)
        return buf.getvalue()

    pool = ThreadPoolExecutor(max_workers=12)

    def leg_a(threads):
        persons = det.predict_images(frames, size=(s, s), score_threshold=thr, annotate=True)
        drawn = [p.pop("annotated") for p in persons]
        files = [host_encode(f) for f in drawn] if threads == 1 else list(pool.map(host_encode, drawn))
        for p, f in zip(persons, files):
            p["annotated_jpeg"] = f
        return persons

    def leg_b():
        return det.predict_images(frames, size=(s, s), score_threshold=thr, annotate='jpeg', jpeg_quality=q, jpeg_subsampling=sub)

    legs = [("annotate_jpeg", leg_b), ("annotate_then_pillow_1_thread", lambda: leg_a(1)),
            ("annotate_then_pillow_12_threads", lambda: leg_a(12))]
    first = {name: fn() for name, fn in legs}                       # warm-up: graphs, buffers, pinned staging
    equal = all(x["annotated_jpeg"] == y["annotated_jpeg"] for x, y in
                zip(first["annotate_jpeg"], first["annotate_then_pillow_1_thread"]))
    file_bytes = [len(p["annotated_jpeg"]) for p in first["annotate_jpeg"]]
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    pool.shutdown()

    ent = next(v for k, v in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and "jpeg" in k)
    enc, plan, rgba = ent.encode, ent.encode_plan, ent.outs["encoded"]
    fallbacks = enc.fallbacks
    scan_bytes = [n - len(h) for n, h in zip(file_bytes, plan.headers)]
    if fallbacks == 0:                                              # what `collect` copied: the records and the streams, no more
        assert enc.copied_bytes == sum(scan_bytes) + enc.n * J.RECORD_BYTES, (enc.copied_bytes, sum(scan_bytes))
    st = _lib.stream_ptr

    def forward():
        _lib.call("mpn_jpeg_forward", _lib.ptr(rgba), rgba.numel(), _lib.ptr(enc._descs), enc.n, _lib.ptr(enc._coefs),
                  enc._coefs.numel(), st())

    def entropy():
        _lib.call("mpn_jpeg_entropy_encode", _lib.ptr(enc._coefs), enc._coefs.numel(), _lib.ptr(enc._descs), enc.n, _lib.ptr(enc._out),
                  enc._out.numel(), _lib.ptr(enc._records), _lib.ptr(enc._work), enc._work.numel(), st())

    forward_ms = [events_ms(forward, args.replays) for _ in range(args.rounds)]
    entropy_ms = [events_ms(entropy, args.replays) for _ in range(args.rounds)]
    graph_ms = [events_ms(ent.graph.replay, 20) for _ in range(args.rounds)]
    drawn_graph = next(v for k, v in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and k[-1] == "annotate").graph
    drawn_graph_ms = [events_ms(drawn_graph.replay, 20) for _ in range(args.rounds)]
    pixels = sum(f.shape[0] * f.shape[1] for f in frames)

    med = statistics.median
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": [sh, sw], "size": [s, s],
              "quality": q, "subsampling": sub, "score_threshold": thr, "batches_per_leg_round": args.batches, "rounds": args.rounds,
              "replays": args.replays, "host_encoder": f"Pillow {PIL.__version__}", "device_files_equal_host_files": equal,
              "images_left_to_the_host_fallback": fallbacks,
              "file_bytes_per_image": {"mean": sum(file_bytes) / b, "min": min(file_bytes), "max": max(file_bytes)},
              "encode_calls": {"mpn_jpeg_forward_device_ms_per_batch": stats(forward_ms),
                               "mpn_jpeg_entropy_encode_device_ms_per_batch": stats(entropy_ms),
                               "rgba_bytes_read_per_batch": 4 * pixels},
              "graph_device_ms_per_image": {"annotate_jpeg": {k: v / b for k, v in stats(graph_ms).items()},
                                            "annotate": {k: v / b for k, v in stats(drawn_graph_ms).items()}},
              "device_to_host_bytes_per_frame": {"annotate": 4 * pixels / b, "annotate_jpeg": enc.copied_bytes / b},
              "legs": {}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": {"median": med(w) * 1e3, "min": w[0] * 1e3, "max": w[-1] * 1e3},
                                "wall_images_per_s": 1.0 / med(w)}
    for other in ("annotate_then_pillow_1_thread", "annotate_then_pillow_12_threads"):
        result[f"annotate_jpeg_over_{other}"] = (result["legs"]["annotate_jpeg"]["wall_images_per_s"]
                                                 / result["legs"][other]["wall_images_per_s"])
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
