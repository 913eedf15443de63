"""Images per second from decoded camera frames to persons in the frames' own coordinates: a host resize in front of
`Detector.predict_batch` (what a user writes without `predict_images`) against `Detector.predict_images`, same process, same GPU.

    timeout -k 10 400 python tools/bench_predict_images.py [--batch 16] [--source 1080 1920] [--size 640] [--batches 8] [--rounds 5]
                                                           [--out profiles/predict_images.json]

(one process, one GPU step: run it under a `timeout` of its own as above; the default run takes about a minute.)

Legs, numpy in / numpy out, wall clock (time.perf_counter around calls that end in a device synchronise):
  A  host_resize_predict_batch   every frame resized on the host to size x size, then predict_batch. The host resize is
                                 Pillow's `Image.resize` (inference/predict.ipynb cell 6) when Pillow is importable, otherwise
                                 torch's CPU interpolate(mode='bicubic', antialias=True) on the uint8 frame; the JSON names which.
  B  predict_images              the resize on the device, inside the captured graph.
Both are warmed up (graph capture, buffers, pinned staging, tables), then ALTERNATE over `--rounds` rounds of `--batches`
batches; the figure of a leg is its median round. Device time comes from HIP events around back-to-back work without host
copies in between: replays of predict_images' whole graph, and the resize launches alone on the same buffers. A run without a
GPU fails; nothing here falls back.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)


def host_resizer(size):
    try:
        from PIL import Image
        import PIL
        return f"Pillow {PIL.__version__} Image.resize (bicubic, one thread)", \
            lambda im: np.asarray(Image.fromarray(im).resize((size, size)))
    except ImportError:
        def resize(im):
            x = torch.from_numpy(im).permute(2, 0, 1)[None]
            y = torch.nn.functional.interpolate(x, size=(size, size), mode="bicubic", antialias=True, align_corners=False)
            return y[0].permute(1, 2, 0).contiguous().numpy()
        return f"torch {torch.__version__} CPU interpolate(bicubic, antialias=True) on uint8, {torch.get_num_threads()} threads", resize


def events_ms(fn, repeats):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(repeats):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=8, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "predict_images.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict_images: no GPU (a measurement path does not fall back)")
    from multiposenet_amd import _lib
    from multiposenet_amd.inference import resample
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    # frames with structure at the network's scale: size x size noise (what tools/bench_inference_batch.py feeds the network)
    # enlarged to the source size by pixel repetition - plain source-resolution noise would average out to grey in the resize
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    resizer_name, resize = host_resizer(s)

    def leg_a():
        persons = 0
        for _ in range(args.batches):
            batch = np.stack([resize(f) for f in frames])
            persons += sum(len(o["boxes"]) for o in det.predict_batch(batch, score_threshold=thr, return_heatmaps=False))
        return persons

    def leg_b():
        persons = 0
        for _ in range(args.batches):
            persons += sum(len(o["boxes"]) for o in det.predict_images(frames, size=(s, s), score_threshold=thr))
        return persons

    legs = [("host_resize_predict_batch", leg_a), ("predict_images", leg_b)]
    persons = {name: fn() for name, fn in legs}                   # warm-up: every shape the timed window uses
    t0 = time.perf_counter()
    for f in frames:
        resize(f)
    host_resize_ms = (time.perf_counter() - t0) * 1e3 / b
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:                                      # alternate the legs inside a round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    key = next(k for k in det._graphs if isinstance(k, tuple) and k[0] == "images")
    ent = det._graphs[key]
    meta = ent.meta
    tables = meta[b * (resample.DESC_WORDS + 4):]

    def resize_only():
        _lib.call("mpn_image_resize", _lib.ptr(ent.sources), _lib.ptr(tables), _lib.ptr(meta), b, s, s, _lib.ptr(ent.x),
                  _lib.ptr(ent.work), ent.work.numel(), _lib.stream_ptr())

    graph_ms = [events_ms(ent.graph.replay, 20) / b for _ in range(args.rounds)]
    resize_ms = [events_ms(resize_only, 20) / b for _ in range(args.rounds)]
    batch_graph = det._graphs[(b, s, s, thr)].graph
    batch_ms = [events_ms(batch_graph.replay, 20) / b for _ in range(args.rounds)]
    plan = resample.Plan([f.shape[:2] for f in frames], s, s)
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": [sh, sw], "size": [s, s],
              "score_threshold": thr, "batches_per_leg_round": args.batches, "rounds": args.rounds,
              "persons_per_image": {k: v / (args.batches * b) for k, v in persons.items()},
              "host_resize": resizer_name, "host_resize_ms_per_image": host_resize_ms,
              "h2d_bytes_per_batch": {"sources": int(plan.stage_bytes), "descriptors_extents_tables": int(plan.meta_words * 4),
                                      "predict_batch_input": b * s * s * 3},
              "legs": {}, "device_ms_per_image": {
                  "predict_images_graph": {"median": statistics.median(graph_ms), "min": min(graph_ms), "max": max(graph_ms)},
                  "resize_launches": {"median": statistics.median(resize_ms), "min": min(resize_ms), "max": max(resize_ms)},
                  "predict_batch_graph": {"median": statistics.median(batch_ms), "min": min(batch_ms), "max": max(batch_ms)}}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": {"median": statistics.median(w) * 1e3, "min": w[0] * 1e3, "max": w[-1] * 1e3},
                                "wall_images_per_s": 1.0 / statistics.median(w)}
    result["predict_images_speedup"] = (result["legs"]["predict_images"]["wall_images_per_s"]
                                        / result["legs"]["host_resize_predict_batch"]["wall_images_per_s"])
    result["resize_share_of_graph_device_time"] = statistics.median(resize_ms) / statistics.median(graph_ms)
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
