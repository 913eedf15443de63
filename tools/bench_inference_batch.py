"""Images per second of `Detector.predict_batch` against a loop of `Detector.__call__`, same process, same GPU.

    python tools/bench_inference_batch.py [--size 640] [--images 256] [--rounds 5] [--out profiles/inference_batch.json]

Legs: the `__call__` loop (the single-image path, one hipGraph replay and its host round trips per image) and `predict_batch` at
b in {1, 4, 16, 32}, each with and without the heatmaps in the result. Every leg is warmed up (graph capture, buffers, pinned
staging), then the legs ALTERNATE over `--rounds` rounds of `--images` images each; the figure of a leg is its median round.

Two clocks per leg:
  wall    time.perf_counter around the calls, numpy in / numpy out - every call ends in a device synchronise. This is what a
          user gets, host round trips included, and what the legs are compared on.
  device  HIP events around back-to-back replays of the leg's captured graph alone (no host copies in between): what the GPU
          spends per image once the host is out of the way.
A run without a GPU fails; nothing here falls back.
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

BATCHES = (1, 4, 16, 32)


def build_detector(dtype):
    from multiposenet_amd.inference import Detector
    from multiposenet_amd.prn import initial_values as prn_values
    from multiposenet_amd.retinanet import initial_head_values
    head = initial_head_values(0)
    # a lively class head: every image fills its 25 slots, so the crops, the PRN and the gather run at full load
    head["class_net/logits/kernel"] = (np.random.RandomState(8).randn(3, 3, 64, 6) * 0.4).astype(np.float32)
    head["class_net/logits/bias"] = np.full(6, -2.0, np.float32)
    return Detector(None, dtype=dtype, detector_path=head, prn_path=prn_values(seed=0))


def device_ms_per_image(graph, images_per_replay, replays):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(replays):
        graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / (replays * images_per_replay)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--images", type=int, default=256, help="images per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "inference_batch.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inference_batch: no GPU (a measurement path does not fall back)")
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    s, thr, n = args.size, args.threshold, args.images
    pool = np.random.RandomState(0).randint(0, 256, (max(BATCHES), s, s, 3)).astype(np.uint8)

    def call_loop():
        persons = 0
        for i in range(n):
            persons += len(det(pool[i % len(pool)], score_threshold=thr)["boxes"])
        return persons

    def batch_leg(b, heat):
        def run():
            persons = 0
            for _ in range(max(1, n // b)):
                persons += sum(len(o["boxes"]) for o in det.predict_batch(pool[:b], score_threshold=thr, return_heatmaps=heat))
            return persons
        return run

    legs = [("call_loop", 1, call_loop)]
    for b in BATCHES:
        for heat in (True, False):
            legs.append((f"predict_batch_b{b}_{'heatmaps' if heat else 'no_heatmaps'}", b, batch_leg(b, heat)))
    persons = {}
    for name, b, fn in legs:                       # warm-up: every shape the timed window uses
        persons[name] = fn()
    wall = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, b, fn in legs:                   # alternate the legs inside a round
            images = n if b == 1 else max(1, n // b) * b
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) / images)
    graphs = {"call_loop": (det._graphs[(s, s)][0], 1)}
    for b in BATCHES:
        graphs[f"b{b}"] = (det._graphs[(b, s, s, thr)].graph, b)
    device = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, (g, b) in graphs.items():
            device[k].append(device_ms_per_image(g, b, max(4, n // b)))
    result = {"device": torch.cuda.get_device_name(0), "size": [s, s], "dtype": args.dtype, "score_threshold": thr,
              "images_per_leg_round": n, "rounds": args.rounds, "persons_per_image": persons["call_loop"] / n, "legs": {}}
    for name, b, _ in legs:
        w = sorted(wall[name])
        dev = device["call_loop" if b == 1 and name == "call_loop" else f"b{b}"]
        result["legs"][name] = {"batch": b, "wall_ms_per_image": {"median": statistics.median(w) * 1e3, "min": w[0] * 1e3, "max": w[-1] * 1e3},
                                "wall_images_per_s": 1.0 / statistics.median(w),
                                "device_ms_per_image": {"median": statistics.median(dev), "min": min(dev), "max": max(dev)}}
    base = result["legs"]["call_loop"]["wall_images_per_s"]
    for name in result["legs"]:
        result["legs"][name]["wall_speedup_over_call_loop"] = result["legs"][name]["wall_images_per_s"] / base
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
