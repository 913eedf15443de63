"""Test-time augmentation of the joint inference graph: what `flip=True` and `scales=` cost against the plain graph - same
process, same GPU, same run - and the device time of the two launches the feature adds against a device copy of their bytes.

    timeout -k 10 600 python tools/bench_tta.py [--batch 16] [--size 640] [--scales 512 512 768 768] [--batches 4]
                                                [--rounds 5] [--replays 50] [--out profiles/tta.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Setup as tools/bench_inference_batch.py: bf16, the lively head (every image fills its 25 slots). Four configurations of
`predict_batch(return_heatmaps=False)`: plain, flip, scales, flip + scales. Per configuration: the device time of its captured
graph (HIP events around back-to-back replays) and wall-clock images/s, numpy in / dicts out. The configurations are warmed
up, then ALTERNATE over `--rounds` rounds of `--batches` batches; the figure of a configuration is its median round.
mpn_tta_merge and mpn_mirror_images are also timed alone on the buffers of the flip + scales entry, against a device copy of the
bytes they read and write. No ratio is fixed in advance; no accuracy is measured (the weights are seeded random ones).
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

from multiposenet_amd.inference import tta  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402
from tools.bench_predict_images import events_ms  # noqa: E402


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--scales", type=int, nargs="+", default=[512, 512, 768, 768], metavar="N", help="W H [W H ...]")
    ap.add_argument("--batches", type=int, default=4, help="batches per configuration and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "tta.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta: no GPU (a measurement path does not fall back)")
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    scales = [(args.scales[i], args.scales[i + 1]) for i in range(0, len(args.scales), 2)]
    images = np.random.RandomState(0).randint(0, 256, (b, s, s, 3)).astype(np.uint8)
    configs = [("plain", {}), ("flip", {"flip": True}), ("scales", {"scales": scales}),
               ("flip_and_scales", {"flip": True, "scales": scales})]

    def run(kw):
        return det.predict_batch(images, score_threshold=thr, return_heatmaps=False, **kw)

    entries = {}
    for name, kw in configs:                                        # warm-up: buffers, graphs, pinned staging
        before = set(det._graphs)
        run(kw)
        (key,) = set(det._graphs) - before
        entries[name] = det._graphs[key]
        run(kw)
    wall = {name: [] for name, _ in configs}
    for _ in range(args.rounds):
        for name, kw in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                run(kw)
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    graph_ms = {name: [events_ms(entries[name].graph.replay, 20) for _ in range(args.rounds)] for name, _ in configs}

    # the two new launches alone, on the buffers of the largest entry
    aug = entries["flip_and_scales"].tta
    x = aug.x
    sources = []
    for xk in [x] + [sc[0] for sc in aug.scales]:
        hk, wk = xk.shape[1] // 4, xk.shape[2] // 4
        heat = torch.rand((2 * b, hk, wk, 17), device=x.device)
        seg = torch.rand((2 * b, hk, wk), device=x.device)
        sources += [(heat[:b], seg[:b], False), (heat[b:], seg[b:], True)]
    merge_ms = [events_ms(lambda: tta.merge(sources, aug.heat, aug.seg), args.replays) for _ in range(args.rounds)]
    merge_bytes = sum(h.numel() + g.numel() for h, g, _ in sources) * 4 + (aug.heat.numel() + aug.seg.numel()) * 4
    flat = torch.empty(merge_bytes // 2, dtype=torch.uint8, device=x.device)        # a copy reads and writes: half the bytes each
    flat2 = torch.empty_like(flat)
    merge_copy_ms = [events_ms(lambda: flat2.copy_(flat), args.replays) for _ in range(args.rounds)]
    mirror_ms = [events_ms(lambda: tta.mirror_images(x[:b], x[b:]), args.replays) for _ in range(args.rounds)]
    other = torch.empty_like(x[b:])
    mirror_copy_ms = [events_ms(lambda: other.copy_(x[:b]), args.replays) for _ in range(args.rounds)]

    med = statistics.median
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "size": [s, s],
              "scales": [list(v) for v in scales], "score_threshold": thr, "batches_per_config_round": args.batches,
              "rounds": args.rounds, "replays": args.replays, "configs": {},
              "mpn_tta_merge": {"sources": len(sources), "device_ms_per_batch": stats(merge_ms),
                                "bytes_read_and_written": int(merge_bytes),
                                "GB_per_s": merge_bytes / (med(merge_ms) * 1e-3) / 1e9,
                                "device_copy_moving_the_same_bytes_ms": stats(merge_copy_ms),
                                "times_the_copy": med(merge_ms) / med(merge_copy_ms)},
              "mpn_mirror_images": {"device_ms_per_batch": stats(mirror_ms), "bytes_read_and_written": int(2 * x[:b].numel()),
                                    "GB_per_s": 2 * x[:b].numel() / (med(mirror_ms) * 1e-3) / 1e9,
                                    "device_copy_of_the_same_bytes_ms": stats(mirror_copy_ms),
                                    "times_the_copy": med(mirror_ms) / med(mirror_copy_ms)}}
    plain_graph, plain_wall = med(graph_ms["plain"]), med(wall["plain"])
    for name, _ in configs:
        w = sorted(wall[name])
        result["configs"][name] = {"graph_device_ms_per_batch": stats(graph_ms[name]),
                                   "graph_device_time_over_plain": med(graph_ms[name]) / plain_graph,
                                   "wall_ms_per_image": {"median": med(w) * 1e3, "min": w[0] * 1e3, "max": w[-1] * 1e3},
                                   "wall_images_per_s": 1.0 / med(w), "wall_time_over_plain": med(w) / plain_wall}
    result["flip_costs_less_than_a_second_plain_call"] = bool(med(graph_ms["flip"]) < 2 * plain_graph)
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
