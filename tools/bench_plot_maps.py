"""Heatmap and mask overlays: `Detector.predict_batch(plot_maps=True)` (made on the device, inside the captured graph) against
what it replaces - `predict_batch(return_heatmaps=True)` followed by the notebook-equivalent Pillow work on the host - same
process, same GPU, and the device time of the launches against a device-to-device copy of the bytes they write.

    timeout -k 10 600 python tools/bench_plot_maps.py [--batch 16] [--size 640] [--batches 4] [--rounds 5] [--replays 50]
                                                      [--out profiles/plot_maps.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Setup as tools/bench_inference_batch.py: bf16, the lively head. Legs, numpy in / numpy out, wall clock:
  A  predict_batch_then_host_maps   return_heatmaps=True, then per frame the normalisation, the colormap lookup, 19 Pillow
                                    Lanczos resizes, 18 alpha_composite, paste and text. Not measured when Pillow is absent.
  B  predict_batch_plot_maps        plot_maps=True, return_heatmaps=False.
Both are warmed up, then ALTERNATE over `--rounds` rounds of `--batches` batches; the figure of a leg is its median round.
Device time (HIP events, warm, `--replays` launches back to back): mpn_heatmap_minmax + mpn_plot_maps on the graph's own
buffers, and a plain device copy of as many bytes as the output has. A run without a GPU fails; nothing here falls back.
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

from multiposenet_amd.inference import maps  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402
from tools.bench_predict_images import events_ms  # noqa: E402


def host_plotter():
    """(name, plot(frame, heatmaps, mask) -> uint8 [18h, w, 4]) with Pillow, or (None, None)."""
    try:
        import PIL
        from PIL import Image, ImageDraw
    except ImportError:
        return None, None
    table = maps.colour_table()

    def plot(frame, heat, mask):
        h, w = frame.shape[0] // 2, frame.shape[1] // 2
        lo, hi = heat.min(0).min(0), heat.max(0).max(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (heat - lo) / (hi - lo) * np.float32(256)
        rgba = table[np.clip(np.nan_to_num(t), 0, 255).astype(np.int64)]
        rgba[np.isnan(t)] = 0
        out = Image.new("RGBA", (w, 18 * h), (255, 255, 255, 255))
        d = ImageDraw.Draw(out, "RGBA")
        base = Image.fromarray(frame).resize((w, h), Image.LANCZOS)
        base.putalpha(255)
        for j in range(18):
            if j < 17:
                over = Image.fromarray(np.ascontiguousarray(rgba[:, :, j])).resize((w, h), Image.LANCZOS)
            else:
                band = Image.fromarray((255 * np.clip(mask, 0.0, 1.0)).astype(np.uint8)).resize((w, h), Image.LANCZOS)
                over = Image.merge("RGBA", (band, band, band, band))
            out.paste(Image.alpha_composite(base, over), (0, j * h))
            d.text((0, j * h), maps.LABELS[j], fill="red")
        return np.asarray(out)

    return f"Pillow {PIL.__version__} (one thread)", plot


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=4, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "plot_maps.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plot_maps: no GPU (a measurement path does not fall back)")
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    images = np.random.RandomState(0).randint(0, 256, (b, s, s, 3)).astype(np.uint8)
    plotter_name, host_plot = host_plotter()

    def leg_a():
        persons = det.predict_batch(images, score_threshold=thr, return_heatmaps=True)
        for im, p in zip(images, persons):
            p["maps"] = host_plot(im, p["keypoint_heatmaps"], p["segmentation_masks"])
        return persons

    def leg_b():
        return det.predict_batch(images, score_threshold=thr, return_heatmaps=False, plot_maps=True)

    legs = [("predict_batch_plot_maps", leg_b)] + ([("predict_batch_then_host_maps", leg_a)] if host_plot else [])
    first = {name: fn() for name, fn in legs}                       # warm-up: graphs, buffers, pinned staging
    equal = None
    if host_plot:
        equal = all(np.array_equal(x["maps"], y["maps"]) for x, y in
                    zip(first["predict_batch_plot_maps"], first["predict_batch_then_host_maps"]))
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))

    ent = next(v for k, v in det._graphs.items() if isinstance(k, tuple) and k[-1] == "maps")
    plotter, heat, seg = ent.maps, ent.outs["heat"], ent.outs["seg"]
    launch_ms = [events_ms(lambda: plotter.launch(ent.x, heat, seg, normalise=True), args.replays) for _ in range(args.rounds)]
    graph_ms = [events_ms(ent.graph.replay, 20) for _ in range(args.rounds)]
    plain = next(v for k, v in det._graphs.items() if isinstance(k, tuple) and k[0] == b and k[-1] != "maps").graph
    plain_graph_ms = [events_ms(plain.replay, 20) for _ in range(args.rounds)]
    other = torch.empty_like(plotter.out)
    copy_ms = [events_ms(lambda: other.copy_(plotter.out), args.replays) for _ in range(args.rounds)]
    nb = plotter.out.numel()
    med = statistics.median
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "size": [s, s], "score_threshold": thr,
              "batches_per_leg_round": args.batches, "rounds": args.rounds, "replays": args.replays,
              "host_maps": plotter_name or "not measured: Pillow is not importable",
              "device_maps_equal_host_maps": equal,
              "plot_maps_launches": {"device_ms_per_batch": stats(launch_ms), "output_bytes_per_batch": int(nb),
                                     "output_GB_per_s": nb / (med(launch_ms) * 1e-3) / 1e9,
                                     "device_copy_of_the_output_ms_per_batch": stats(copy_ms),
                                     "times_the_copy": med(launch_ms) / med(copy_ms)},
              "graph_device_ms_per_batch": {"plot_maps": stats(graph_ms), "plain": stats(plain_graph_ms)},
              "legs": {}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": {"median": med(w) * 1e3, "min": w[0] * 1e3, "max": w[-1] * 1e3},
                                "wall_images_per_s": 1.0 / med(w)}
    if host_plot:
        result["plot_maps_speedup_over_host_maps"] = (result["legs"]["predict_batch_plot_maps"]["wall_images_per_s"]
                                                      / result["legs"]["predict_batch_then_host_maps"]["wall_images_per_s"])
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
