"""What density maps cost: `Detector.predict_images(annotate='jpeg', track=, density=)` - mpn_density_map behind the tracker's
launches and mpn_draw_density behind the drawing inside the captured graph - against the same call without `density=` in the
same process (what the parent commit runs), and the launches alone.

    timeout -k 10 400 python tools/bench_density.py [--batch 16] [--source 720 1280] [--size 640] [--cell 16] [--rounds 5]
                                                    [--out profiles/density.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

The setting is that of tools/bench_trails.py: bf16, --batch frames of one stream, the lively head, ONE frame panned by 4 pixels
a frame; two warm-up calls fill the state. Measured, all warmed up, as device time (HIP events around 20 back-to-back repeats,
medians of --rounds rounds with their ranges), the legs ALTERNATING:
    the captured graph with track= (what the parent commit runs), and the same with density=;
    mpn_density_map alone over the graph's own record, for both footprints, with its snapshots;
    mpn_draw_density's two launches, smooth and not, over a hand-filled grid in which every cell counts, so that every pixel
    blends, against a device copy of the same frames (one read and one write per pixel, as the raster does).
mpn_draw_density is in place, so the launches alone blend over their own output: the bytes differ from launch to launch, the
work does not. No figure is fixed in advance. A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "density.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_density: no GPU (a measurement path does not fall back)")
    from multiposenet_amd.density import IMAGE, ROW
    from multiposenet_amd.inference import DensityMap, PoseTracker
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    pan = 4
    rng = np.random.RandomState(0)
    wide = sw + pan * (b - 1)
    yy, xx = np.arange(sh) * s // sh, np.arange(wide) * s // sw        # structure at the network's scale (bench_predict_images.py)
    base = rng.randint(0, 256, (s, int(xx.max()) + 1, 3)).astype(np.uint8)[yy][:, xx]
    frames = [np.ascontiguousarray(base[:, pan * i:pan * i + sw]) for i in range(b)]
    max_boxes = det.params['max_boxes']
    kw = dict(streams=1, similarity='oks', max_boxes=max_boxes)
    with_density, without = PoseTracker(**kw), PoseTracker(**kw)
    make = lambda **more: DensityMap(streams=1, frame_size=(sh, sw), cell=args.cell, max_boxes=max_boxes, **more)   # noqa: E731
    density, boxes, blocky = make(), make(footprint='box'), make(smooth=False)
    common = dict(size=(s, s), score_threshold=thr, annotate='jpeg')
    for _ in range(2):                                              # warm-up: graphs captured, states filled
        outs = det.predict_images(frames, track=with_density, density=density, **common)
        det.predict_images(frames, track=without, **common)
    ents = {"with": next(e for e in det._graphs.values() if getattr(e, 'density', None) is density),
            "without": next(e for e in det._graphs.values() if getattr(e, 'track', None) is without)}
    ent = ents["with"]
    whole = ent.outs['record']
    layout = ent.layout                                             # the entry's own: where each stage's rows lie
    record, rows, density_rows = whole[layout.record], whole[layout.track], whole[layout.density]
    track_rows = rows[:with_density.track_bytes(b)]
    frames_rgba = ent.draw.out
    copy_of_frames = torch.empty_like(frames_rgba)

    # a hand-filled grid: every cell counts, so that every level is >= 1 and every pixel blends
    G = density.gh * density.gw
    grid = rng.randint(40, 1000, (b, G)).astype(np.uint32)
    hand_snapshots = torch.from_numpy(grid.view(np.uint8).reshape(-1)).to(whole.device)
    hand = np.zeros(b * max_boxes * ROW.itemsize + b * IMAGE.itemsize, np.uint8)
    hand[b * max_boxes * ROW.itemsize:].view(IMAGE)['max_dwell'] = grid.max(axis=1)
    hand_rows = torch.from_numpy(hand).to(whole.device)
    box_rows = torch.empty_like(density_rows)

    timed = {
        "graph_with_density": ents["with"].graph.replay,
        "graph_without": ents["without"].graph.replay,
        "density_map_anchor": lambda: density.launch(record, track_rows, density_rows, b, True, density.snapshots(b)),
        "density_map_box": lambda: boxes.launch(record, track_rows, box_rows, b, True, boxes.snapshots(b)),
        "draw_density_smooth": lambda: density.launch_draw(ent.draw.desc, hand_snapshots, hand_rows, frames_rgba, b),
        "draw_density_cells": lambda: blocky.launch_draw(ent.draw.desc, hand_snapshots, hand_rows, frames_rgba, b),
        "copy_of_the_frames": lambda: copy_of_frames.copy_(frames_rgba),
    }
    for fn in timed.values():
        fn()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    moved = 2 * b * sh * sw * 4
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "streams": 1, "source": [sh, sw],
              "size": [s, s], "score_threshold": thr, "cell": args.cell, "grid": [density.gh, density.gw],
              "pan_pixels_per_frame": pan, "rounds": args.rounds, "repeats_per_round": 20,
              "persons_per_image": sum(len(o['scores']) for o in outs) / b,
              "counted_per_image_last_batch": sum(o['density']['counted'] for o in outs) / b,
              "density_rows_d2h_bytes_per_batch": int(density.out_bytes(b)), "state_bytes": int(density.state_bytes),
              "snapshot_bytes": int(density.snapshots(b).numel()),
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "graph_added_ms": med["graph_with_density"] - med["graph_without"],
              "graph_with_density_over_without": med["graph_with_density"] / med["graph_without"],
              "frame_bytes_read_and_written": moved,
              "gb_per_s": {name: moved / med[name] / 1e6 for name in ("draw_density_smooth", "draw_density_cells", "copy_of_the_frames")},
              "draw_density_smooth_rate_over_copy": med["copy_of_the_frames"] / med["draw_density_smooth"],
              "draw_density_cells_rate_over_copy": med["copy_of_the_frames"] / med["draw_density_cells"]}
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
