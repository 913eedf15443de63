"""What motion trails cost: `Detector.predict_images(annotate='jpeg', track=, track_style=, trails=)` - mpn_track_trails behind
the tracker's launches and mpn_draw_trails behind the drawing inside the captured graph - against the same call without
`trails=` in the same process (what the parent commit runs), and the launches alone against mpn_draw_tracks' two launches.

    timeout -k 10 400 python tools/bench_trails.py [--batch 16] [--source 720 1280] [--size 640] [--length 32] [--rounds 5]
                                                   [--out profiles/trails.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

The setting is that of tools/bench_zones.py: bf16, --batch frames of one stream, the lively head. The frames are ONE frame
panned by 4 pixels a frame, so that the persons move and the trails grow where the tracker follows them; two warm-up calls fill
the state. Measured, all warmed up, as device time (HIP events around 20 back-to-back repeats, medians of --rounds rounds with
their ranges), the legs ALTERNATING:
    the captured graph with track= and track_style= (what the parent commit runs), and the same with trails=;
    mpn_track_trails alone, and mpn_draw_trails' two launches alone over the graph's own rows, against mpn_draw_tracks' two
    launches on the same record and frames;
    mpn_draw_trails' two launches over handwritten rows: every slot of every image a trail with a full ring at K = 64.
mpn_draw_trails is in place, so the launches alone blend over their own output: the bytes differ from launch to launch, the
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
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "trails.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trails: no GPU (a measurement path does not fall back)")
    from multiposenet_amd import _lib
    from multiposenet_amd.inference import PoseTracker, TrackStyle, TrackTrails
    from multiposenet_amd.trails import row_dtype
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
    with_trails, without = PoseTracker(**kw), PoseTracker(**kw)
    style = TrackStyle()
    trails = TrackTrails(streams=1, frame_size=(sh, sw), length=args.length, max_boxes=max_boxes)
    common = dict(size=(s, s), score_threshold=thr, annotate='jpeg', track_style=style)
    for _ in range(2):                                              # warm-up: graphs captured, states filled
        outs = det.predict_images(frames, track=with_trails, trails=trails, **common)
        det.predict_images(frames, track=without, **common)
    tracked = [int(o['trails']['tracked'].sum()) for o in outs]
    counts = np.concatenate([o['trails']['count'][o['trails']['tracked']] for o in outs])
    ents = {"with": next(e for e in det._graphs.values() if getattr(e, 'trails', None) is trails),
            "without": next(e for e in det._graphs.values() if getattr(e, 'track', None) is without)}
    ent = ents["with"]
    whole = ent.outs['record']
    layout = ent.layout                                             # the entry's own: where each stage's rows lie
    record, rows, trail_rows = whole[layout.record], whole[layout.track], whole[layout.trails]
    track_rows = rows[:with_trails.track_bytes(b)]
    table = ent.style[1]
    frames_rgba = ent.draw.out

    # handwritten rows: every slot of every image a tracked trail of K + 1 = 65 points, a random walk of 6 pixel steps
    K = 64
    full = TrackTrails(streams=1, frame_size=(sh, sw), length=K, max_boxes=max_boxes)
    hand = np.zeros(b * max_boxes, row_dtype(K))
    hand['n'], hand['flags'] = K + 1, 1
    start = rng.uniform(0.2, 0.8, (b * max_boxes, 1, 2)) * (sw, sh)
    hand['points'] = (start + np.cumsum(rng.uniform(-6, 6, (b * max_boxes, K + 1, 2)), axis=1)).astype(np.float32)
    hand_rows = torch.from_numpy(hand.view(np.uint8)).to(whole.device)
    full_record = whole[layout.record].clone()
    header = np.zeros(1 + b, np.int32)
    header[0], header[1:] = b * max_boxes, max_boxes
    full_record[:header.nbytes].copy_(torch.from_numpy(header.view(np.uint8)))
    ids = np.zeros((b * max_boxes, 6), np.int32)
    ids[:, 0] = 1 + np.arange(b * max_boxes)
    full_ids = torch.from_numpy(ids.view(np.uint8).reshape(-1)).to(whole.device)

    timed = {
        "graph_with_trails": ents["with"].graph.replay,
        "graph_without": ents["without"].graph.replay,
        "track_trails_launch": lambda: trails.launch(record, track_rows, trail_rows, b),
        "draw_trails_two_launches": lambda: trails.launch_draw(ent.draw.desc, record, track_rows, trail_rows, frames_rgba, b),
        "draw_tracks_two_launches": lambda: ent.draw.launch_tracks(ent.sources, record, track_rows, None, table, True),
        "draw_trails_full_rings_k64": lambda: full.launch_draw(ent.draw.desc, full_record, full_ids, hand_rows, frames_rgba, b),
    }
    for fn in timed.values():
        fn()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "streams": 1, "source": [sh, sw],
              "size": [s, s], "score_threshold": thr, "length": args.length, "pan_pixels_per_frame": pan, "rounds": args.rounds,
              "repeats_per_round": 20, "persons_per_image": sum(len(o['scores']) for o in outs) / b,
              "tracked_persons_per_image_last_batch": sum(tracked) / b,
              "trail_points_last_batch": {"mean": float(counts.mean()) if len(counts) else 0.0,
                                          "max": int(counts.max()) if len(counts) else 0},
              "trail_rows_d2h_bytes_per_batch": int(trails.out_bytes(b)), "state_bytes": int(trails.state_bytes),
              "draw_workspace_bytes": int(_lib.lib().mpn_draw_trails_workspace_bytes(b, max_boxes, args.length)),
              "full_rings": {"length": K, "trails": b * max_boxes, "segments_per_trail": K},
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "graph_added_ms": med["graph_with_trails"] - med["graph_without"],
              "graph_with_trails_over_without": med["graph_with_trails"] / med["graph_without"],
              "draw_trails_over_draw_tracks": med["draw_trails_two_launches"] / med["draw_tracks_two_launches"],
              "draw_trails_full_rings_over_draw_tracks": med["draw_trails_full_rings_k64"] / med["draw_tracks_two_launches"]}
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
