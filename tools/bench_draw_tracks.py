"""What drawing identities costs: the two launches of `mpn_draw_tracks` against the two of `mpn_draw_detections` on the SAME
record and frames, and the captured graph of `Detector.predict_images(annotate='jpeg', track=...)` with and without
`track_style=`.

    timeout -k 10 400 python tools/bench_draw_tracks.py [--batch 16] [--source 720 1280] [--size 640] [--rounds 5]
                                                        [--out profiles/draw_tracks.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Device time from HIP events around 20 back-to-back repeats, all warmed up, ALTERNATING over `--rounds` rounds; the figure of a
leg is its median round, and the spread of the plain legs is the noise a difference has to exceed. One stream per image and
new_track_score 0, so EVERY person of the record is tracked: every box and dot takes its ink from the table and every person
has a label - the most the new launches can be asked to draw for this record. The yardstick is mpn_draw_detections in the same
run; no ratio is fixed in advance. A run without a GPU fails."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "draw_tracks.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_draw_tracks: no GPU (a measurement path does not fall back)")
    from multiposenet_amd.inference import PoseTracker, TrackStyle
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw          # structure at the network's scale (bench_predict_images.py)
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    kw = dict(streams=b, similarity='iou', new_track_score=0.0, max_boxes=det.params['max_boxes'])
    style = TrackStyle()
    legs = {"plain": (PoseTracker(**kw), None), "styled": (PoseTracker(**kw), style)}
    persons = tracked = 0
    for name, (t, st) in legs.items():                                  # warm-up: graphs captured, tracks born and matched
        for _ in range(3):
            outs = det.predict_images(frames, size=(s, s), score_threshold=thr, annotate='jpeg', track=t, track_style=st)
        persons = sum(len(o['track_ids']) for o in outs) / b
        tracked = sum(int((o['track_ids'] > 0).sum()) for o in outs) / b
    ents = {name: next(e for e in det._graphs.values() if getattr(e, 'track', None) is t) for name, (t, _) in legs.items()}
    ent, t = ents["styled"], legs["styled"][0]
    whole = ent.outs['record']
    nbytes = whole.numel() - t.out_bytes(b)
    record, rows = whole[:nbytes], whole[nbytes:nbytes + t.track_bytes(b)]
    timed = {"graph_annotate_jpeg_track": ents["plain"].graph.replay,
             "graph_annotate_jpeg_track_style": ents["styled"].graph.replay,
             "draw_detections_two_launches": lambda: ent.draw.launch(ent.sources, record, True),
             "draw_tracks_two_launches": lambda: ent.draw.launch_tracks(ent.sources, record, rows, None, ent.style[1], True)}
    for fn in timed.values():
        fn()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    plain_spread = (max(ms["draw_detections_two_launches"]) - min(ms["draw_detections_two_launches"])) / med["draw_detections_two_launches"]
    pixels = b * sh * sw
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": [sh, sw], "size": [s, s],
              "score_threshold": thr, "rounds": args.rounds, "repeats_per_round": 20, "style": repr(style),
              "persons_per_image": persons, "tracked_per_image": tracked,
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "draw_tracks_over_draw_detections": med["draw_tracks_two_launches"] / med["draw_detections_two_launches"],
              "draw_detections_spread_over_median": plain_spread,
              "draw_tracks_added_ms": med["draw_tracks_two_launches"] - med["draw_detections_two_launches"],
              "graph_with_style_over_without": med["graph_annotate_jpeg_track_style"] / med["graph_annotate_jpeg_track"],
              "graph_added_ms": med["graph_annotate_jpeg_track_style"] - med["graph_annotate_jpeg_track"],
              # the raster pass reads 3 and writes 4 bytes per pixel; the primitives are noise next to it
              "draw_tracks_bytes_per_s": pixels * 7 / (med["draw_tracks_two_launches"] * 1e-3),
              "draw_detections_bytes_per_s": pixels * 7 / (med["draw_detections_two_launches"] * 1e-3)}
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
