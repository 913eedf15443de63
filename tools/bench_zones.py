"""What counting persons in zones and across lines costs: `Detector.predict_images(..., track=, zones=)` - mpn_zone_events behind
the tracker's launches inside the captured graph, its state advanced by one small device copy - against the same call without
`zones=` in the same process, and against that call followed by the plain-loop numpy definition on the host
(tests/zones_ref.py: what the counting costs without the kernel).

    timeout -k 10 400 python tools/bench_zones.py [--batch 16] [--source 720 1280] [--size 640] [--batches 4] [--rounds 5]
                                                  [--out profiles/zones.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

The record is that of tools/bench_pose_track.py: --batch unrelated random frames of one stream, the lively head's 25 persons per
image. The geometry is the largest a counter takes: 16 zones of 16 vertices and 16 lines, spread over the frame, so that every
person is tested against 256 edges and every known one against 16 lines. Measured, all warmed up:
  device time (HIP events around 20 back-to-back repeats, medians of --rounds rounds with their ranges), ALTERNATING:
    the captured graph with track= (what the parent commit runs), and the same with zones=;
    the mpn_zone_events launch plus its commit alone, and the tracker's launch plus its commit alone, on that record;
  wall clock, numpy in / numpy out, ALTERNATING over --rounds rounds of --batches batches:
    predict_images(track=, zones=), and predict_images(track=) followed by zones_ref.run on the returned dicts.
No figure is fixed in advance. A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zones_ref as ref  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def geometry(sh, sw):
    """16 polygons of 16 vertices on a 4 x 4 grid over the frame and 16 lines, 8 upright and 8 level, in quarter pixels."""
    zones, lines = {}, {}
    for i in range(16):
        cx, cy, r = sw * (2 * (i % 4) + 1) / 8.0, sh * (2 * (i // 4) + 1) / 8.0, min(sh, sw) / 6.0
        a = 2 * np.pi * np.arange(16) / 16
        zones[f"zone{i}"] = [(float(np.round((cx + r * np.cos(t)) * 4) / 4), float(np.round((cy + r * np.sin(t)) * 4) / 4)) for t in a]
        k = i // 2 + 1
        lines[f"line{i}"] = ((sw * k / 9.0, 0.0), (sw * k / 9.0 + 8.0, float(sh))) if i % 2 == 0 else ((0.0, sh * k / 9.0), (float(sw), sh * k / 9.0 + 8.0))
    return zones, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=4, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "zones.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_zones: no GPU (a measurement path does not fall back)")
    from multiposenet_amd.inference import PoseTracker, ZoneCounter
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw          # structure at the network's scale (bench_predict_images.py)
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    max_boxes = det.params['max_boxes']
    zones, lines = geometry(sh, sw)
    kw = dict(streams=1, similarity='oks', max_boxes=max_boxes)
    with_zones, without = PoseTracker(**kw), PoseTracker(**kw)
    counter = ZoneCounter(streams=1, frame_size=(sh, sw), zones=zones, lines=lines, max_boxes=max_boxes)
    host_geo = ref.Geometry((sh, sw), list(zones.values()), list(lines.values()))
    host_state = ref.new_state(1)
    host_ms = []

    def leg_device():
        outs = det.predict_images(frames, size=(s, s), score_threshold=thr, track=with_zones, zones=counter)
        return int(sum(o['zones']['occupancy'].sum() for o in outs))

    def leg_host():
        outs = det.predict_images(frames, size=(s, s), score_threshold=thr, track=without)
        t0 = time.perf_counter()
        _, images = ref.run(host_geo, outs, host_state, max_boxes)
        host_ms.append((time.perf_counter() - t0) * 1e3 / b)
        return int(images['occupancy'].sum())

    legs = [("predict_images_zones", leg_device), ("predict_images_host_counting", leg_host)]
    occupancy = {name: [fn() for _ in range(2)][-1] for name, fn in legs}   # warm-up: graphs captured, states filled
    persons = sum(len(o['scores']) for o in det.predict_images(frames, size=(s, s), score_threshold=thr)) / b
    del host_ms[:]
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    ents = {"with": next(e for e in det._graphs.values() if getattr(e, 'zones', None) is counter),
            "without": next(e for e in det._graphs.values() if getattr(e, 'track', None) is without)}
    ent = ents["with"]
    whole = ent.outs['record']
    layout = ent.layout                                             # the entry's own: where each stage's rows lie
    record, track_rows, zone_rows = whole[layout.record], whole[layout.track], whole[layout.zones]

    def zones_and_commit():
        counter.launch(record, track_rows[:with_zones.track_bytes(b)], zone_rows, b)
        counter.commit()

    def track_and_commit():
        with_zones.launch(record, track_rows, b)
        with_zones.commit()
    timed = {"graph_with_zones": ents["with"].graph.replay, "graph_without": ents["without"].graph.replay,
             "zone_events_launch_and_commit": zones_and_commit, "track_launch_and_commit": track_and_commit,
             "zone_events_launch": lambda: counter.launch(record, track_rows[:with_zones.track_bytes(b)], zone_rows, b)}
    for fn in timed.values():
        fn()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "streams": 1, "source": [sh, sw],
              "size": [s, s], "score_threshold": thr, "zones": 16, "vertices_per_zone": 16, "lines": 16, "rounds": args.rounds,
              "batches_per_leg_round": args.batches, "persons_per_image": persons, "occupancy_sum_last_batch": occupancy,
              "host_counting": "tests/zones_ref.py run (plain-loop numpy, one thread)",
              "host_counting_ms_per_image": spread(host_ms), "zone_rows_d2h_bytes_per_batch": int(counter.out_bytes(b)),
              "state_bytes": int(counter.state_bytes), "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "graph_added_ms": med["graph_with_zones"] - med["graph_without"],
              "graph_with_zones_over_without": med["graph_with_zones"] / med["graph_without"],
              "zone_events_over_track_launch": med["zone_events_launch_and_commit"] / med["track_launch_and_commit"], "legs": {}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": spread([x * 1e3 for x in w]), "wall_images_per_s": 1.0 / statistics.median(w)}
    result["zones_rate_over_host_counting"] = (result["legs"]["predict_images_zones"]["wall_images_per_s"] /
                                               result["legs"]["predict_images_host_counting"]["wall_images_per_s"])
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
