"""What persistent person identities cost: `Detector.predict_images(..., track=)` - mpn_pose_track inside the captured graph,
the state advanced by one small device copy behind it - against the same call without `track=` in the same process, and
against that call followed by the plain-loop numpy tracker on the host (tests/track_ref.py: what tracking cost before the
kernel existed).

    timeout -k 10 400 python tools/bench_pose_track.py [--batch 16] [--streams 1] [--source 720 1280] [--size 640] [--batches 8]
                                                       [--rounds 5] [--similarity oks] [--out profiles/pose_track.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Legs, numpy in / numpy out, wall clock (time.perf_counter around calls that end in a device synchronise), all warmed up, then
ALTERNATING over `--rounds` rounds of `--batches` batches; the figure of a leg is its median round:
  A  predict_images                 no tracking
  B  predict_images_track           predict_images(track=): the ids come back with the record
  C  predict_images_host_tracker    predict_images, then track_ref.run on the returned dicts
Device time from HIP events around back-to-back work: replays of A's and B's whole graphs, and the mpn_pose_track launch plus
the commit copy alone on B's buffers - with --streams 1 the block walks the batch's frames one after the other, the longest
launch a batch can ask for; the same launch with one stream per image is reported next to it. The frames are unrelated random
images (as in bench_predict_images.py): few persons of a frame are found again in the next, the 32 slots fill within the first
frames and most later persons find none - the similarity matrix and the births run at full load, the greedy rounds do not.
A run without a GPU fails."""
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

import track_ref as ref  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--source", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=8, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--similarity", default="oks", choices=["oks", "iou"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "pose_track.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_track: no GPU (a measurement path does not fall back)")
    from multiposenet_amd.inference import PoseTracker
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw          # structure at the network's scale (bench_predict_images.py)
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    max_boxes = det.params['max_boxes']
    tracker = PoseTracker(streams=args.streams, similarity=args.similarity, max_boxes=max_boxes)
    p = ref.Params(tracker.max_tracks, args.similarity, tracker.match_threshold, tracker.max_misses, tracker.new_track_score)
    host_state = ref.new_state(args.streams, tracker.max_tracks)
    host_ms = []

    def leg_a():
        return sum(len(o['scores']) for _ in range(args.batches) for o in det.predict_images(frames, size=(s, s), score_threshold=thr))

    def leg_b():
        tracked = 0
        for _ in range(args.batches):
            for o in det.predict_images(frames, size=(s, s), score_threshold=thr, track=tracker):
                tracked += int((o['track_ids'] > 0).sum())
        return tracked

    def leg_c():
        tracked = 0
        for _ in range(args.batches):
            outs = det.predict_images(frames, size=(s, s), score_threshold=thr)
            t0 = time.perf_counter()
            rows = ref.run(outs, host_state, p)
            host_ms.append((time.perf_counter() - t0) * 1e3 / b)
            tracked += sum(int((r['track_ids'] > 0).sum()) for r in rows)
        return tracked

    legs = [("predict_images", leg_a), ("predict_images_track", leg_b), ("predict_images_host_tracker", leg_c)]
    counts = {name: fn() for name, fn in legs}                         # warm-up: every shape the timed window uses
    del host_ms[:]
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    ent = next(e for k, e in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and "track" in k)
    plain = next(e for k, e in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and "track" not in k)
    whole = ent.outs['record']
    nbytes = whole.numel() - tracker.out_bytes(b)

    def track_and_commit(t):
        t.launch(whole[:nbytes], whole[nbytes:], b)
        t.commit()
    per_image = PoseTracker(streams=b, similarity=args.similarity, max_boxes=max_boxes)
    for t in (tracker, per_image):                                     # (both warm: state filled, code object loaded)
        track_and_commit(t)
    graph_ms = [events_ms(ent.graph.replay, 20) for _ in range(args.rounds)]
    plain_ms = [events_ms(plain.graph.replay, 20) for _ in range(args.rounds)]
    track_ms = [events_ms(lambda: track_and_commit(tracker), 20) for _ in range(args.rounds)]
    track_per_image_ms = [events_ms(lambda: track_and_commit(per_image), 20) for _ in range(args.rounds)]

    def spread(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "streams": args.streams,
              "source": [sh, sw], "size": [s, s], "score_threshold": thr, "similarity": args.similarity,
              "max_tracks": tracker.max_tracks, "batches_per_leg_round": args.batches, "rounds": args.rounds,
              "persons_per_image": counts["predict_images"] / (args.batches * b),
              "tracked_per_image": counts["predict_images_track"] / (args.batches * b),
              "tracked_per_image_host_tracker": counts["predict_images_host_tracker"] / (args.batches * b),
              "host_tracker": "tests/track_ref.py run (plain-loop numpy, one thread)",
              "host_tracker_ms_per_image": spread(host_ms),
              "track_rows_d2h_bytes_per_batch": int(tracker.out_bytes(b)), "state_bytes": int(tracker.state_bytes),
              "legs": {},
              "device_ms_per_batch": {"graph_with_track": spread(graph_ms), "graph_without": spread(plain_ms),
                                      "track_launch_and_commit": spread(track_ms),
                                      "track_launch_and_commit_one_stream_per_image": spread(track_per_image_ms)}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": spread([x * 1e3 for x in w]), "wall_images_per_s": 1.0 / statistics.median(w)}
    rate = {name: result["legs"][name]["wall_images_per_s"] for name, _ in legs}
    result["track_rate_over_plain"] = rate["predict_images_track"] / rate["predict_images"]
    result["track_rate_over_host_tracker"] = rate["predict_images_track"] / rate["predict_images_host_tracker"]
    result["track_share_of_graph_device_time"] = statistics.median(track_ms) / statistics.median(graph_ms)
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
