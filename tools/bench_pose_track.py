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
A run without a GPU fails.

    timeout -k 10 300 python tools/bench_pose_track.py --smooth [the same options]

measures what `PoseTracker(smooth=OneEuro())` adds and writes it under the "smooth" key of --out, whose other keys stay (the
file is read first): device time, ALTERNATING in one run, of the captured graph with a smoothing tracker against the same graph
with a plain tracker, and of the mpn_pose_smooth launch plus its state's commit copy alone against the mpn_pose_track launch plus
its commit copy alone. The comparison is the plain-tracker graph of the same run; no ratio is fixed in advance.

    timeout -k 10 300 python tools/bench_pose_track.py --assignment optimal [the same options]

measures what `PoseTracker(assignment='optimal')` costs against the greedy tracker and writes it under the "optimal" key of
--out in the same way: device time, ALTERNATING in one run, of the captured graph and of the track launch plus commit alone,
for one stream and for one stream per image, each with a greedy and an optimal tracker on the same record; and of the launch
alone on two records made for it (tests/track_assign_cases.py: the chain of 64 boxes stepping half a box to and fro, and 64
random overlapping boxes, 64 slots, --batch frames of one stream, IoU) - the longest searches the reference counts. The
comparison is the greedy launch of the same run; no ratio is fixed in advance.

    timeout -k 10 300 python tools/bench_pose_track.py --motion [--assignment greedy|optimal] [the same options]

measures what `PoseTracker(motion=ConstantVelocity())` adds and writes it under the "motion" key of --out in the same way:
device time, ALTERNATING in one run and on the same record, of the captured graph with a motion tracker against the graph with
a plain tracker of the same assignment, and of the track launch plus the commit copies alone (mpn_pose_track_motion and two
state copies against the plain entry and one), for one stream and for one stream per image. The frames are one frame panned by
4 pixels a frame, so that tracks go on and carry velocities. The yardstick is the plain tracker of the same run; no ratio is
fixed in advance, and nothing is said about tracking quality."""
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


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def smooth_leg(args, det, frames):
    from multiposenet_amd.inference import OneEuro, PoseTracker
    b, s, thr = args.batch, args.size, args.threshold
    kw = dict(streams=args.streams, similarity=args.similarity, max_boxes=det.params['max_boxes'])
    # one camera's frames that follow each other (the first frame panned by 4 pixels a frame): the tracks go on from frame to
    # frame and their filters run, which the unrelated frames of the other legs would not make them do
    frames = [np.roll(frames[0], 4 * f, axis=1) for f in range(b)]
    trackers = {"plain": PoseTracker(**kw), "smooth": PoseTracker(smooth=OneEuro(), **kw)}
    tracked = {}
    for name, t in trackers.items():                                   # warm-up: graphs captured, states filled
        for _ in range(3):
            outs = det.predict_images(frames, size=(s, s), score_threshold=thr, track=t)
        tracked[name] = sum(int((o['track_ids'] > 0).sum()) for o in outs) / b
    filtered = sum(int(np.count_nonzero(o['keypoint_velocities'].any(axis=2))) for o in outs) / b
    ents = {name: next(e for e in det._graphs.values() if getattr(e, 'track', None) is t) for name, t in trackers.items()}
    t = trackers["smooth"]
    whole = ents["smooth"].outs['record']
    nbytes = whole.numel() - t.out_bytes(b)
    record, rows, out = whole[:nbytes], whole[nbytes:nbytes + t.track_bytes(b)], whole[nbytes + t.track_bytes(b):]

    def track_and_commit():
        t.launch(record, rows, b)
        t.prev.copy_(t.next, non_blocking=True)

    def smooth_and_commit():
        t.launch_smooth(record, rows, out, b)
        t.smooth_prev.copy_(t.smooth_next, non_blocking=True)
    # the same launch with EVERY person of the record tracked (handwritten track rows: person r of a frame in slot r, id r + 1):
    # all filters of a frame step in every frame, which the tracker's own rows do not make them do when few persons of a
    # frame are found again in the next
    from multiposenet_amd import tracking
    counts = whole[4:4 + 4 * b].cpu().numpy().view(np.int32)
    full_rows = np.zeros(b * t.max_boxes, tracking._OUT)
    full_rows['slot'] = -1
    at = 0
    for n in counts:
        m = min(int(n), t.max_tracks)
        full_rows['slot'][at:at + m] = np.arange(m)
        full_rows['track_id'][at:at + m] = np.arange(m) + 1
        at += int(n)
    full_rows_dev = torch.from_numpy(full_rows.view(np.uint8)).to(whole.device)
    full_out = torch.zeros_like(out)

    def smooth_full_and_commit():
        t.launch_smooth(record, full_rows_dev, full_out, b)
        t.smooth_prev.copy_(t.smooth_next, non_blocking=True)
    timed = {"graph_with_smoothing_tracker": ents["smooth"].graph.replay, "graph_with_plain_tracker": ents["plain"].graph.replay,
             "smooth_launch_and_commit": smooth_and_commit, "smooth_launch_and_commit_every_person_tracked": smooth_full_and_commit,
             "track_launch_and_commit": track_and_commit}
    for fn in timed.values():
        fn()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    velocities = full_out.cpu().numpy().view(tracking._SMOOTH_OUT)['velocities']
    t.reset()                                                          # (the handwritten rows left filters no track owns)
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "streams": args.streams,
              "source": list(args.source), "size": [s, s], "score_threshold": thr, "similarity": args.similarity,
              "max_tracks": t.max_tracks, "rounds": args.rounds, "one_euro": repr(t.smooth),
              "tracked_per_image": tracked, "filtered_joints_per_image": filtered,
              "filtered_joints_per_image_every_person_tracked": int(np.count_nonzero(velocities.any(axis=2))) / b,
              "smooth_rows_d2h_bytes_per_batch": int(t.out_bytes(b) - t.track_bytes(b)), "smooth_state_bytes": int(t.smooth_state_bytes),
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "graph_added_ms": med["graph_with_smoothing_tracker"] - med["graph_with_plain_tracker"],
              "graph_with_smoothing_over_plain": med["graph_with_smoothing_tracker"] / med["graph_with_plain_tracker"],
              "smooth_over_track_launch": med["smooth_launch_and_commit"] / med["track_launch_and_commit"],
              "smooth_every_person_tracked_over_track_launch":
                  med["smooth_launch_and_commit_every_person_tracked"] / med["track_launch_and_commit"]}
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged["smooth"] = result
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print(json.dumps({"smooth": result}))


def motion_leg(args, det, frames):
    from multiposenet_amd.inference import ConstantVelocity, PoseTracker
    b, s, thr = args.batch, args.size, args.threshold
    frames = [np.roll(frames[0], 4 * f, axis=1) for f in range(b)]     # (as in smooth_leg: one camera's consecutive frames)
    timed, tracked, coasting = {}, {}, {}
    for streams in (1, b):
        kw = dict(streams=streams, similarity=args.similarity, max_boxes=det.params['max_boxes'], assignment=args.assignment)
        trackers = {"plain": PoseTracker(**kw), "motion": PoseTracker(motion=ConstantVelocity(), **kw)}
        tag = "one_stream" if streams == 1 else "one_stream_per_image"
        for name, t in trackers.items():                               # warm-up: graphs captured, states filled
            for _ in range(3):
                outs = det.predict_images(frames, size=(s, s), score_threshold=thr, track=t)
            tracked[f"{name}_{tag}"] = sum(int((o['track_ids'] > 0).sum()) for o in outs) / b
            if name == "motion":
                coasting[tag] = sum(len(o['coasting_ids']) for o in outs) / b
            ent = next(e for e in det._graphs.values() if getattr(e, 'track', None) is t)
            whole = ent.outs['record']
            nbytes = whole.numel() - t.out_bytes(b)

            def track_and_commit(t=t, record=whole[:nbytes], rows=whole[nbytes:]):
                t.launch(record, rows, b)
                t.commit()
            timed[f"graph_{name}_{tag}"] = ent.graph.replay
            timed[f"track_launch_and_commit_{name}_{tag}"] = track_and_commit
    for fn in timed.values():
        fn()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    ratios = {name.replace("_motion", ""): med[name] / med[name.replace("_motion", "_plain")] for name in med if "_motion" in name}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": list(args.source), "size": [s, s],
              "score_threshold": thr, "similarity": args.similarity, "assignment": args.assignment, "max_tracks": t.max_tracks,
              "rounds": args.rounds, "constant_velocity": repr(t.motion), "tracked_per_image": tracked,
              "coasting_per_image": coasting, "coasting_rows_d2h_bytes_per_batch": int(t.out_bytes(b) - t.coast_offset(b)),
              "motion_state_bytes_one_stream_per_image": int(t.motion_state_bytes),
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()}, "motion_over_plain": ratios,
              "graph_added_ms_one_stream": med["graph_motion_one_stream"] - med["graph_plain_one_stream"],
              "graph_added_ms_one_stream_per_image": med["graph_motion_one_stream_per_image"] - med["graph_plain_one_stream_per_image"]}
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged["motion"] = result
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print(json.dumps({"motion": result}))


def optimal_leg(args, det, frames):
    from multiposenet_amd.inference import PoseTracker
    from multiposenet_amd.pose_metrics import fill_record
    import track_assign_cases as acases
    import track_assign_ref as opt
    b, s, thr = args.batch, args.size, args.threshold
    device = torch.device("cuda", 0)
    timed, tracked = {}, {}
    for streams in (1, b):
        kw = dict(streams=streams, similarity=args.similarity, max_boxes=det.params['max_boxes'])
        trackers = {"greedy": PoseTracker(**kw), "optimal": PoseTracker(assignment='optimal', **kw)}
        tag = "one_stream" if streams == 1 else "one_stream_per_image"
        for name, t in trackers.items():                               # warm-up: graphs captured, states filled
            for _ in range(3):
                outs = det.predict_images(frames, size=(s, s), score_threshold=thr, track=t)
            tracked[f"{name}_{tag}"] = sum(int((o['track_ids'] > 0).sum()) for o in outs) / b
            ent = next(e for e in det._graphs.values() if getattr(e, 'track', None) is t)
            whole = ent.outs['record']
            nbytes = whole.numel() - t.out_bytes(b)

            def track_and_commit(t=t, record=whole[:nbytes], rows=whole[nbytes:]):
                t.launch(record, rows, b)
                t.commit()
            timed[f"graph_{name}_{tag}"] = ent.graph.replay
            timed[f"track_launch_and_commit_{name}_{tag}"] = track_and_commit
    # the launch alone on the records made for it: a state with 64 live tracks, then --batch frames in one launch, not committed
    # (the launch is pure: every repeat does the same work)
    chain = acases.chain(64)
    made = {"chain64": [chain[0]] + [chain[1 - f % 2] for f in range(b)], "random64": acases.random64(frames=b + 1)}
    searches = {}
    for case, seq in made.items():
        p = acases.iou_params(64, 0.3)
        state, log = opt.new_state(1, 64), []
        opt.run(seq, state, p, log)
        steps = [e[3] for e in log if e[0] == 'path']
        searches[case] = {"scan_trips_per_batch": sum(steps), "longest_search": max(steps), "longest_path": opt.longest_path(log)}
        record = torch.from_numpy(fill_record(seq[1:], b, 64)[0]).to(device)
        for name in ("greedy", "optimal"):
            t = PoseTracker(1, 64, 'iou', 0.3, acases.MAX_MISSES, acases.NEW_TRACK_SCORE, 64, assignment=name)
            t.update(seq[:1])
            rows = torch.zeros(t.out_bytes(b), dtype=torch.uint8, device=device)
            timed[f"launch_{name}_{case}"] = lambda t=t, record=record, rows=rows: t.launch(record, rows, b)
    for fn in timed.values():
        fn()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    ratios = {name.replace("_optimal", ""): med[name] / med[name.replace("_optimal", "_greedy")] for name in med if "_optimal" in name}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": list(args.source), "size": [s, s],
              "score_threshold": thr, "similarity": args.similarity, "max_tracks": 32, "rounds": args.rounds,
              "tracked_per_image": tracked, "made_records": {"similarity": "iou", "max_tracks": 64, "max_boxes": 64, **searches},
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()}, "optimal_over_greedy": ratios,
              "graph_added_ms_one_stream": med["graph_optimal_one_stream"] - med["graph_greedy_one_stream"]}
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged["optimal"] = result
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print(json.dumps({"optimal": result}))


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
    ap.add_argument("--smooth", action="store_true", help="only the smoothing leg; merged into --out under 'smooth'")
    ap.add_argument("--assignment", default="greedy", choices=["greedy", "optimal"],
                    help="optimal: only the optimal-assignment leg; merged into --out under 'optimal'")
    ap.add_argument("--motion", action="store_true",
                    help="only the motion leg (with --assignment: of that assignment); merged into --out under 'motion'")
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
    if args.smooth:
        return smooth_leg(args, det, frames)
    if args.motion:
        return motion_leg(args, det, frames)
    if args.assignment == "optimal":
        return optimal_leg(args, det, frames)
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
    if os.path.exists(args.out):                                       # the --smooth and --assignment optimal runs' records stay
        with open(args.out) as f:
            result.update({k: v for k, v in json.load(f).items() if k in ("smooth", "optimal", "motion")})
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
