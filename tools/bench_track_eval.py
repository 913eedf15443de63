"""What scoring the tracker's identities costs: `Detector.predict_images(..., track=, groundtruth=, track_eval=)` - mpn_track_eval
behind the tracker's launch inside the captured graph, its state advanced by one small device copy - against the same call
without `track_eval=` in the same process, and against that call followed by the plain-loop numpy definition on the host
(tests/track_eval_ref.py: what the evaluation costs without the kernel).

    timeout -k 10 400 python tools/bench_track_eval.py [--batch 16] [--source 720 1280] [--size 640] [--batches 4] [--rounds 5]
                                                       [--out profiles/track_eval.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

The record is that of tools/bench_pose_track.py: --batch unrelated random frames of one stream, the lively head's 25 persons per
image. The ground truth is every frame's own persons, each with an identity of its own (25 x --batch identities a stream), so
that the similarity matrix, the masks and the assignment run at the record's full load; few persons of a frame are found
again in the next, so most tracked persons of a frame are new tracks. Measured, all warmed up:
  device time (HIP events around 20 back-to-back repeats, medians of --rounds rounds with their ranges), ALTERNATING:
    the captured graph with track= and groundtruth= (what the parent commit runs), and the same with track_eval=;
    the mpn_track_eval launch plus its commit alone, and the tracker's launch plus its commit alone, on that record;
    the mpn_track_eval launch alone as it is, with a threshold no pair reaches, and without ground truth (where its time goes);
  wall clock, numpy in / numpy out, ALTERNATING over --rounds rounds of --batches batches:
    predict_images(track=, groundtruth=, track_eval=), and predict_images(track=, groundtruth=) followed by
    track_eval_ref.run on the returned dicts.
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

import track_eval_ref as ref  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=4, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "track_eval.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_eval: no GPU (a measurement path does not fall back)")
    from multiposenet_amd.inference import PoseTracker, TrackEvaluator
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw          # structure at the network's scale (bench_predict_images.py)
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    max_boxes = det.params['max_boxes']
    plain = det.predict_images(frames, size=(s, s), score_threshold=thr)
    groundtruth, identities = [], []
    for f, o in enumerate(plain):
        kp = o['keypoints'].astype(np.float64)
        kp[:, :, 2] = 2
        box = o['boxes'].astype(np.float64)
        ids = f * max_boxes + np.arange(len(kp))
        groundtruth.append({'keypoints': kp, 'track_ids': ids,
                            'boxes': np.stack([box[:, 1] * sw, box[:, 0] * sh, (box[:, 3] - box[:, 1]) * sw, (box[:, 2] - box[:, 0]) * sh], 1)})
        identities.append(ids.astype(np.int32))
    kw = dict(streams=1, similarity='oks', max_boxes=max_boxes)
    with_eval, without = PoseTracker(**kw), PoseTracker(**kw)
    evaluator = TrackEvaluator(streams=1, max_identities=1024, max_boxes=max_boxes)
    host_state = ref.new_state(1, 1024)
    host_ms = []

    def leg_device():
        outs = det.predict_images(frames, size=(s, s), score_threshold=thr, track=with_eval, groundtruth=groundtruth, track_eval=evaluator)
        return sum(o['track_eval']['matches'] for o in outs)

    def leg_host():
        outs = det.predict_images(frames, size=(s, s), score_threshold=thr, track=without, groundtruth=groundtruth)
        t0 = time.perf_counter()
        rows = ref.run(outs, groundtruth, identities, host_state, evaluator.threshold)
        host_ms.append((time.perf_counter() - t0) * 1e3 / b)
        return sum(int(r['frame']['matches']) for r in rows)

    legs = [("predict_images_track_eval", leg_device), ("predict_images_host_evaluation", leg_host)]
    matches = {name: [fn() for _ in range(2)][-1] for name, fn in legs}     # warm-up: graphs captured, states filled
    del host_ms[:]
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    ents = {"with": next(e for e in det._graphs.values() if getattr(e, 'track_eval', None) is evaluator),
            "without": next(e for e in det._graphs.values() if getattr(e, 'track', None) is without)}
    ent = ents["with"]
    whole = ent.outs['record']
    layout = ent.layout                                             # the entry's own: where each stage's rows lie
    record, track_rows, eval_rows = whole[layout.record], whole[layout.track], whole[layout.track_eval]

    def eval_and_commit():
        evaluator.launch(record, track_rows[:with_eval.track_bytes(b)], eval_rows, b, *ent.oks.device_groundtruth())
        evaluator.commit()

    def track_and_commit():
        with_eval.launch(record, track_rows, b)
        with_eval.commit()
    timed = {"graph_with_track_eval": ents["with"].graph.replay, "graph_without": ents["without"].graph.replay,
             "track_eval_launch_and_commit": eval_and_commit, "track_launch_and_commit": track_and_commit}
    # where the launch's time goes: the same launch (alone, not committed: it is pure, every repeat does the same work) on the
    # same record with the ground truth in the evaluator's own buffers, with a threshold no pair reaches (the similarities and the
    # masks are computed, nothing is kept and no row enters the assignment), and without any ground
    # truth (the walk over the frames, the barriers and the rows alone)
    nobody = {'keypoints': np.zeros((0, 17, 3)), 'boxes': np.zeros((0, 4)), 'track_ids': np.zeros(0, np.int64)}
    spare = torch.zeros_like(eval_rows)
    for name, threshold, gts in (("track_eval_launch", evaluator.threshold, groundtruth),
                                 ("track_eval_launch_no_eligible_pair", 1e9, groundtruth),
                                 ("track_eval_launch_no_groundtruth", evaluator.threshold, [nobody] * b)):
        probe = TrackEvaluator(streams=1, threshold=threshold, max_identities=1024, max_boxes=max_boxes)
        probe.place(gts, b)
        timed[name] = lambda probe=probe: probe.launch(record, track_rows[:with_eval.track_bytes(b)], spare, b)
    timed["track_launch"] = lambda: with_eval.launch(record, track_rows, b)
    for fn in timed.values():
        fn()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "streams": 1, "source": [sh, sw],
              "size": [s, s], "score_threshold": thr, "eval_threshold": evaluator.threshold, "rounds": args.rounds,
              "batches_per_leg_round": args.batches, "persons_per_image": sum(len(o['scores']) for o in plain) / b,
              "matches_per_batch": matches, "host_evaluation": "tests/track_eval_ref.py run (plain-loop numpy, one thread)",
              "host_evaluation_ms_per_image": spread(host_ms), "eval_rows_d2h_bytes_per_batch": int(evaluator.out_bytes(b)),
              "identity_h2d_bytes_per_batch": 4 * b * evaluator.max_gt, "state_bytes": int(evaluator.state_bytes),
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "graph_added_ms": med["graph_with_track_eval"] - med["graph_without"],
              "graph_with_track_eval_over_without": med["graph_with_track_eval"] / med["graph_without"],
              "track_eval_over_track_launch": med["track_eval_launch_and_commit"] / med["track_launch_and_commit"], "legs": {}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": spread([x * 1e3 for x in w]), "wall_images_per_s": 1.0 / statistics.median(w)}
    result["track_eval_rate_over_host_evaluation"] = (result["legs"]["predict_images_track_eval"]["wall_images_per_s"] /
                                                      result["legs"]["predict_images_host_evaluation"]["wall_images_per_s"])
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
