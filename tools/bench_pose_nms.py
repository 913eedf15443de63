"""What keypoint-similarity NMS costs: `Detector.predict_images(..., pose_nms=)` - mpn_pose_nms behind the gather inside the
captured graph - against the same call without it in the same process.

    timeout -k 10 400 python tools/bench_pose_nms.py [--batch 16] [--source 720 1280] [--size 640] [--batches 8] [--rounds 5]
                                                     [--threshold-nms 0.9] [--out profiles/pose_nms.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Device time from HIP events around 20 back-to-back repeats, ALTERNATING over `--rounds` rounds; a figure is its median round,
written with its minimum and maximum:
  graph_with_pose_nms / graph_without   replays of the two captured graphs of the same Detector on the same frames
  pose_nms_launches                     mpn_pose_nms alone (its two launches) on the record the graph's gather wrote
  pose_nms_launches_hard_record         the same on a hand-made record of --batch x 64 persons where nothing is suppressed
                                        (tests/pose_nms_cases.py, image 4): all 2016 pairs of every image are computed and
                                        every row is copied
Wall clock, numpy in / numpy out (time.perf_counter around calls that end in a device synchronise), warmed up, alternating:
`predict_images` images/s with and without `pose_nms=`.
The weights are seeded random ones (tools/bench_inference_batch.py's lively head: 25 persons per image); how many persons
the stage drops on them says nothing about trained weights, and nothing here says anything about AP or tracking quality.
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

import pose_nms_cases as cases  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=8, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--threshold-nms", type=float, default=None, help="PoseNms's threshold (default: the class's)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "pose_nms.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_nms: no GPU (a measurement path does not fall back)")
    from multiposenet_amd import pose_nms as stage
    from multiposenet_amd.inference import PoseNms
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    nms = PoseNms() if args.threshold_nms is None else PoseNms(args.threshold_nms)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw          # structure at the network's scale (bench_predict_images.py)
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]

    def leg(**kw):
        def run():
            return sum(len(o['scores']) for _ in range(args.batches)
                       for o in det.predict_images(frames, size=(s, s), score_threshold=thr, **kw))
        return run
    legs = [("predict_images", leg()), ("predict_images_pose_nms", leg(pose_nms=nms))]
    counts = {name: fn() for name, fn in legs}                         # warm-up: both graphs captured
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    ent = next(e for k, e in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and "pose_nms" in k)
    plain = next(e for k, e in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and "pose_nms" not in k)
    max_boxes = det.params['max_boxes']
    device = ent.nms.raw.device
    out = torch.zeros_like(ent.nms.raw)
    info = torch.zeros(ent.nms.info_bytes, dtype=torch.uint8, device=device)
    hard = torch.from_numpy(cases.pack([cases.images()[4]] * b, b=b, max_boxes=64)).to(device)
    hard_out = torch.zeros_like(hard)
    hard_info = torch.zeros(stage.info_layout(b, 64)[0], dtype=torch.uint8, device=device)
    timed = {"graph_with_pose_nms": ent.graph.replay, "graph_without": plain.graph.replay,
             "pose_nms_launches": lambda: stage.launch(ent.nms.raw, b, max_boxes, nms, out, info),
             "pose_nms_launches_hard_record": lambda: stage.launch(hard, b, 64, nms, hard_out, hard_info)}
    for fn in timed.values():
        fn()
    torch.cuda.synchronize()
    hard_kept = int(hard_out[:4].cpu().numpy().view(np.int32)[0])
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": [sh, sw], "size": [s, s],
              "score_threshold": thr, "pose_nms": repr(nms), "max_boxes": max_boxes, "batches_per_leg_round": args.batches,
              "rounds": args.rounds, "repeats_per_round": 20,
              "persons_per_image": counts["predict_images"] / (args.batches * b),
              "persons_per_image_after_pose_nms": counts["predict_images_pose_nms"] / (args.batches * b),
              "hard_record": {"persons_per_image": 64, "pairs_per_image": 2016, "kept_rows": hard_kept, "of": 64 * b},
              "info_d2h_bytes_per_batch": int(ent.nms.info_bytes), "unfiltered_record_bytes_kept_on_device": int(ent.nms.raw.numel()),
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "graph_added_ms": med["graph_with_pose_nms"] - med["graph_without"],
              "graph_with_pose_nms_over_without": med["graph_with_pose_nms"] / med["graph_without"],
              "pose_nms_share_of_graph_device_time": med["pose_nms_launches"] / med["graph_with_pose_nms"],
              "legs": {}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": spread([x * 1e3 for x in w]), "wall_images_per_s": 1.0 / statistics.median(w)}
    result["pose_nms_rate_over_plain"] = (result["legs"]["predict_images_pose_nms"]["wall_images_per_s"]
                                          / result["legs"]["predict_images"]["wall_images_per_s"])
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
