"""What COCO keypoint matching costs: `Detector.predict_images(..., groundtruth=)` - mpn_oks_match inside the captured graph -
against `predict_images` without it followed by the plain-loop numpy COCOeval matcher on the host (tests/pose_eval_ref.py:
what evaluation cost before the kernel existed), same process, same GPU.

    timeout -k 10 400 python tools/bench_pose_eval.py [--batch 16] [--source 720 1280] [--size 640] [--batches 8] [--rounds 5]
                                                      [--groundtruth 8] [--out profiles/pose_eval.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Legs, numpy in / numpy out, wall clock (time.perf_counter around calls that end in a device synchronise), both warmed up, then
ALTERNATING over `--rounds` rounds of `--batches` batches; the figure of a leg is its median round:
  A  predict_images_host_matcher   predict_images, then evaluate_image(output, ground truth) of the reference per image
  B  predict_images_groundtruth    predict_images(groundtruth=): the match tables come back with the record
Device time from HIP events around back-to-back work: replays of B's whole graph, and the mpn_oks_match launch alone on the
same buffers. The ground truth of an image is made from its own detections (the first `--groundtruth` persons moved by a
hundredth of their size, one crowd copy), so that the matcher has real matches to make. A run without a GPU fails."""
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

import pose_eval_ref as ref  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402


def groundtruth_from(outs, sizes, persons):
    gts = []
    for o, (h, w) in zip(outs, sizes):
        n = min(len(o['keypoints']), persons)
        b = o['boxes'][:n].astype(np.float64)
        boxes = np.stack([b[:, 1] * w, b[:, 0] * h, (b[:, 3] - b[:, 1]) * w, (b[:, 2] - b[:, 0]) * h], 1)
        kp = o['keypoints'][:n].astype(np.float64)
        kp[:, :, :2] += 0.01 * np.sqrt(np.abs(boxes[:, 2] * boxes[:, 3]))[:, None, None]
        kp[:, :, 2] = 2.0
        crowd = np.zeros(n, np.int32)
        if n:
            kp, boxes, crowd = np.concatenate([kp, kp[:1]]), np.concatenate([boxes, boxes[:1]]), np.append(crowd, 1)
        gts.append({'keypoints': kp, 'boxes': boxes, 'iscrowd': crowd})
    return gts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=8, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--groundtruth", type=int, default=8, help="ground-truth persons per image (+ one crowd copy)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "pose_eval.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_eval: no GPU (a measurement path does not fall back)")
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw          # structure at the network's scale (bench_predict_images.py)
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    sizes = [f.shape[:2] for f in frames]
    first = det.predict_images(frames, size=(s, s), score_threshold=thr)
    gts = groundtruth_from(first, sizes, args.groundtruth)

    def leg_a():
        matched = 0
        for _ in range(args.batches):
            outs = det.predict_images(frames, size=(s, s), score_threshold=thr)
            for o, g in zip(outs, gts):
                matched += int((ref.evaluate_image(o, g)['matches'][:, 0, 0] >= 0).sum())
        return matched

    def leg_b():
        matched = 0
        for _ in range(args.batches):
            for o in det.predict_images(frames, size=(s, s), score_threshold=thr, groundtruth=gts):
                matched += int((o['oks']['matches'][:, 0, 0] >= 0).sum())
        return matched

    legs = [("predict_images_host_matcher", leg_a), ("predict_images_groundtruth", leg_b)]
    matched = {name: fn() for name, fn in legs}                        # warm-up: every shape the timed window uses
    if matched["predict_images_host_matcher"] != matched["predict_images_groundtruth"]:
        raise SystemExit(f"bench_pose_eval: the legs disagree on the matches at OKS .5: {matched}")
    t0 = time.perf_counter()
    for o, g in zip(first, gts):
        ref.evaluate_image(o, g)
    host_matcher_ms = (time.perf_counter() - t0) * 1e3 / b
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    ent = next(e for k, e in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and "oks" in k)
    plain = next(e for k, e in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and "oks" not in k)
    whole = ent.outs['record']
    nbytes = whole.numel() - ent.oks.out_bytes
    graph_ms = [events_ms(ent.graph.replay, 20) / b for _ in range(args.rounds)]
    plain_ms = [events_ms(plain.graph.replay, 20) / b for _ in range(args.rounds)]
    match_ms = [events_ms(lambda: ent.oks.launch(whole[:nbytes], whole[nbytes:]), 20) / b for _ in range(args.rounds)]

    def spread(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": [sh, sw], "size": [s, s],
              "score_threshold": thr, "batches_per_leg_round": args.batches, "rounds": args.rounds,
              "detections_per_image": sum(len(o['scores']) for o in first) / b,
              "groundtruth_per_image": sum(len(g['keypoints']) for g in gts) / b,
              "matches_at_oks_50_per_image": matched["predict_images_groundtruth"] / (args.batches * b),
              "host_matcher": "tests/pose_eval_ref.py evaluate_image (plain-loop numpy COCOeval, one thread)",
              "host_matcher_ms_per_image": host_matcher_ms,
              "groundtruth_h2d_bytes_per_batch": int(ent.oks.stage.numel() * 8), "match_rows_d2h_bytes_per_batch": int(ent.oks.out_bytes),
              "legs": {}, "device_ms_per_image": {"graph_with_groundtruth": spread(graph_ms), "graph_without": spread(plain_ms),
                                                   "oks_match_launch": spread(match_ms)}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": spread([x * 1e3 for x in w]), "wall_images_per_s": 1.0 / statistics.median(w)}
    result["in_graph_speedup"] = (result["legs"]["predict_images_groundtruth"]["wall_images_per_s"]
                                  / result["legs"]["predict_images_host_matcher"]["wall_images_per_s"])
    result["match_share_of_graph_device_time"] = statistics.median(match_ms) / statistics.median(graph_ms)
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
