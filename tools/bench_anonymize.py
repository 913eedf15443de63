"""What anonymising persons on the device costs: the captured graph of `Detector.predict_images(annotate='jpeg', anonymize=)`
for each mode against the same graph without it in the same process, the stage's launches alone against a plain device copy
of the same frame bytes, and the images/s of the call against the same call followed by the reference on the host.

    timeout -k 10 600 python tools/bench_anonymize.py [--batch 16] [--source 720 1280] [--size 640] [--batches 4] [--rounds 5]
                                                      [--region head] [--out profiles/anonymize.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Device time from HIP events around 20 back-to-back repeats, ALTERNATING over `--rounds` rounds; a figure is its median round,
written with its minimum and maximum:
  graph_without / graph_<mode>          replays of the captured graphs of the same Detector on the same frames
  stage_<mode>                          mpn_anonymize alone (its three or four launches) on the record the graph's gather wrote
  device_copy                           `Tensor.copy_` of the same frame bytes, device to device: the floor of any stage that
                                        writes every frame once
Wall clock, numpy in / numpy out (time.perf_counter around calls that end in a device synchronise), warmed up, alternating:
`predict_images(annotate='jpeg')` images/s without the stage, with it (per mode), and without it but followed by
tests/anonymize_ref.py on the host for every frame (--host-frames of them per round, scaled: the reference is slow) - what a
deployment without the stage would run in some form; a JPEG re-encode on the host would come on top and is not counted.
The weights are seeded random ones (tools/bench_inference_batch.py's lively head: 25 persons per image), so the regions are
where random boxes and keypoints fall; nothing here says anything about how well a face is hidden.
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

import anonymize_ref as R  # noqa: E402
from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402

MODES = ("pixelate", "blur", "fill")


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
    ap.add_argument("--region", default="head", choices=["head", "box"])
    ap.add_argument("--host-frames", type=int, default=4, help="frames per round the host reference anonymises")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "anonymize.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_anonymize: no GPU (a measurement path does not fall back)")
    from multiposenet_amd.inference import Anonymize
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    specs = {mode: Anonymize(region=args.region, mode=mode) for mode in MODES}
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw          # structure at the network's scale (bench_predict_images.py)
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]

    def call(**kw):
        return det.predict_images(frames, size=(s, s), score_threshold=thr, annotate='jpeg', **kw)

    def leg(**kw):
        def run():
            return sum(len(o['scores']) for _ in range(args.batches) for o in call(**kw))
        return run

    def host_leg():
        """The call without the stage, then the reference on the host for --host-frames frames; the time of those frames is
        scaled to the whole batch."""
        t0 = time.perf_counter()
        outs = call()
        t1 = time.perf_counter()
        for frame, o in list(zip(frames, outs))[:args.host_frames]:
            R.anonymize_outputs(frame, o, specs["pixelate"])
        t2 = time.perf_counter()
        return (t1 - t0) + (t2 - t1) * b / min(args.host_frames, b)
    legs = [("predict_images", leg())] + [(f"predict_images_{m}", leg(anonymize=specs[m])) for m in MODES]
    counts = {name: fn() for name, fn in legs}                         # warm-up: every graph captured
    wall = {name: [] for name, _ in legs}
    host_wall = []
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
        torch.cuda.synchronize()
        host_wall.append(host_leg() / b)

    def entry(mode):
        for k, e in det._graphs.items():
            if isinstance(k, tuple) and k[0] == "images" and (("anonymize" in k and k[-1] == specs[mode]) if mode else "anonymize" not in k):
                return e
        raise SystemExit(f"bench_anonymize: no graph for {mode}")
    plain = entry(None)
    ents = {m: entry(m) for m in MODES}
    first = ents[MODES[0]]
    frame_bytes = sum(f.size for f in frames)
    record = first.outs['record']
    src, dst = first.sources[:frame_bytes], torch.empty(frame_bytes, dtype=torch.uint8, device=first.sources.device)
    with_kp = det.assigner is not None
    timed = {"graph_without": plain.graph.replay}
    for m in MODES:
        timed[f"graph_{m}"] = ents[m].graph.replay
    for m in MODES:
        timed[f"stage_{m}"] = (lambda e: lambda: e.anonymize.launch(e.sources, record, with_kp))(ents[m])
    timed["device_copy"] = lambda: dst.copy_(src)
    for fn in timed.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": [sh, sw], "size": [s, s],
              "score_threshold": thr, "specs": {m: repr(v) for m, v in specs.items()}, "max_boxes": det.params['max_boxes'],
              "batches_per_leg_round": args.batches, "rounds": args.rounds, "repeats_per_round": 20,
              "persons_per_image": counts["predict_images"] / (args.batches * b), "frame_bytes_per_batch": frame_bytes,
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "graph_added_ms": {m: med[f"graph_{m}"] - med["graph_without"] for m in MODES},
              "graph_over_without": {m: med[f"graph_{m}"] / med["graph_without"] for m in MODES},
              "stage_over_device_copy": {m: med[f"stage_{m}"] / med["device_copy"] for m in MODES},
              "legs": {}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": spread([x * 1e3 for x in w]), "wall_images_per_s": 1.0 / statistics.median(w)}
    result["legs"]["predict_images_then_host_reference"] = {
        "wall_ms_per_image": spread([x * 1e3 for x in host_wall]), "wall_images_per_s": 1.0 / statistics.median(host_wall),
        "host_frames_per_round": min(args.host_frames, b), "scaled_to_batch": True}
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
