"""What cutting out persons on the device costs: the captured graph of `Detector.predict_images(crops=)` for both formats
against the same graph without it in the same process, the stage's launches alone against a plain device copy of the bytes
they read and write, the images/s of the call against `annotate=True` followed by Pillow crops on the host, and the bytes each
route brings to the host per batch.

    timeout -k 10 600 python tools/bench_person_crops.py [--batch 16] [--source 720 1280] [--size 640] [--batches 4] [--rounds 5]
                                                         [--crop 256 128] [--out profiles/person_crops.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Device time from HIP events around 20 back-to-back repeats, ALTERNATING over `--rounds` rounds; a figure is its median round,
written with its minimum and maximum:
  graph_without / graph_rgb / graph_jpeg   replays of the captured graphs of the same Detector on the same frames
  stage_rgb / stage_jpeg                   mpn_person_crops alone (two launches; jpeg: and the encoder's two) on the record the
                                           graph's gather wrote
  device_copy                              `Tensor.copy_`, device to device, of as many bytes as the stage reads and writes at
                                           least once: the frames and every slot of the crop buffer
Wall clock, numpy in / numpy out (time.perf_counter around calls that end in a device synchronise), warmed up, alternating:
`predict_images` images/s without the stage, with it (per format), and `predict_images(annotate=True)` followed by
`Image.fromarray(annotated RGB).resize(size, BICUBIC, box=rect)` on the host for every person - what a deployment without the
stage runs today. The unused slots are encoded too (format='jpeg'): that cost is in graph_jpeg and stage_jpeg.
The weights are seeded random ones (tools/bench_inference_batch.py's lively head: 25 persons per image, the person count
tools/bench_anonymize.py uses). A run without a GPU fails."""
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

from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402

FORMATS = ("rgb", "jpeg")


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--crop", type=int, nargs=2, default=(256, 128), metavar=("H", "W"))
    ap.add_argument("--batches", type=int, default=4, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "person_crops.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_person_crops: no GPU (a measurement path does not fall back)")
    from PIL import Image

    from multiposenet_amd.inference import PersonCrops
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    specs = {f: PersonCrops(size=tuple(args.crop), format=f, max_boxes=det.params['max_boxes']) for f in FORMATS}
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw          # structure at the network's scale (bench_predict_images.py)
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    copied = {}

    def call(**kw):
        return det.predict_images(frames, size=(s, s), score_threshold=thr, **kw)

    def leg(**kw):
        def run():
            return sum(len(o['scores']) for _ in range(args.batches) for o in call(**kw))
        return run

    def host_crops(outs):
        """Pillow on the annotated frames the host received: the crops of every person, and the bytes that crossed the link."""
        nbytes = 0
        for o in outs:
            frame = Image.fromarray(np.ascontiguousarray(o['annotated'][..., :3]))
            nbytes += o['annotated'].nbytes
            h, w = o['annotated'].shape[:2]
            for ymin, xmin, ymax, xmax in o['boxes'].astype(np.float64):
                x0, y0, x1, y1 = max(xmin * w, 0.0), max(ymin * h, 0.0), min(xmax * w, float(w)), min(ymax * h, float(h))
                if x1 - x0 > 0 and y1 - y0 > 0:
                    np.asarray(frame.resize((args.crop[1], args.crop[0]), Image.BICUBIC, box=(x0, y0, x1, y1)))
        return nbytes

    def host_leg():
        def run():
            n = 0
            for _ in range(args.batches):
                outs = call(annotate=True)
                copied["annotate_then_pillow"] = host_crops(outs)
                n += sum(len(o['scores']) for o in outs)
            return n
        return run
    legs = [("predict_images", leg())] + [(f"predict_images_crops_{f}", leg(crops=specs[f])) for f in FORMATS] + \
           [("predict_images_annotate_then_pillow", host_leg())]
    counts = {name: fn() for name, fn in legs}                         # warm-up: every graph captured
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    outs = call(crops=specs["rgb"])
    copied["crops_rgb"] = sum(o['crops'].nbytes for o in outs)
    outs = call(crops=specs["jpeg"])
    copied["crops_jpeg"] = sum(len(data) for o in outs for data in o['crops'])

    def entry(fmt):
        for k, e in det._graphs.items():
            if isinstance(k, tuple) and k[0] == "images" and "annotate" not in k and \
                    (("crops" in k and k[-1] == specs[fmt]) if fmt else "crops" not in k):
                return e
        raise SystemExit(f"bench_person_crops: no graph for {fmt}")
    plain = entry(None)
    ents = {f: entry(f) for f in FORMATS}
    first = ents["rgb"]
    frame_bytes = sum(f.size for f in frames)
    info_bytes = first.crops.info.numel()
    record = first.outs['record']
    moved = frame_bytes + first.crops.out.numel()
    src = torch.empty(moved, dtype=torch.uint8, device=first.sources.device)
    dst = torch.empty_like(src)
    timed = {"graph_without": plain.graph.replay}
    for f in FORMATS:
        timed[f"graph_{f}"] = ents[f].graph.replay
    for f in FORMATS:
        timed[f"stage_{f}"] = (lambda e: lambda: e.crops.launch(e.sources, record))(ents[f])
    timed["device_copy"] = lambda: dst.copy_(src)
    for fn in timed.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in timed}
    for _ in range(args.rounds):
        for name, fn in timed.items():
            ms[name].append(events_ms(fn, 20))
    med = {name: statistics.median(v) for name, v in ms.items()}
    persons = counts["predict_images"] / (args.batches * b)
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": [sh, sw], "size": [s, s],
              "score_threshold": thr, "specs": {f: repr(v) for f, v in specs.items()}, "max_boxes": det.params['max_boxes'],
              "batches_per_leg_round": args.batches, "rounds": args.rounds, "repeats_per_round": 20,
              "persons_per_image": persons, "frame_bytes_per_batch": frame_bytes, "crop_buffer_bytes": first.crops.out.numel(),
              "device_copy_bytes": moved,
              "device_ms_per_batch": {name: spread(v) for name, v in ms.items()},
              "graph_added_ms": {f: med[f"graph_{f}"] - med["graph_without"] for f in FORMATS},
              "graph_over_without": {f: med[f"graph_{f}"] / med["graph_without"] for f in FORMATS},
              "stage_over_device_copy": {f: med[f"stage_{f}"] / med["device_copy"] for f in FORMATS},
              "device_to_host_bytes_per_batch": {"crops_rgb": copied["crops_rgb"] + info_bytes, "crops_jpeg": copied["crops_jpeg"] + info_bytes,
                                                 "annotate_then_pillow": copied["annotate_then_pillow"]},
              "legs": {}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": spread([x * 1e3 for x in w]), "wall_images_per_s": 1.0 / statistics.median(w)}
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
