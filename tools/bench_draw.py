"""Annotated frames: `Detector.predict_images(annotate=True)` (the drawing on the device, inside the captured graph) against
what it replaces - `predict_images(annotate=False)` followed by the notebook-equivalent Pillow drawing of every frame on the
host - same process, same GPU, and the device time of the draw launches against the bytes they must move.

    timeout -k 10 600 python tools/bench_draw.py [--batch 16] [--source 1080 1920] [--size 640] [--batches 4] [--rounds 5]
                                                 [--replays 100] [--out profiles/draw_detections.json]

(one process, one GPU step: run it under a `timeout` of its own as above.)

Setup as tools/bench_predict_images.py: bf16, 25 persons per image (the lively head). Legs, numpy in / numpy out, wall clock:
  A  predict_images_then_host_draw   annotate=False, then per frame Image.fromarray, putalpha(255), ImageDraw rectangle / 16
                                     lines / 17 ellipses per person, np.asarray. Not measured when Pillow is absent.
  B  predict_images_annotate         annotate=True.
Both are warmed up, then ALTERNATE over `--rounds` rounds of `--batches` batches; the figure of a leg is its median round.
Device time (HIP events, warm, `--replays` launches back to back): mpn_draw_detections alone on the graph's own buffers, against
3 bytes read + 4 written per source pixel, and a plain device copy of as many bytes for scale; the device-to-host copy of the
annotated frames into pinned memory, and the host's copy out of it. A run without a GPU fails; nothing here falls back.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_inference_batch import build_detector  # noqa: E402  (the lively head: 25 persons per image)
from tools.bench_predict_images import events_ms  # noqa: E402

# the skeleton as (keypoint, keypoint): the limbs mpn_draw_detections draws
EDGES = ((0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 7), (5, 11), (6, 8), (6, 12), (7, 9), (8, 10), (11, 13), (12, 14),
         (13, 15), (14, 16))


def host_drawer():
    """(name, draw(frame, person) -> uint8 [h, w, 4]) with Pillow, or (None, None)."""
    try:
        import PIL
        from PIL import Image, ImageDraw
    except ImportError:
        return None, None

    def draw(frame, person):
        im = Image.fromarray(frame)
        im.putalpha(255)
        d = ImageDraw.Draw(im, "RGBA")
        w, h = im.size
        boxes = np.array([h, w, h, w]) * person["boxes"]
        for box, pos in zip(boxes, person["keypoint_positions"]):
            ymin, xmin, ymax, xmax = box
            d.rectangle([(xmin, ymin), (xmax, ymax)], outline="red")
            kp = pos[:, ::-1].copy()
            kp *= np.array([xmax - xmin, ymax - ymin])
            kp += np.array([xmin, ymin])
            for p, q in EDGES:
                d.line([tuple(kp[p]), tuple(kp[q])])
            for x, y in kp:
                d.ellipse([(x - 2, y - 2), (x + 2, y + 2)], fill="red")
        return np.asarray(im)

    return f"Pillow {PIL.__version__} ImageDraw (one thread)", draw


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=4, help="batches per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=os.path.join("profiles", "draw_detections.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_draw: no GPU (a measurement path does not fall back)")
    det = build_detector(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    b, s, thr = args.batch, args.size, args.threshold
    sh, sw = args.source
    rng = np.random.RandomState(0)
    yy, xx = np.arange(sh) * s // sh, np.arange(sw) * s // sw      # frames as tools/bench_predict_images.py makes them
    frames = [np.ascontiguousarray(rng.randint(0, 256, (s, s, 3)).astype(np.uint8)[yy][:, xx]) for _ in range(b)]
    drawer_name, host_draw = host_drawer()

    def leg_a():
        persons = det.predict_images(frames, size=(s, s), score_threshold=thr)
        for f, p in zip(frames, persons):
            p["annotated"] = host_draw(f, p)
        return persons

    def leg_b():
        return det.predict_images(frames, size=(s, s), score_threshold=thr, annotate=True)

    legs = [("predict_images_annotate", leg_b)] + ([("predict_images_then_host_draw", leg_a)] if host_draw else [])
    first = {name: fn() for name, fn in legs}                       # warm-up: graphs, buffers, pinned staging
    persons_per_image = sum(len(p["boxes"]) for p in first["predict_images_annotate"]) / b
    equal = None
    if host_draw:
        equal = all(np.array_equal(x["annotated"], y["annotated"]) for x, y in
                    zip(first["predict_images_annotate"], first["predict_images_then_host_draw"]))
    wall = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                fn()
            wall[name].append((time.perf_counter() - t0) / (args.batches * b))
    host_draw_ms = None
    if host_draw:
        plain = det.predict_images(frames, size=(s, s), score_threshold=thr)
        t0 = time.perf_counter()
        for f, p in zip(frames, plain):
            host_draw(f, p)
        host_draw_ms = (time.perf_counter() - t0) * 1e3 / b

    ent = next(v for k, v in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and k[-1] == "annotate")
    buf, record = ent.draw, ent.outs["record"]
    pixels = sum(f.shape[0] * f.shape[1] for f in frames)
    moved = 7 * pixels
    draw_ms = [events_ms(lambda: buf.launch(ent.sources, record, True), args.replays) for _ in range(args.rounds)]
    graph_ms = [events_ms(ent.graph.replay, 20) for _ in range(args.rounds)]
    plain_graph = next(v for k, v in det._graphs.items() if isinstance(k, tuple) and k[0] == "images" and k[-1] != "annotate").graph
    plain_graph_ms = [events_ms(plain_graph.replay, 20) for _ in range(args.rounds)]
    a, c = torch.empty(moved // 2, dtype=torch.uint8, device=buf.out.device), torch.empty(moved // 2, dtype=torch.uint8, device=buf.out.device)
    copy_ms = [events_ms(lambda: c.copy_(a), args.replays) for _ in range(args.rounds)]
    nb, pinned = buf.out_bytes, ent.host["annotated"]
    d2h_ms = [events_ms(lambda: pinned[:nb].copy_(buf.out[:nb], non_blocking=True), 10) for _ in range(args.rounds)]
    t0 = time.perf_counter()
    for _ in range(3):
        buf.unpack(pinned.numpy())
    unpack_ms = (time.perf_counter() - t0) * 1e3 / 3

    med = statistics.median
    annotated_wall_ms = med(wall["predict_images_annotate"]) * 1e3 * b      # per batch
    result = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "batch": b, "source": [sh, sw], "size": [s, s],
              "score_threshold": thr, "batches_per_leg_round": args.batches, "rounds": args.rounds, "replays": args.replays,
              "persons_per_image": persons_per_image,
              "host_draw": drawer_name or "not measured: Pillow is not importable",
              "host_draw_ms_per_image": host_draw_ms, "device_frames_equal_host_frames": equal,
              "draw_launches": {"device_ms_per_image": {k: v / b for k, v in stats(draw_ms).items()},
                                "bytes_per_image": moved // b, "GB_per_s": moved / (med(draw_ms) * 1e-3) / 1e9,
                                "plain_device_copy_of_as_many_bytes_GB_per_s": moved / (med(copy_ms) * 1e-3) / 1e9,
                                "share_of_copy_rate": med(copy_ms) / med(draw_ms)},
              "graph_device_ms_per_image": {"annotate": {k: v / b for k, v in stats(graph_ms).items()},
                                            "plain": {k: v / b for k, v in stats(plain_graph_ms).items()}},
              "annotated_d2h": {"bytes_per_batch": int(nb), "device_ms_per_batch": stats(d2h_ms),
                                "GB_per_s": nb / (med(d2h_ms) * 1e-3) / 1e9,
                                "host_copy_out_of_pinned_ms_per_batch": unpack_ms,
                                "d2h_share_of_annotated_call": med(d2h_ms) / annotated_wall_ms,
                                "host_copy_share_of_annotated_call": unpack_ms / annotated_wall_ms},
              "legs": {}}
    for name, _ in legs:
        w = sorted(wall[name])
        result["legs"][name] = {"wall_ms_per_image": {"median": med(w) * 1e3, "min": w[0] * 1e3, "max": w[-1] * 1e3},
                                "wall_images_per_s": 1.0 / med(w)}
    if host_draw:
        result["annotate_speedup_over_host_draw"] = (result["legs"]["predict_images_annotate"]["wall_images_per_s"]
                                                     / result["legs"]["predict_images_then_host_draw"]["wall_images_per_s"])
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
