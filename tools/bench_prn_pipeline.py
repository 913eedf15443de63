"""Cost of the PRN input pipeline: device time of `mpn_prn_examples`, the host rates, and whether the host side starves
the PRN train step.

    python tools/bench_prn_pipeline.py [--iters 500] [--steps 300] [--records 256] [--dtype bf16]

Prints one JSON line. Annotations are toy-shard-like (the generator of tools/make_toy_tfrecords.py: 1-4 persons per image,
uniform, images 200-480 x 240-640; the records carry a JPEG header instead of pixels - they are never decoded - padded to
`--record-bytes` so that reading from files moves a realistic number of bytes):
  kernel_us            device time per `mpn_prn_examples` call at batch 32 and 128 (HIP events around `iters` launches after
                       warm-up, two runs each), the bytes it writes (crops + labels) and that over 6.3 TB/s (the rate a
                       float4 copy reaches on the MI355X)
  host examples / s    `PoseResidualNetworkPipeline.samples()` on one thread, served from the annotation cache and from
                       files (a fresh cache per pass)
  train steps / s      the step loop of `train_prn.train` (one `model_fn` TRAIN call per batch; batch 32 and 128, no checkpoint
                       inside the timed window) fed by the pipeline, against the same loop fed one resident batch, two
                       alternating runs each - the ratio tells whether the host side starves the step
"""
import argparse
import json
import os
import shutil
import struct
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _jpeg_header(height, width, pad):
    frame = struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    seg = lambda m, p: bytes([0xFF, m]) + struct.pack(">H", len(p) + 2) + p   # noqa: E731
    return b"\xff\xd8" + seg(0xC0, frame) + seg(0xDA, bytes(10)) + bytes(pad) + b"\xff\xd9"


def _toy_record(rng, record_bytes):
    h, w = int(rng.integers(200, 481)), int(rng.integers(240, 641))
    p = int(rng.integers(1, 5))
    boxes, kps = [], []
    for _ in range(p):
        bh, bw = rng.uniform(0.2, 0.8) * h, rng.uniform(0.1, 0.5) * w
        y0, x0 = rng.uniform(0, h - bh), rng.uniform(0, w - bw)
        boxes.append((y0, x0, y0 + bh, x0 + bw))
        y = np.clip(rng.uniform(y0, y0 + bh, 17), 0, h - 1).astype(np.int64)
        x = np.clip(rng.uniform(x0, x0 + bw, 17), 0, w - 1).astype(np.int64)
        kps.append(np.stack([y, x, rng.integers(0, 3, 17)], 1))
    return {"image": _jpeg_header(h, w, record_bytes), "num_persons": np.array([p], np.int64),
            "boxes": np.array(boxes, np.float32).reshape(-1), "keypoints": np.stack(kps).astype(np.int64).reshape(-1),
            "masks": b"\0"}


def main():
    import torch
    from multiposenet_amd import _lib, prn_model, train_prn
    from multiposenet_amd.detector.input_pipeline import AnnotationCache, PoseResidualNetworkPipeline
    from multiposenet_amd.detector.input_pipeline.tfrecord import encode_example, frame_record
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--records", type=int, default=256, help="records per shard (two shards)")
    ap.add_argument("--record-bytes", type=int, default=150000)
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prn_pipeline measures on the GPU"
    rng = np.random.default_rng(0)
    tmp = tempfile.mkdtemp(prefix="prn_bench_")
    paths = []
    for s in range(2):
        paths.append(os.path.join(tmp, f"shard-{s:04d}.tfrecords"))
        with open(paths[-1], "wb") as f:
            for _ in range(args.records):
                f.write(frame_record(encode_example(_toy_record(rng, args.record_bytes))))
    out = {"metric": "prn_pipeline", "persons_per_image": "uniform 1..4 (mean 2.5)", "records": 2 * args.records}
    cache = AnnotationCache()
    dev = "cuda"

    # ---- device: one call on fixed tables
    for B in (32, 128):
        pipe = PoseResidualNetworkPipeline(paths, True, B, annotations=cache, shuffle_buffer_size=512)
        t = next(pipe.samples())
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
        kp, bx, fp = up(t["keypoints"]), up(t["boxes"]), up(t["first_person"])
        w, h, ex = up(t["width"]), up(t["height"]), up(t["examples"])
        Q, R = len(t["boxes"]), len(t["width"])
        crops = torch.empty((B, 56, 36, 17), device=dev)
        labels = torch.empty_like(crops)
        nws = _lib.lib().mpn_prn_examples_workspace_bytes(Q)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)

        def launch():
            _lib.call("mpn_prn_examples", _lib.ptr(kp), _lib.ptr(bx), Q, _lib.ptr(fp), _lib.ptr(w), _lib.ptr(h), R,
                      _lib.ptr(ex), B, 56, 36, 4, _lib.ptr(crops), _lib.ptr(labels), _lib.ptr(ws), nws, _lib.stream_ptr())
        for _ in range(50):
            launch()
        torch.cuda.synchronize()
        runs = []
        for _ in range(2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                launch()
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / args.iters)
        nbytes = 2 * crops.numel() * 4
        out[f"b{B}"] = {"kernel_us_two_runs": [round(r, 2) for r in runs], "launches_per_call": 2, "images": R, "persons": Q,
                        "bytes_written": nbytes, "frac_of_6p3TBps": round(nbytes / (min(runs) * 1e-6) / 6.3e12, 3)}

    # ---- host: tables per second on one thread
    def rate(make, n_batches, B=32):
        it = make().samples()
        next(it)
        t0 = time.perf_counter()
        for _ in range(n_batches):
            next(it)
        return B * n_batches / (time.perf_counter() - t0)
    out["host_examples_per_s_cached"] = round(rate(
        lambda: PoseResidualNetworkPipeline(paths, True, 32, annotations=cache, shuffle_buffer_size=512), 400), 1)
    # from files: one evaluation pass with a fresh cache (every record is read and parsed once)
    t0 = time.perf_counter()
    n = sum(len(t["examples"]) for t in PoseResidualNetworkPipeline(paths, False, 32).samples())
    dt = time.perf_counter() - t0
    out["host_examples_per_s_from_files"] = round(n / dt, 1)
    out["host_records_per_s_from_files"] = round(2 * args.records / dt, 1)
    out["cache_bytes_per_person"] = round(cache.nbytes / cache.num_persons, 1)

    # ---- train loop: fed by the pipeline against one resident batch
    for B in (32, 128):
        res = {}
        for feed in ("resident", "pipeline", "resident", "pipeline"):
            prn_model.reset_registry()
            params = dict(train_prn.PARAMS, model_dir=os.path.join(tmp, f"m{B}"), batch_size=B, dtype=args.dtype,
                          num_steps=10 ** 6)
            pipe = PoseResidualNetworkPipeline(paths, True, B, annotations=cache, shuffle_buffer_size=512)
            if feed == "resident":
                c, l = next(pipe.batches())
                c, l = c.clone(), l.clone()

                def batches():
                    while True:
                        yield c, l
            else:
                batches = pipe.batches()
            net = train_prn._net(params)
            it = iter(batches() if callable(batches) else batches)
            mode = train_prn.ModeKeys.TRAIN
            for _ in range(30):                                    # warm-up: every shape, the allocator, the slots
                train_prn.model_fn(*next(it), mode, params)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                train_prn.model_fn(*next(it), mode, params)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res.setdefault(feed, []).append(round(args.steps / dt, 1))
            del net
        out[f"train_b{B}"] = {"steps_per_s_resident": res["resident"], "steps_per_s_pipeline": res["pipeline"],
                              "ms_per_step_resident": round(1e3 / max(res["resident"]), 3),
                              "ms_per_step_pipeline": round(1e3 / max(res["pipeline"]), 3),
                              "ratio_pipeline_over_resident": round(max(res["pipeline"]) / max(res["resident"]), 3)}
    prn_model.reset_registry()
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
