"""Runnable replacement of the reference's `train_prn.py` (:7-65): PARAMS, the curriculum over `max_keypoints` and the
tf.estimator loops with their cadence, on `prn_model.model_fn` (the HIP kernels) fed by `PoseResidualNetworkPipeline`.

    python -m multiposenet_amd.train_prn --train-dataset DIR --val-dataset DIR [--steps N] [--steps-per-keypoint K]
                                         [--model-dir DIR] [--batch B] [--dtype bf16|f32]

Training in three parts, as train_prn.py:51-65:
  1. the 14 curriculum stages max_keypoints = 4..17 of `steps_per_keypoint` steps each (NUM_STEPS_PER_KEYPOINT = 10000);
     every stage builds its own training pipeline and is followed by a checkpoint and a full evaluation (:54-58),
  2. the unfiltered stage up to `num_steps` (:61-62),
  3. during it, an evaluation every 3600 s (:63).
Run config (:36-41): summaries every 200 steps (`summaries.jsonl`), a checkpoint every 1800 s, a log line every 1000 steps.
Checkpoints are `model.ckpt-<step>.npz` (multiposenet_amd.checkpoint); a run resumes from the newest readable one.

Deviation: on resume the stage is derived from the restored `global_step` by `stage_for_step` - a restarted run goes on
where it stopped. The reference's script restarts its `for i in range(14)` loop at max_keypoints = 4 whatever the
checkpoint holds (each `estimator.train(steps=...)` adds NUM_STEPS_PER_KEYPOINT more steps).

Data: the TFRecord shards of the reference's data/create_tfrecords.py (tools/make_toy_tfrecords.py writes small ones of the
same contract). All stages of a run share one `AnnotationCache` per dataset, so the files are parsed once. `train()` takes
any iterator of (crops, labels) - f32 [b, 56, 36, 17] - or a callable returning one; a callable with a parameter receives
the stage's `max_keypoints` (None for the unfiltered stage).
"""
import argparse
import inspect
import json
import os
import time

import torch

from . import checkpoint, prn_model
from .keypoints_model import ModeKeys
from .prn import CROP_SIZE, NUM_KEYPOINTS
from .prn_model import model_fn
from .train_keypoints import dataset_files, latest_checkpoint

NUM_STEPS_PER_KEYPOINT = 10000   # train_prn.py:7
NUM_STEPS = 200000               # :8
FIRST_MAX_KEYPOINTS, NUM_CURRICULUM_STAGES = 4, 14   # :54-55: max_keypoints = i + 4 for i in range(14)

PARAMS = {   # train_prn.py:11-20
    'model_dir': 'models/run02/',
    'train_dataset': '/home/dan/datasets/COCO/multiposenet/train/',
    'val_dataset': '/home/dan/datasets/COCO/multiposenet/val/',

    'num_steps': NUM_STEPS,
    'initial_learning_rate': 1e-3,

    'batch_size': 32,
}
RUN_CONFIG = {'save_summary_steps': 200, 'save_checkpoints_secs': 1800, 'log_step_count_steps': 1000,   # train_prn.py:36-41
              'eval_start_delay_secs': 3600, 'eval_throttle_secs': 3600}                                 # :63


def stage_for_step(step, steps_per_keypoint=NUM_STEPS_PER_KEYPOINT):
    """The `max_keypoints` of the stage that global step `step` (the number of steps already taken) belongs to: 4..17 for
    the 14 curriculum stages of `steps_per_keypoint` steps each, None for the unfiltered stage that follows."""
    if step < 0 or steps_per_keypoint < 1:
        raise ValueError("step >= 0 and steps_per_keypoint >= 1")
    i = step // steps_per_keypoint
    return FIRST_MAX_KEYPOINTS + i if i < NUM_CURRICULUM_STAGES else None


def _open(batches, max_keypoints):
    if not callable(batches):
        return iter(batches)
    takes_stage = any(p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD, p.VAR_POSITIONAL)
                      for p in inspect.signature(batches).parameters.values())
    return iter(batches(max_keypoints) if takes_stage else batches())


def _net(params):
    """The variables `model_fn` trains under these params (prn_model's registry, keyed by model_dir)."""
    return prn_model._model(params, int(params["batch_size"]), tuple(CROP_SIZE) + (NUM_KEYPOINTS,))


def train(params, train_batches, val_batches=None, run_config=None, max_steps=None, steps_per_keypoint=None, log=print):
    """The three parts of train_prn.py:51-65 for the pose residual network. Returns the global step reached."""
    cfg = dict(RUN_CONFIG, **(run_config or {}))
    spk = int(steps_per_keypoint if steps_per_keypoint is not None else NUM_STEPS_PER_KEYPOINT)
    params = dict(params)
    net = _net(params)
    model_dir = params["model_dir"]
    os.makedirs(model_dir, exist_ok=True)
    last = latest_checkpoint(model_dir)
    if last is not None:
        checkpoint.load_npz(last[1], net)
        log(f"[train] restored {last[1]} (global_step {int(net.global_step.item())})")
    max_steps = int(max_steps if max_steps is not None else params["num_steps"])
    step = int(net.global_step.item())
    summaries = os.path.join(model_dir, "summaries.jsonl")
    clock = {"ckpt": time.time(), "log": time.time(), "step_log": step}
    clock["eval"] = time.time() + cfg["eval_start_delay_secs"] - cfg["eval_throttle_secs"]

    def save():
        path = os.path.join(model_dir, f"model.ckpt-{step}.npz")
        checkpoint.save_npz(path, net)
        log(f"[train] saved {path}")

    while step < max_steps:
        max_keypoints = stage_for_step(step, spk)
        stage_end = max_steps if max_keypoints is None else min(max_steps, (step // spk + 1) * spk)
        log(f"[train] step {step}: stage max_keypoints={max_keypoints} up to step {stage_end}")
        it = _open(train_batches, max_keypoints)
        while step < stage_end:
            crops, labels = next(it)
            spec = model_fn(crops, labels, ModeKeys.TRAIN, params)
            step += 1
            if step % cfg["save_summary_steps"] == 0:
                with open(summaries, "a") as f:
                    f.write(json.dumps({"step": step, "max_keypoints": max_keypoints, "logloss": float(spec.loss)}) + "\n")
            if step % cfg["log_step_count_steps"] == 0:
                torch.cuda.synchronize()
                now = time.time()
                log(f"[train] step {step}: loss {float(spec.loss):.4f}, "
                    f"{(step - clock['step_log']) / (now - clock['log']):.2f} steps/s")
                clock["log"], clock["step_log"] = now, step
            now = time.time()
            if now - clock["ckpt"] >= cfg["save_checkpoints_secs"]:
                save()
                clock["ckpt"] = now
            if max_keypoints is None and val_batches is not None and now - clock["eval"] >= cfg["eval_throttle_secs"]:
                evaluate(params, val_batches, log=log, step=step)
                clock["eval"] = now
        del it
        if max_keypoints is not None:            # estimator.train() ends on a checkpoint; then estimator.evaluate (:57-58)
            save()
            clock["ckpt"] = time.time()
            if val_batches is not None:
                evaluate(params, val_batches, log=log, step=step)
    if latest_checkpoint(model_dir) is None or latest_checkpoint(model_dir)[0] != step:
        save()
    return step


def evaluate(params, val_batches, log=print, step=None):
    """estimator.evaluate(steps=None): one pass over the validation batches, the partial last one included; the mean of
    `eval_loss` over the batches (tf.metrics.mean of the per-batch loss, prn_model.py:34-37)."""
    total, n = 0.0, 0
    for crops, labels in _open(val_batches, None):
        spec = model_fn(crops, labels, ModeKeys.EVAL, params)
        total += float(spec.eval_metric_ops["eval_loss"])
        n += 1
    out = {"eval_loss": total / max(n, 1)}
    log(f"[eval] step {step}: eval_loss {out['eval_loss']:.5f} over {n} batches")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-dataset", default=None, help="directory of training TFRecords (default: PARAMS)")
    ap.add_argument("--val-dataset", default=None, help="directory of evaluation TFRecords (default: PARAMS)")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--steps-per-keypoint", type=int, default=NUM_STEPS_PER_KEYPOINT)
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    args = ap.parse_args(argv)
    params = dict(PARAMS, dtype=args.dtype)
    if args.model_dir:
        params["model_dir"] = args.model_dir
    if args.batch:
        params["batch_size"] = args.batch
    if args.train_dataset:
        params["train_dataset"] = args.train_dataset
    if args.val_dataset:
        params["val_dataset"] = args.val_dataset
    train_files, val_files = dataset_files(params["train_dataset"]), dataset_files(params["val_dataset"])
    if not train_files:
        raise SystemExit(f"no TFRecord files under {params['train_dataset']!r}: pass --train-dataset DIR "
                         "(tools/make_toy_tfrecords.py writes a small one)")
    from .detector.input_pipeline import AnnotationCache, PoseResidualNetworkPipeline
    train_cache, val_cache = AnnotationCache(), AnnotationCache()
    batch = params["batch_size"]

    def train_batches(max_keypoints):   # train_prn.py:23-34 get_input_fn(is_training=True, max_keypoints)
        return PoseResidualNetworkPipeline(train_files, True, batch, max_keypoints, annotations=train_cache).batches()

    def val_batches():
        return PoseResidualNetworkPipeline(val_files, False, batch, annotations=val_cache).batches()
    val = val_batches if val_files else None
    step = train(params, train_batches, val_batches=val, max_steps=args.steps, steps_per_keypoint=args.steps_per_keypoint)
    if val is not None:
        evaluate(params, val, step=step)


if __name__ == "__main__":
    main()
