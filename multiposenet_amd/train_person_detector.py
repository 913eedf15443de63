"""Runnable replacement of the reference's `train_person_detector.py` (:7-71): PARAMS, warm start of `MobilenetV1/*`, the
tf.estimator train loop with its cadence (summaries every `save_summary_steps`, a checkpoint every `save_checkpoints_secs`,
steps/sec log every `log_step_count_steps`, evaluation every `throttle_secs`), resume from the newest checkpoint in
`model_dir` - on `person_detector_model.model_fn` (the HIP kernels) fed by `DetectorPipeline`.

    python -m multiposenet_amd.train_person_detector --train-dataset DIR --val-dataset DIR [--pretrained-checkpoint NPZ]
                                                     [--model-dir DIR] [--steps N] [--batch B] [--image-size W H]
                                                     [--dtype bf16|f32] [--eval-every SECONDS]

Data: the TFRecord shards (`*.tfrecords`, else every file) of the reference's data/create_tfrecords.py
(tools/make_toy_tfrecords.py writes small ones of the same contract; only `image`, `num_persons` and `boxes` are read).
`train()` takes any iterator of (features, labels) in the pipeline's output contract, or a callable returning one.
Evaluation (person_detector_model.py:49-71) runs `model_fn` in EVAL mode image by image, feeds the predictions to
`metrics.Evaluator` and reports the means of the four losses and the seven metrics under the reference's names
(`metrics/AP`, ...). Checkpoints are `model.ckpt-<step>.npz` (multiposenet_amd.checkpoint): the head's variables, moving
statistics and Adam slots, `global_step`, and the frozen backbone's `MobilenetV1/*` variables and statistics, so a run
resumes from model_dir alone.
"""
import argparse
import json
import os
import time

import torch

from . import checkpoint
from .keypoints_model import ModeKeys
from .metrics import METRIC_NAMES, Evaluator
from .person_detector_model import get_detector, model_fn
from .train_keypoints import dataset_files, latest_checkpoint

PARAMS = {   # train_person_detector.py:7-29
    'model_dir': 'models/run01/',
    'train_dataset': '/home/dan/datasets/COCO/multiposenet/train/',
    'val_dataset': '/home/dan/datasets/COCO/multiposenet/val/',
    'pretrained_checkpoint': 'models/run00/model.ckpt-200000.npz',   # the keypoint run's checkpoint (train_keypoints)

    'backbone': 'mobilenet',
    'depth_multiplier': 1.0,
    'weight_decay': 5e-5,

    'score_threshold': 0.3, 'iou_threshold': 0.6, 'max_boxes': 25,
    'localization_loss_weight': 1.0, 'classification_loss_weight': 2.0,

    'gamma': 2.0,
    'alpha': 0.25,

    'num_steps': 150000,
    'initial_learning_rate': 1e-3,

    'min_dimension': 640,
    'batch_size': 16,
    'image_size': (640, 640),
}
RUN_CONFIG = {'save_summary_steps': 200, 'save_checkpoints_secs': 1800, 'log_step_count_steps': 1000,   # :52-57
              'eval_start_delay_secs': 7200, 'eval_throttle_secs': 7200}                                 # :69


BACKBONE_SCOPE = "MobilenetV1/"


class _DetectorState:
    """The detector's trained head and its frozen backbone under one name space, as the estimator's checkpoint holds them:
    what multiposenet_amd.checkpoint reads and writes. The Adam slots, `global_step` and everything else are the head's (the
    backbone has no optimizer state here, person_detector_model.py:14-17)."""

    def __init__(self, net):
        self.head, self.backbone = net, net.backbone

    def __getattr__(self, name):
        return getattr(self.head, name)

    def _backbone_names(self):
        b = self.backbone
        return [k for k in list(b.vars) + list(b.stats) if k.startswith(BACKBONE_SCOPE)]

    @property
    def vars(self):
        return {**{k: None for k in self._backbone_names()}, **self.head.vars}

    @property
    def stats(self):
        return self.head.stats

    def state_dict(self):
        out = {k: v for k, v in self.backbone.state_dict().items() if k.startswith(BACKBONE_SCOPE)}
        out.update(self.head.state_dict())
        return out

    def load_state_dict(self, values, strict=False):
        self.backbone.load_state_dict({k: v for k, v in values.items() if k.startswith(BACKBONE_SCOPE)}, strict=False)
        self.head.load_state_dict({k: v for k, v in values.items() if not k.startswith(BACKBONE_SCOPE)}, strict=False)


def _open(batches):
    return iter(batches() if callable(batches) else batches)


def train(params, train_batches, val_batches=None, run_config=None, max_steps=None, log=print):
    """tf.estimator.train_and_evaluate for the person detector. train_batches / val_batches: iterators (or callables
    returning iterators) of (features, labels). Returns the global step reached."""
    cfg = dict(RUN_CONFIG, **(run_config or {}))
    params = dict(params)
    net = _DetectorState(get_detector(params))
    model_dir = params["model_dir"]
    os.makedirs(model_dir, exist_ok=True)
    last = latest_checkpoint(model_dir)
    if last is not None:                     # the estimator resumes from model_dir before it looks at warm_start_from
        checkpoint.load_npz(last[1], net)
        log(f"[train] restored {last[1]} (global_step {int(net.global_step.item())})")
    elif params.get("pretrained_checkpoint") and os.path.exists(params["pretrained_checkpoint"]):
        names = checkpoint.warm_start(params["pretrained_checkpoint"], net, scopes=("MobilenetV1/",))   # :64
        log(f"[train] warm start: {len(names)} variables from {params['pretrained_checkpoint']}")
    max_steps = int(max_steps if max_steps is not None else params["num_steps"])
    it = _open(train_batches)
    step = int(net.global_step.item())
    t_ckpt = t_log = t_start = time.time()
    t_eval = t_start + cfg["eval_start_delay_secs"] - cfg["eval_throttle_secs"]
    step_log = step
    summaries = os.path.join(model_dir, "summaries.jsonl")

    def save():
        path = os.path.join(model_dir, f"model.ckpt-{step}.npz")
        checkpoint.save_npz(path, net)
        log(f"[train] saved {path}")
    while step < max_steps:
        features, labels = next(it)
        spec = model_fn(features, labels, ModeKeys.TRAIN, params)
        step += 1
        if step % cfg["save_summary_steps"] == 0:
            with open(summaries, "a") as f:
                f.write(json.dumps({"step": step, **{k: float(v) for k, v in spec.losses.items()}}) + "\n")
        if step % cfg["log_step_count_steps"] == 0:
            torch.cuda.synchronize()
            now = time.time()
            log(f"[train] step {step}: loss {float(spec.loss):.4f}, {(step - step_log) / (now - t_log):.2f} steps/s")
            t_log, step_log = now, step
        now = time.time()
        if now - t_ckpt >= cfg["save_checkpoints_secs"]:
            save()
            t_ckpt = now
        if val_batches is not None and now - t_eval >= cfg["eval_throttle_secs"]:
            evaluate(params, val_batches, log=log, step=step)
            t_eval = now
    last = latest_checkpoint(model_dir)
    if last is None or last[0] != step:
        save()
    return step


def evaluate(params, val_batches, log=print, step=None):
    """EvalSpec(steps=None): one pass over the validation images (batches of one). Returns the means of the losses
    (person_detector_model.py:60-66) and the seven `metrics/<name>` of metrics.Evaluator at IoU 0.5."""
    evaluator = Evaluator()
    sums, n = None, 0
    for features, labels in _open(val_batches):
        spec = model_fn(features, labels, ModeKeys.EVAL, params)
        evaluator.update(labels, spec.eval_metric_ops)          # (the EVAL spec carries the predictions there)
        losses = torch.stack([spec.losses[k].reshape(()) for k in sorted(spec.losses)]).to(torch.float64)
        sums = losses if sums is None else sums + losses
        n += 1
    out = {}
    if n:
        out = dict(zip(sorted(spec.losses), (sums / n).tolist()))
    out.update({"metrics/" + k: v for k, v in evaluator.evaluate().items()})
    assert set(METRIC_NAMES) == {k[8:] for k in out if k.startswith("metrics/")}
    log(f"[eval] step {step}: " + ", ".join(f"{k} {v:.5f}" for k, v in sorted(out.items())) + f" over {n} images")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-dataset", default=None, help="directory of training TFRecords (default: PARAMS)")
    ap.add_argument("--val-dataset", default=None, help="directory of evaluation TFRecords (default: PARAMS)")
    ap.add_argument("--pretrained-checkpoint", default=None, help=".npz whose MobilenetV1/* variables warm-start the backbone")
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--image-size", type=int, nargs=2, metavar=("WIDTH", "HEIGHT"), default=None)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--decode", default="host", choices=["host", "device"],
                    help="where the pixel half of the JPEG decode runs (device: Huffman on the host, inverse DCT and colour in HIP)")
    ap.add_argument("--entropy", default="host", choices=["host", "device"],
                    help="with --decode device: where the Huffman decode runs (device: only the file's bytes cross the link)")
    ap.add_argument("--eval-every", type=float, default=None, help="seconds between evaluations (default: 7200)")
    args = ap.parse_args(argv)
    params = dict(PARAMS, dtype=args.dtype)
    for key, value in (("model_dir", args.model_dir), ("batch_size", args.batch), ("train_dataset", args.train_dataset),
                       ("val_dataset", args.val_dataset), ("pretrained_checkpoint", args.pretrained_checkpoint),
                       ("image_size", tuple(args.image_size) if args.image_size else None)):
        if value:
            params[key] = value
    train_files, val_files = dataset_files(params["train_dataset"]), dataset_files(params["val_dataset"])
    if not train_files:
        raise SystemExit(f"no TFRecord files under {params['train_dataset']!r}: pass --train-dataset DIR "
                         "(tools/make_toy_tfrecords.py writes a small one)")
    from .detector.input_pipeline import DetectorPipeline
    run_config = {}
    if args.eval_every is not None:
        run_config = {"eval_start_delay_secs": args.eval_every, "eval_throttle_secs": args.eval_every}
    val = (lambda: DetectorPipeline(val_files, False, params, decode=args.decode, entropy=args.entropy).batches()) if val_files else None
    step = train(params, lambda: DetectorPipeline(train_files, True, params, decode=args.decode, entropy=args.entropy).batches(), val_batches=val,
                 run_config=run_config, max_steps=args.steps)
    if val is not None:
        evaluate(params, val, step=step)


if __name__ == "__main__":
    main()
