"""Average precision of the person detector at one IoU threshold, PASCAL VOC style - a host port of the reference's
`metrics.py` (:15-254). Evaluation sees one image at a time and at most `max_boxes` detections per image, so this is plain
Python on the host, with the reference's operations in the reference's order (its numbers are reproduced to the last bits,
tests/test_metrics_oracle.py):

  * all detections sorted by confidence, highest first, ties in the order they were added (`list.sort` is stable);
  * each detection goes to the ground-truth box of its image with the largest IoU (the first one on ties; IoU must be
    > 0), and is a true positive if that IoU >= iou_threshold and the box is not taken yet - else a false positive;
  * precision[k] = TP / (k + 1), recall[k] = TP / max(number of ground-truth boxes, 1);
  * AP = sum_k precision[k] * (recall[k] - recall[k-1]) (no interpolation);
  * the best threshold is the confidence at argmax_k of p * r * (1 - |p - r|).

Coordinates keep the dtype they arrive in (float32 from the detector): the IoU is computed in it and divided in float64.

    evaluator = Evaluator()
    for features, labels in pipeline:                       # evaluation batches of one image
        spec = model_fn(features, labels, ModeKeys.EVAL, params)
        evaluator.update(labels, spec.eval_metric_ops)      # the EVAL spec's predictions
    metrics = evaluator.evaluate()                          # the seven values
    evaluator.initialize()                                  # before the next evaluation
"""
import numpy as np

METRIC_NAMES = ("AP", "precision", "recall", "mean_iou_for_TP", "best_threshold", "total_FP", "total_FN")


def compute_iou(a, b):
    """IoU of two boxes (ymin, xmin, ymax, xmax); 0.0 unless they overlap with positive width and height."""
    w = min(a[3], b[3]) - max(a[1], b[1])
    if not w > 0:
        return 0.0
    h = min(a[2], b[2]) - max(a[0], b[0])
    if not h > 0:
        return 0.0
    intersection = w * h
    union = ((a[3] - a[1]) * (a[2] - a[0]) + (b[3] - b[1]) * (b[2] - b[0])) - intersection
    return float(intersection) / float(union)


def match(box, groundtruth_boxes):
    """(index of the ground-truth box with the largest IoU or -1, that IoU)."""
    best_i, max_iou = -1, 0.0
    for i, g in enumerate(groundtruth_boxes):
        iou = compute_iou(box, g)
        if iou > max_iou:
            best_i, max_iou = i, iou
    return best_i, max_iou


def compute_ap(precision, recall):
    ap, previous = 0.0, 0.0
    for p, r in zip(precision, recall):
        ap += p * (r - previous)
        previous = r
    return ap


def compute_best_threshold(precision, recall, confidences):
    """(confidence, precision, recall) where p * r * (1 - |p - r|) is largest (the first such place)."""
    if len(confidences) == 0:
        return 0.0, 0.0, 0.0
    p, r = np.array(precision), np.array(recall)
    i = int(np.argmax((p * r) * (1.0 - np.abs(p - r))))
    return confidences[i], p[i], r[i]


def evaluate_detector(groundtruth, detections, iou_threshold=0.5):
    """groundtruth: {image name: boxes [n,4]}; detections: a sequence of (image name, box [4], confidence).
    Returns the dict of the seven METRIC_NAMES. Neither argument is modified."""
    groundtruth = {name: [np.asarray(b) for b in boxes] for name, boxes in groundtruth.items()}
    num_groundtruth = max(sum(len(b) for b in groundtruth.values()), 1)
    taken = {name: [False] * len(b) for name, b in groundtruth.items()}
    detections = sorted(detections, key=lambda d: d[2], reverse=True)

    tp, iou_sum = 0, 0.0
    precision, recall = [0.0] * len(detections), [0.0] * len(detections)
    for k, (name, box, _) in enumerate(detections):
        i, iou = match(box, groundtruth.get(name, []))
        if i >= 0 and iou >= iou_threshold and not taken[name][i]:
            taken[name][i] = True
            tp += 1
            iou_sum += iou
        precision[k] = tp / (k + 1)
        recall[k] = tp / num_groundtruth
    best_threshold, best_precision, best_recall = compute_best_threshold(precision, recall, [d[2] for d in detections])
    return {"AP": compute_ap(precision, recall), "precision": float(best_precision), "recall": float(best_recall),
            "mean_iou_for_TP": iou_sum / max(tp, 1), "best_threshold": float(best_threshold),
            "total_FP": len(detections) - tp, "total_FN": num_groundtruth - tp}


class Evaluator:
    """Collects ground truth and detections image by image; `evaluate()` scores them."""

    def __init__(self):
        self.initialize()

    def initialize(self):
        self.detections = []
        self.groundtruth = {}          # image name -> list of boxes
        self.unique_image_id = 0
        self.metrics = None

    def add_groundtruth(self, image_name, boxes):
        for box in boxes:
            self.groundtruth.setdefault(image_name, []).append(np.asarray(box))

    def add_detections(self, image_name, boxes, scores):
        for box, score in zip(boxes, scores):
            self.detections.append((image_name, np.asarray(box), score))

    def update(self, labels, predictions):
        """One evaluated image: labels {'boxes': [1,N,4], 'num_boxes': [1]} of the pipeline and the EVAL spec's
        predictions {'boxes': [1,M,4], 'scores': [1,M], 'num_boxes': [1]} (device tensors or arrays). Rows beyond either
        `num_boxes` are padding. One device -> host copy."""
        import torch
        gt, pb, ps = labels["boxes"], predictions["boxes"], predictions["scores"]
        if torch.is_tensor(pb):
            n, m = gt.shape[1], pb.shape[1]
            counts = torch.stack([torch.as_tensor(labels["num_boxes"]).reshape(-1)[0].to(pb.device),
                                  torch.as_tensor(predictions["num_boxes"]).reshape(-1)[0].to(pb.device)])
            flat = torch.cat([torch.as_tensor(gt).to(pb.device, torch.float32)[0].reshape(-1), pb[0].reshape(-1),
                              ps[0].reshape(-1), counts.to(torch.float32)]).cpu().numpy()
            gt, pb, ps = flat[:n * 4].reshape(n, 4), flat[n * 4:(n + m) * 4].reshape(m, 4), flat[(n + m) * 4:(n + m) * 4 + m]
            num_gt, num_pred = int(flat[-2]), int(flat[-1])
        else:
            gt, pb, ps = np.asarray(gt)[0], np.asarray(pb)[0], np.asarray(ps)[0]
            num_gt, num_pred = int(np.asarray(labels["num_boxes"]).reshape(-1)[0]), int(np.asarray(predictions["num_boxes"]).reshape(-1)[0])
        name = str(self.unique_image_id)
        self.unique_image_id += 1
        self.add_groundtruth(name, gt[:num_gt])
        self.add_detections(name, pb[:num_pred], ps[:num_pred])

    def evaluate(self, iou_threshold=0.5):
        """Scores what was collected; returns (and keeps in `self.metrics`) the seven values. Nothing is forgotten:
        `initialize()` starts the next evaluation."""
        self.metrics = evaluate_detector(self.groundtruth, self.detections, iou_threshold)
        return self.metrics
