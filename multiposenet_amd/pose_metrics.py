"""COCO keypoint AP: average precision and recall over object keypoint similarity (OKS), the metric of the COCO keypoint
challenge, for the persons `Detector.predict_*` returns. The reference publishes no such number; the algorithm is
pycocotools' COCOeval for iouType='keypoints' (cocoeval.py: computeOks, evaluateImg, accumulate, summarize).

The per-image part - OKS of every detection against every ground truth and the greedy matching at 10 thresholds x 3 area
ranges - runs on the device (`mpn_oks_match`, include/mpn.h): inside the Detector's captured graph when `predict_*` is given
`groundtruth=`, or through `OksMatcher` for host arrays. `PoseEvaluator` collects the small per-detection results and does
COCOeval's accumulate and summarize once per evaluation, on the host in numpy.

    evaluator = PoseEvaluator()
    for images, groundtruth in batches:                         # groundtruth: a list of dicts, see `groundtruth_arrays`
        evaluator.update(detector.predict_images(images, groundtruth=groundtruth), groundtruth)
    stats = evaluator.evaluate()                                # AP, AP50, AP75, APM, APL, AR, AR50, AR75, ARM, ARL

Deviations from the official number, all on the data side: detections are float32 (COCO's result files round to two decimals
anyway); an image may hold at most 64 ground-truth persons (more raises); ground truth made from TFRecords
(`groundtruth_from_record`) has the box area in place of the segment area and lacks the persons create_tfrecords.py dropped.
"""
import json

import numpy as np

from . import _lib

# cocoeval.py, Params.setKpParams
KEYPOINT_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
OKS_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
AREA_RANGES = (('all', 0.0, 1e10), ('medium', 32.0 ** 2, 96.0 ** 2), ('large', 96.0 ** 2, 1e10))
MAX_DETS = 20
MAX_GT = 64                            # ground-truth persons per image the kernel takes (a 64-bit matched set per lane)
NUM_KEYPOINTS = 17
STAT_NAMES = ('AP', 'AP50', 'AP75', 'APM', 'APL', 'AR', 'AR50', 'AR75', 'ARM', 'ARL')
SCORE_MODES = {'box': 0, 'box*keypoints': 1}

GT_DOUBLES = 64                        # a ground-truth row (checked against the library)
# a row of mpn_oks_match's output (include/mpn.h)
_OUT = np.dtype([('rank', np.int32), ('score', np.float32), ('area', np.float64), ('match', np.int32, (3, 10)),
                 ('ignore', np.uint32, (3,)), ('pad', np.uint32)])


def groundtruth_arrays(gt):
    """A ground-truth dict -> (keypoints f64 [g,17,3], boxes f64 [g,4], area f64 [g], iscrowd bool [g], ignore bool [g]).

    'keypoints': [g,17,3] (x, y, v); 'boxes': [g,4] (x, y, w, h), both in the pixels of the detections' 'keypoints';
    'area': optional [g], default w * h; 'iscrowd': optional [g], default 0. ignore = iscrowd | (no keypoint with v > 0),
    as COCOeval._prepare sets it."""
    kp = np.asarray(gt['keypoints'], np.float64).reshape(-1, NUM_KEYPOINTS, 3)
    g = len(kp)
    boxes = np.asarray(gt['boxes'], np.float64).reshape(-1, 4)
    if len(boxes) != g:
        raise ValueError(f"groundtruth: {g} keypoint sets and {len(boxes)} boxes")
    area = gt.get('area')
    area = boxes[:, 2] * boxes[:, 3] if area is None else np.asarray(area, np.float64).reshape(-1)
    crowd = gt.get('iscrowd')
    crowd = np.zeros(g, bool) if crowd is None else np.asarray(crowd).reshape(-1) != 0
    if len(area) != g or len(crowd) != g:
        raise ValueError(f"groundtruth: {g} persons, {len(area)} areas, {len(crowd)} iscrowd flags")
    ignore = crowd | ~(kp[:, :, 2] > 0).any(axis=1)
    return kp, boxes, area, crowd, ignore


def groundtruth_from_record(example):
    """What input_pipeline/tfrecord.py's `decode_keypoint_example` parses -> a ground-truth dict in the image's pixels:
    keypoints (y, x, v) -> (x, y, v), boxes (ymin, xmin, ymax, xmax) -> (x, y, w, h).

    The records hold neither COCO's segment areas nor the persons data/create_tfrecords.py dropped as poorly annotated:
    'area' is the BOX area (larger than a segment's, so OKS is a little more lenient and the medium / large split moves) and a
    detection on a dropped person counts as a false positive. AP from records is a consistent yardstick between runs of
    this project, not the official number; `groundtruth_from_coco` gives that."""
    kp = np.asarray(example['keypoints'], np.float64).reshape(-1, NUM_KEYPOINTS, 3)
    b = np.asarray(example['boxes'], np.float64).reshape(-1, 4)
    boxes = np.stack([b[:, 1], b[:, 0], b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]], axis=1)
    return {'keypoints': kp[:, :, [1, 0, 2]].copy(), 'boxes': boxes, 'area': boxes[:, 2] * boxes[:, 3],
            'iscrowd': np.zeros(len(kp), np.int32)}


def groundtruth_from_coco(json_path):
    """person_keypoints_*.json -> {image_id: (file_name, groundtruth)} for every image of the file (plain `json`), with
    COCO's own 'area' and 'iscrowd'; an annotation with num_keypoints == 0 has no v > 0 and so is ignored."""
    with open(json_path) as f:
        data = json.load(f)
    per_image = {im['id']: [] for im in data['images']}
    for ann in data.get('annotations', []):
        if 'keypoints' in ann and ann['image_id'] in per_image:
            per_image[ann['image_id']].append(ann)
    out = {}
    for im in data['images']:
        anns = per_image[im['id']]
        gt = {'keypoints': np.array([a['keypoints'] for a in anns], np.float64).reshape(-1, NUM_KEYPOINTS, 3),
              'boxes': np.array([a['bbox'] for a in anns], np.float64).reshape(-1, 4),
              'area': np.array([a['area'] for a in anns], np.float64),
              'iscrowd': np.array([a.get('iscrowd', 0) for a in anns], np.int32)}
        out[im['id']] = (im['file_name'], gt)
    return out


def check_max_gt(max_gt):
    if not 1 <= int(max_gt) <= MAX_GT:
        raise ValueError(f"max_gt must be in 1..{MAX_GT} (got {max_gt}): mpn_oks_match keeps a matched set in one 64-bit mask")
    return int(max_gt)


def pack_groundtruth(groundtruth, rows, counts):
    """b ground-truth dicts -> rows f64 [b, max_gt, 64] and counts int32 [b] (both written in place), mpn_oks_match's layout."""
    b, max_gt, _ = rows.shape
    if len(groundtruth) != b:
        raise ValueError(f"groundtruth must be a list of {b} dicts, one per image (got {len(groundtruth)})")
    rows[...] = 0.0
    for i, gt in enumerate(groundtruth):
        kp, boxes, area, crowd, ignore = groundtruth_arrays(gt)
        g = len(kp)
        if g > max_gt:
            raise ValueError(f"groundtruth: image {i} has {g} persons, mpn_oks_match takes {max_gt}")
        rows[i, :g, :51] = kp.reshape(g, 51)
        rows[i, :g, 51:55] = boxes
        rows[i, :g, 55], rows[i, :g, 56], rows[i, :g, 57] = area, ignore, crowd
        counts[i] = g


def fill_record(outputs, b, max_boxes):
    """b result dicts ('scores' and, where present, 'boxes', 'keypoint_scores', 'keypoint_positions', 'keypoints' as
    `Detector.predict_batch` returns them) -> (record uint8 [record_bytes], counts int32 [b]) on the host: a record of
    mpn_pose_gather's layout for (b, max_boxes), what `OksMatcher` and `tracking.PoseTracker.update` upload."""
    from .inference.detector import _ROW
    lib = _lib.lib()
    record_bytes, first = lib.mpn_pose_gather_record_bytes(b, max_boxes), lib.mpn_pose_gather_row_offset(b, max_boxes, 0)
    if len(outputs) != b:
        raise ValueError(f"outputs must be a list of {b} dicts (got {len(outputs)})")
    if _ROW.itemsize != lib.mpn_pose_gather_row_offset(b, max_boxes, 1) - first:
        raise _lib.MpnError("mpn_pose_gather: the record's layout is not the one this binding was written against")
    record = np.zeros(record_bytes, np.uint8)
    header = record[:first].view(np.int32)
    rows = record[first:].view(_ROW)
    s = 0
    for i, o in enumerate(outputs):
        n = len(o['scores'])
        if n > max_boxes:
            raise ValueError(f"outputs: image {i} has {n} detections, this matcher takes {max_boxes}")
        r = rows[s:s + n]
        r['image_index'], r['score'] = i, o['scores']
        for k in ('keypoint_scores', 'keypoint_positions', 'keypoints'):
            if k in o and len(o[k]) == n:
                r[k] = o[k]
        if 'boxes' in o and len(o['boxes']) == n:
            r['box'] = o['boxes']
        header[1 + i] = n
        header[1 + b + i] = int(o.get('num_boxes', n))
        s += n
    header[0] = s
    return record, header[1:1 + b].copy()


class OksBuffers:
    """The device side of `mpn_oks_match` for one (b, max_boxes, max_gt): a pinned staging buffer and its device twin holding
    the thresholds, the ground-truth rows and their counts (`place`: one host-to-device copy), and the launch over a record
    on the device (the grid depends on b alone: it can be captured, and the graph follows whatever `place` uploads later)."""

    def __init__(self, b, max_boxes, max_gt=MAX_GT, device=None, score='box', max_dets=MAX_DETS):
        self.max_gt = check_max_gt(max_gt)
        if score not in SCORE_MODES:
            raise ValueError(f"score must be one of {sorted(SCORE_MODES)} (got {score!r})")
        import torch
        lib = _lib.lib()
        if lib.mpn_oks_gt_row_bytes() != GT_DOUBLES * 8:
            raise _lib.MpnError("mpn_oks_match: the ground-truth row is not the one this binding was written against")
        self.b, self.max_boxes, self.score_mode, self.max_dets = int(b), int(max_boxes), SCORE_MODES[score], int(max_dets)
        self.out_bytes = lib.mpn_oks_match_out_bytes(self.b, self.max_boxes)
        if self.out_bytes == 0 or self.out_bytes != self.b * self.max_boxes * _OUT.itemsize:
            raise ValueError(f"mpn_oks_match: {self.b} x {self.max_boxes} slots are more than one launch takes")
        self.device = torch.device(device) if device is not None else _lib.current_device()
        t = len(OKS_THRESHOLDS)
        words = t + self.b * self.max_gt * GT_DOUBLES + (self.b + 1) // 2              # in doubles
        self.stage = torch.zeros(words, dtype=torch.float64).pin_memory()
        self.dev = torch.zeros(words, dtype=torch.float64, device=self.device)
        host = self.stage.numpy()
        host[:t] = OKS_THRESHOLDS
        self._rows = host[t:t + self.b * self.max_gt * GT_DOUBLES].reshape(self.b, self.max_gt, GT_DOUBLES)
        self._counts = host[t + self._rows.size:].view(np.int32)[:self.b]
        self._at = (0, t, t + self._rows.size)                                          # thresholds, rows, counts

    def place(self, groundtruth):
        """This call's ground truth goes to the device: one small pinned copy on the current stream."""
        pack_groundtruth(groundtruth, self._rows, self._counts)
        self.dev.copy_(self.stage, non_blocking=True)

    def device_groundtruth(self):
        """The device tensors `place` fills: (rows f64 [b, max_gt, 64] flat, counts int32 [b] as the words behind them) - what
        mpn_track_eval reads beside mpn_oks_match."""
        return self.dev[self._at[1]:], self.dev[self._at[2]:]

    def launch(self, record, out, oks_out=None):
        """record: the uint8 device tensor mpn_pose_gather wrote; out: uint8 device tensor of `out_bytes`; oks_out: float64
        device tensor [b * max_boxes, max_gt] or None."""
        thr, rows, counts = (self.dev[at:] for at in self._at)
        _lib.call("mpn_oks_match", _lib.ptr(record), self.b, self.max_boxes, _lib.ptr(rows), _lib.ptr(counts), self.max_gt,
                  _lib.ptr(thr), len(OKS_THRESHOLDS), self.score_mode, self.max_dets, _lib.ptr(out), _lib.ptr(oks_out),
                  _lib.stream_ptr())
        return out

    def unpack(self, out, counts, oks=None):
        """A host copy of the output rows (uint8 array) and the record's per-image counts -> a list of b dicts:
        'rank' int32 [n], 'score' f32 [n], 'area' f64 [n], 'matches' int32 [n,3,10], 'ignore' bool [n,3,10] in the image's
        record order, 'score_mode', 'max_dets' (and 'oks' f64 [n, max_gt] from `oks`)."""
        rows = np.frombuffer(out, np.uint8, self.out_bytes).view(_OUT)
        bits = np.arange(len(OKS_THRESHOLDS), dtype=np.uint32)
        res, s = [], 0
        for i in range(self.b):
            e = s + int(counts[i])
            r = rows[s:e]
            d = {'rank': r['rank'].copy(), 'score': r['score'].copy(), 'area': r['area'].copy(), 'matches': r['match'].copy(),
                 'ignore': ((r['ignore'][:, :, None] >> bits) & 1).astype(bool), 'score_mode': self.score_mode,
                 'max_dets': self.max_dets}
            if oks is not None:
                d['oks'] = oks[s:e].copy()
            res.append(d)
            s = e
        return res


class OksMatcher:
    """`mpn_oks_match` for host arrays: fills a record of mpn_pose_gather's layout from b result dicts ('scores',
    'keypoint_scores', 'keypoints' as `Detector.predict_batch` returns them), uploads it with the ground truth, runs the
    kernel and returns, per image, {'rank', 'score', 'area', 'matches' [n,3,10], 'ignore' [n,3,10]} (+ 'oks' [n, max_gt] with
    return_oks=True). An image may have at most max_boxes detections and max_gt ground-truth persons."""

    def __init__(self, b, max_boxes, max_gt=MAX_GT, device=None, score='box', max_dets=MAX_DETS):
        check_max_gt(max_gt)
        import torch
        self.buffers = OksBuffers(b, max_boxes, max_gt, device, score, max_dets)
        lib = _lib.lib()
        self.b, self.max_boxes = int(b), int(max_boxes)
        self.record_bytes = lib.mpn_pose_gather_record_bytes(self.b, self.max_boxes)
        self.first = lib.mpn_pose_gather_row_offset(self.b, self.max_boxes, 0)
        dev = self.buffers.device
        self.record = torch.zeros(self.record_bytes, dtype=torch.uint8, device=dev)
        self.out = torch.zeros(self.buffers.out_bytes, dtype=torch.uint8, device=dev)
        self.oks = torch.zeros((self.b * self.max_boxes, self.buffers.max_gt), dtype=torch.float64, device=dev)

    def fill_record(self, outputs):
        """b result dicts -> (record uint8 [record_bytes], counts int32 [b]) on the host."""
        return fill_record(outputs, self.b, self.max_boxes)

    def __call__(self, outputs, groundtruth, return_oks=False):
        import torch
        record, counts = self.fill_record(outputs)
        with torch.cuda.device(self.buffers.device):
            self.buffers.place(groundtruth)
            self.record.copy_(torch.from_numpy(record))
            self.buffers.launch(self.record, self.out, self.oks if return_oks else None)
            out = self.out.cpu().numpy()
            oks = self.oks.cpu().numpy() if return_oks else None
        return self.buffers.unpack(out, counts, oks)


class PoseEvaluator:
    """Collects per-image match tables; `evaluate()` is COCOeval's accumulate + summarize. Mirrors `metrics.Evaluator`.

    score: 'box' ranks detections by the person detector's score, 'box*keypoints' by that times the mean keypoint score.
    max_dets: detections evaluated per image (COCO's keypoint evaluation uses 20)."""

    def __init__(self, score='box', max_dets=MAX_DETS, max_gt=MAX_GT):
        if score not in SCORE_MODES:
            raise ValueError(f"score must be one of {sorted(SCORE_MODES)} (got {score!r})")
        self.score, self.max_dets, self.max_gt = score, int(max_dets), check_max_gt(max_gt)
        self._matchers = {}
        self.initialize()

    def initialize(self):
        self.scores, self.matched, self.ignored = [], [], []       # per image, in rank order
        self.num_groundtruth = np.zeros(len(AREA_RANGES), np.int64)    # not ignored, per range
        self.num_images = 0
        self.stats = None

    def _match(self, outputs, groundtruth):
        b = len(outputs)
        most = max([len(o['scores']) for o in outputs] + [1])
        max_boxes = 32
        while max_boxes < most:
            max_boxes *= 2
        key = (b, max_boxes)
        if key not in self._matchers:
            self._matchers[key] = OksMatcher(b, max_boxes, self.max_gt, None, self.score, self.max_dets)
        return self._matchers[key](outputs, groundtruth)

    def update(self, outputs, groundtruth):
        """outputs: the list of b result dicts of a `Detector.predict_*` call; groundtruth: the b ground-truth dicts. An
        output's 'oks' entry (made inside the Detector's graph when the call was given `groundtruth=`) is used as it is;
        without it the batch goes through `OksMatcher`."""
        outputs, groundtruth = list(outputs), list(groundtruth)
        if len(outputs) != len(groundtruth):
            raise ValueError(f"{len(outputs)} outputs and {len(groundtruth)} ground-truth dicts")
        if all('oks' in o for o in outputs):
            tables = [o['oks'] for o in outputs]
        else:
            tables = self._match(outputs, groundtruth)
        for t, gt in zip(tables, groundtruth):
            if t['score_mode'] != SCORE_MODES[self.score] or t['max_dets'] != self.max_dets:
                raise ValueError("the 'oks' entry was made with another score mode or max_dets than this evaluator's")
            self.add_image(t, gt)

    def add_image(self, table, gt):
        """One image's match table ('rank', 'score', 'matches', 'ignore') and its ground truth."""
        _, _, area, _, ignore = groundtruth_arrays(gt)
        for r, (_, lo, hi) in enumerate(AREA_RANGES):
            self.num_groundtruth[r] += int(np.count_nonzero(~(ignore | (area < lo) | (area > hi))))
        rank = np.asarray(table['rank'])
        sel = np.nonzero(rank < self.max_dets)[0]
        sel = sel[np.argsort(rank[sel], kind='mergesort')]
        self.scores.append(np.asarray(table['score'])[sel])
        self.matched.append(np.asarray(table['matches'])[sel] >= 0)
        self.ignored.append(np.asarray(table['ignore'])[sel].astype(bool))
        self.num_images += 1

    def evaluate(self):
        """The ten numbers of COCO's keypoint summary as a dict (kept in `self.stats`); -1 where a range has no ground truth."""
        nt, nr = len(OKS_THRESHOLDS), len(AREA_RANGES)
        if self.scores:
            scores, matched, ignored = np.concatenate(self.scores), np.concatenate(self.matched), np.concatenate(self.ignored)
        else:
            scores, matched, ignored = np.zeros(0, np.float32), np.zeros((0, nr, nt), bool), np.zeros((0, nr, nt), bool)
        precision, recall = evaluate_tables(scores, matched, ignored, self.num_groundtruth)
        self.stats = summarize(precision, recall)
        return self.stats


def evaluate_tables(scores, matched, ignored, num_groundtruth):
    """COCOeval.accumulate for one category and one max_dets: scores [n] in image order and, per image, rank order;
    matched, ignored bool [n, 3, T]; num_groundtruth [3] not-ignored counts -> precision [T, 101, 3], recall [T, 3]."""
    nt, nr, nrec = len(OKS_THRESHOLDS), len(AREA_RANGES), len(RECALL_THRESHOLDS)
    precision, recall = -np.ones((nt, nrec, nr)), -np.ones((nt, nr))
    order = np.argsort(-np.asarray(scores), kind='mergesort')
    matched, ignored = np.asarray(matched, bool)[order], np.asarray(ignored, bool)[order]
    eps = np.spacing(1)
    for r in range(nr):
        npig = int(num_groundtruth[r])
        if npig == 0:
            continue
        tp = np.cumsum(matched[:, r] & ~ignored[:, r], axis=0).astype(np.float64)           # [n, T]
        fp = np.cumsum(~matched[:, r] & ~ignored[:, r], axis=0).astype(np.float64)
        for t in range(nt):
            rc = tp[:, t] / npig
            pr = tp[:, t] / (fp[:, t] + tp[:, t] + eps)
            recall[t, r] = rc[-1] if len(rc) else 0.0
            q = np.zeros(nrec)
            if len(pr):
                pr = np.maximum.accumulate(pr[::-1])[::-1]                                  # the right-to-left envelope
                at = np.searchsorted(rc, RECALL_THRESHOLDS, side='left')
                ok = at < len(pr)
                q[ok] = pr[at[ok]]
            precision[t, :, r] = q
    return precision, recall


def summarize(precision, recall):
    """COCOeval.summarize's keypoint rows: means over the entries > -1, or -1 when there are none."""
    def mean(a):
        a = a[a > -1]
        return float(np.mean(a)) if a.size else -1.0
    t50, t75 = 0, 5                                                 # OKS_THRESHOLDS[0] = .5, [5] = .75
    return {'AP': mean(precision[:, :, 0]), 'AP50': mean(precision[t50, :, 0]), 'AP75': mean(precision[t75, :, 0]),
            'APM': mean(precision[:, :, 1]), 'APL': mean(precision[:, :, 2]),
            'AR': mean(recall[:, 0]), 'AR50': mean(recall[t50:t50 + 1, 0]), 'AR75': mean(recall[t75:t75 + 1, 0]),
            'ARM': mean(recall[:, 1]), 'ARL': mean(recall[:, 2])}
