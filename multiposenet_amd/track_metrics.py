"""Tracking accuracy: CLEAR MOT (Bernardin & Stiefelhagen 2008: MOTA, MOTP, switches, fragmentations, mostly tracked / lost)
and the identity measures of Ristani et al. 2016 (IDF1, IDP, IDR), for the persons `Detector.predict_*(track=...)` returns,
against annotations that carry a `track_id` (PoseTrack-style JSON). No tracking-metrics package is a dependency of this
project.

The per-frame part - keypoint OKS of every annotated person against every tracked person, the CLEAR MOT mapping rule, which
remembers the last frame's correspondences, and an optimal assignment of the rest - runs on the device (`mpn_track_eval`,
include/mpn.h): inside the Detector's captured graph behind the tracker's launch when `predict_*` is given `track_eval=`, or
through `TrackEvaluator.update` for host dicts. `evaluate()` accumulates the small per-frame rows and solves the one global
identity matching of IDF1, once per evaluation, on the host.

    tracker, evaluator = PoseTracker(streams=1), TrackEvaluator(streams=1)
    for frames, groundtruth in batches:                     # groundtruth: dicts of pose_metrics.groundtruth_arrays + 'track_ids'
        evaluator.collect(detector.predict_images(frames, track=tracker, groundtruth=groundtruth, track_eval=evaluator))
    evaluator.evaluate()                                    # {'mota': ..., 'idf1': ..., ...}

Like the tracker's, the launch is a PURE function of its inputs and the previous state; `commit()` advances the state (the
Detector does that once per call). The similarity is OKS only: a record's boxes are normalised and ground-truth boxes are
pixels."""
import itertools
import json

import numpy as np

from . import _lib
from .pose_metrics import GT_DOUBLES, MAX_GT, NUM_KEYPOINTS, check_max_gt, fill_record, groundtruth_arrays, pack_groundtruth
from .stream_state import StreamState

MAX_IDENTITIES = 1024                    # identities per stream the kernel's state takes
MAX_BOXES = 64
GT_MATCHED, GT_SWITCH, GT_KEPT, GT_IGNORED = 1, 2, 4, 8
HYP_FALSE_POSITIVE, HYP_IGNORED, HYP_UNTRACKED = 1, 2, 4

# the rows of mpn_track_eval's out and the head of one stream's state (include/mpn.h)
_FRAME = np.dtype([('num_gt', np.int32), ('num_hyp', np.int32), ('matches', np.int32), ('switches', np.int32),
                   ('misses', np.int32), ('false_positives', np.int32), ('ignored_hyp', np.int32), ('untracked', np.int32),
                   ('similarity_sum', np.float64), ('pad', np.uint64)])
_GT = np.dtype([('track_id', np.int32), ('row', np.int32), ('flags', np.int32), ('stored', np.int32),
                ('similarity', np.float64), ('overlaps', np.uint64)])
_HYP = np.dtype([('gt', np.int32), ('flags', np.int32)])
_TRACK_ROW = np.dtype([('track_id', np.int32), ('slot', np.int32), ('hits', np.int32), ('flags', np.int32),
                       ('similarity', np.float64)])
_STATE_HEADER_WORDS = 4


def groundtruth_track_ids(gt, g):
    """The 'track_ids' of a ground-truth dict with g persons -> a list of g Python ints, unique within the image."""
    if not isinstance(gt, dict) or gt.get('track_ids') is None:
        raise ValueError("track_eval: every ground-truth dict needs 'track_ids' (int [g]), the persons' identities")
    ids = [int(v) for v in np.asarray(gt['track_ids']).reshape(-1)]
    if len(ids) != g:
        raise ValueError(f"groundtruth: {g} persons and {len(ids)} track_ids")
    if len(set(ids)) != g:
        raise ValueError("groundtruth: 'track_ids' must be unique within an image")
    return ids


def groundtruth_from_posetrack(json_path):
    """A COCO-style file whose annotations carry `track_id` (PoseTrack) -> [(file_name, groundtruth), ...] in video order: by
    (vid_id, frame_id) where every image has both, else in the file's order. A ground-truth dict is that of
    `pose_metrics.groundtruth_arrays` plus 'track_ids'. An annotation without keypoints with v > 0 (or without 'keypoints' at
    all) is an ignore region; one without `track_id` gets an id no other annotation of the file has."""
    with open(json_path) as f:
        data = json.load(f)
    images = list(data['images'])
    if all('vid_id' in im and 'frame_id' in im for im in images):
        images.sort(key=lambda im: (im['vid_id'], im['frame_id']))
    per_image = {im['id']: [] for im in images}
    for ann in data.get('annotations', []):
        if ann['image_id'] in per_image:
            per_image[ann['image_id']].append(ann)
    spare = max([int(a['track_id']) for a in data.get('annotations', []) if 'track_id' in a] + [0])
    out = []
    for im in images:
        anns = per_image[im['id']]
        ids = []
        for a in anns:
            if 'track_id' not in a:
                spare += 1
            ids.append(int(a['track_id']) if 'track_id' in a else spare)
        boxes = np.array([a.get('bbox', (0, 0, 0, 0)) for a in anns], np.float64).reshape(-1, 4)
        gt = {'keypoints': np.array([a.get('keypoints', [0] * (3 * NUM_KEYPOINTS)) for a in anns],
                                    np.float64).reshape(-1, NUM_KEYPOINTS, 3),
              'boxes': boxes,
              'area': np.array([a.get('area', b[2] * b[3]) for a, b in zip(anns, boxes)], np.float64),
              'iscrowd': np.array([a.get('iscrowd', 0) for a in anns], np.int32),
              'track_ids': np.array(ids, np.int64)}
        out.append((im['file_name'], gt))
    return out


def max_weight_matching(table):
    """table: {(row key, column key): non-negative int} -> the largest total weight any one-to-one matching of rows and
    columns reaches (exact integers): the Hungarian method (shortest augmenting paths with potentials) on the dense square
    matrix of `largest - weight`, absent pairs and padding at weight 0."""
    rows = sorted({r for r, _ in table}, key=repr)
    cols = sorted({c for _, c in table}, key=repr)
    n = max(len(rows), len(cols))
    if n == 0:
        return 0
    weight = np.zeros((n, n), np.int64)
    ri, ci = {r: i for i, r in enumerate(rows)}, {c: i for i, c in enumerate(cols)}
    for (r, c), w in table.items():
        if int(w) < 0:
            raise ValueError("max_weight_matching: weights must not be negative")
        weight[ri[r], ci[c]] = int(w)
    cost = int(weight.max()) - weight
    inf = np.iinfo(np.int64).max // 4
    u, v = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    p, way = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, inf, np.int64)
        used = np.zeros(n + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            better = ~used[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            open_ = np.where(used[1:], inf, minv[1:])
            j1 = int(np.argmin(open_)) + 1
            delta = open_[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0 != 0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return int(sum(weight[p[j] - 1, j - 1] for j in range(1, n + 1)))


def _ratio(a, b):
    return float('nan') if b == 0 else float(a) / float(b)


class _Buffers:
    """The ground truth of one batch size on the device: a pinned staging buffer and its device twin holding the rows of
    mpn_oks_match, their counts and the identity indices (`place`: one host-to-device copy), and the output rows."""

    def __init__(self, b, max_gt, max_boxes, device):
        import torch
        self.b, self.max_gt = b, max_gt
        rows = b * max_gt * GT_DOUBLES
        words = rows + (b + 1) // 2 + (b * max_gt + 1) // 2                                # in doubles
        self.stage = torch.zeros(words, dtype=torch.float64).pin_memory()
        self.dev = torch.zeros(words, dtype=torch.float64, device=device)
        host = self.stage.numpy()
        self.rows = host[:rows].reshape(b, max_gt, GT_DOUBLES)
        self.counts = host[rows:rows + (b + 1) // 2].view(np.int32)[:b]
        self.identity = host[rows + (b + 1) // 2:].view(np.int32)[:b * max_gt].reshape(b, max_gt)
        self.at = (0, rows, rows + (b + 1) // 2)                                           # rows, counts, identities
        self.record = self.track_rows = self.out = None                                    # update(): made on its first call


class TrackAccumulator:
    """The host side of the evaluation: collects the per-image rows (`TrackEvaluator.unpack`'s dicts) with the persons' track
    ids; `evaluate()` sums the counts, walks every annotated person's history and solves the identity matching."""

    def __init__(self):
        self.initialize()

    def initialize(self):
        """Forget what was collected (a TrackEvaluator's state of the mapping rule stays: `reset()` clears that)."""
        self.totals = {k: 0 for k in _FRAME.names[:8]}
        self.similarity_sum = 0.0
        self.num_frames = 0
        self.history = {}                # (stream, epoch, identity) -> [matched in its 1st, 2nd, ... frame]
        self.overlaps = {}               # ((stream, epoch, identity), (stream, epoch, track id)) -> frames
        self.stats = None

    def collect(self, outputs):
        """The b result dicts of a `Detector.predict_*(track=..., track_eval=self)` call, in the order of the calls."""
        for o in outputs:
            if 'track_eval' not in o or 'track_ids' not in o:
                raise ValueError("collect: the dicts carry no 'track_eval'; call predict_* with track= and track_eval=")
            self.add_image(o['track_eval'], o['track_ids'])

    def add_image(self, rows, track_ids):
        """One image's rows (a dict of `unpack`) and its persons' track ids."""
        for k in self.totals:
            self.totals[k] += int(rows[k])
        self.similarity_sum += float(rows['similarity_sum'])
        self.num_frames += 1
        where = (rows['stream'], rows['epoch'])
        track_ids = np.asarray(track_ids).reshape(-1)
        for g in range(len(rows['gt_ignored'])):
            if rows['gt_ignored'][g]:
                continue
            who = where + (int(rows['gt_identities'][g]),)
            self.history.setdefault(who, []).append(bool(rows['gt_matched'][g]))
            mask = int(rows['gt_overlaps'][g])
            for p in range(len(track_ids)):
                if (mask >> p) & 1:
                    key = (who, where + (int(track_ids[p]),))
                    self.overlaps[key] = self.overlaps.get(key, 0) + 1

    def evaluate(self):
        """The measures over everything collected, as a dict (kept in `self.stats`); a ratio with a zero denominator is nan."""
        t = self.totals
        mostly_tracked = mostly_lost = fragmentations = 0
        for seen in self.history.values():
            share = sum(seen) / len(seen)
            mostly_tracked += share >= 0.8
            mostly_lost += share < 0.2
            state = 0                                               # 0 never matched, 1 matched, 2 lost after a match
            for m in seen:
                if m:
                    fragmentations += state == 2
                    state = 1
                elif state == 1:
                    state = 2
        idtp = max_weight_matching(self.overlaps)
        idfn, idfp = t['num_gt'] - idtp, t['num_hyp'] - idtp
        self.stats = {
            'num_frames': self.num_frames, 'num_objects': t['num_gt'], 'num_predictions': t['num_hyp'],
            'num_matches': t['matches'], 'num_switches': t['switches'], 'num_misses': t['misses'],
            'num_false_positives': t['false_positives'],
            'mota': 1 - _ratio(t['misses'] + t['false_positives'] + t['switches'], t['num_gt']),
            'motp': _ratio(self.similarity_sum, t['matches']), 'recall': _ratio(t['matches'], t['num_gt']),
            'precision': _ratio(t['matches'], t['num_hyp']),
            'num_unique_objects': len(self.history), 'mostly_tracked': int(mostly_tracked), 'mostly_lost': int(mostly_lost),
            'partially_tracked': len(self.history) - int(mostly_tracked) - int(mostly_lost),
            'num_fragmentations': int(fragmentations),
            'idtp': idtp, 'idfp': idfp, 'idfn': idfn, 'idp': _ratio(idtp, idtp + idfp), 'idr': _ratio(idtp, idtp + idfn),
            'idf1': _ratio(2 * idtp, 2 * idtp + idfp + idfn)}
        return self.stats


class TrackEvaluator(StreamState, TrackAccumulator):
    """CLEAR MOT and identity measures of `streams` independent cameras, on the device (`mpn_track_eval`).

    A call over b images sees b / streams consecutive frames per stream, stream s owning images s*F .. s*F+F-1 in time order,
    as `tracking.PoseTracker` does. threshold: an annotated person and a tracked person can correspond at OKS >= threshold.
    max_gt: annotated persons per image (at most 64). max_identities: distinct annotated persons per stream between two
    `reset()`s (at most 1024); a stream that needs more raises. max_boxes: the detection slots per image of the records
    (the Detector's params['max_boxes'], the tracker's max_boxes).

    The evaluator owns the state of the mapping rule - per stream and identity the track id it was last matched to - as a prev /
    next pair on the device, and, on the host, one dict per stream from the file's ids to the dense indices the state is
    addressed by. `launch` is pure; `commit()` advances the state. `collect()` takes what `Detector.predict_*(track_eval=self)`
    returns, `update()` is the same launch for host dicts; `evaluate()` gives the numbers."""
    keyword, _serials = 'track_eval', itertools.count(1)

    def __init__(self, streams=1, threshold=0.5, max_gt=MAX_GT, max_identities=256, max_boxes=25, device=None):
        self.streams, self.max_gt = int(streams), check_max_gt(max_gt)
        self.max_identities, self.max_boxes = int(max_identities), int(max_boxes)
        self.threshold = float(threshold)
        if self.streams < 1:
            raise ValueError(f"streams must be at least 1 (got {streams})")
        if self.threshold != self.threshold:
            raise ValueError("threshold must be a number (got nan)")
        if not 1 <= self.max_identities <= MAX_IDENTITIES:
            raise ValueError(f"max_identities must be in 1..{MAX_IDENTITIES} (got {max_identities})")
        if not 1 <= self.max_boxes <= MAX_BOXES:
            raise ValueError(f"max_boxes must be in 1..{MAX_BOXES} (got {max_boxes})")
        import torch
        self.device = torch.device(device) if device is not None else _lib.current_device()
        self.state_bytes = _lib.lib().mpn_track_eval_state_bytes(self.streams, self.max_identities)
        stream_bytes = 4 * (_STATE_HEADER_WORDS + self.max_identities)
        if self.state_bytes == 0 or self.state_bytes != self.streams * stream_bytes:
            raise _lib.MpnError("mpn_track_eval: the state's layout is not the one this binding was written against")
        self._make_state(stream_bytes)
        self._ids = [{} for _ in range(self.streams)]               # per stream: the file's id -> dense index
        self._buffers = {}
        self._placed = None                                         # (b, counts, identities) of the last `place`
        self.last_out = None
        self._epoch = [0] * self.streams                            # the resets of every stream: told apart in `evaluate`
        self.initialize()

    # ---------------------------------------------------------------- the device side
    def out_bytes(self, b):
        """The bytes of a call's rows for b images."""
        self.check_batch(b)
        n = _lib.lib().mpn_track_eval_out_bytes(b, self.max_boxes, self.max_gt)
        if n == 0 or n != b * (_FRAME.itemsize + self.max_gt * _GT.itemsize + self.max_boxes * _HYP.itemsize):
            raise ValueError(f"mpn_track_eval: {b} x {self.max_boxes} slots are more than one launch takes")
        return n

    def buffers(self, b):
        if b not in self._buffers:
            self.out_bytes(b)
            self._buffers[b] = _Buffers(b, self.max_gt, self.max_boxes, self.device)
        return self._buffers[b]

    def dense_identities(self, groundtruth, b):
        """The dense identity indices int32 [b, max_gt] of a call's ground truth (-1: an ignored row, which has no memory).
        New ids take the next free index of their stream; running out of them raises. Nothing changes when it raises."""
        F = self.check_batch(b)
        if not isinstance(groundtruth, (list, tuple)) or len(groundtruth) != b:
            raise ValueError(f"groundtruth must be a list of {b} dicts, one per image")
        out = np.full((b, self.max_gt), -1, np.int32)
        fresh = [dict() for _ in range(self.streams)]
        for i, gt in enumerate(groundtruth):
            s = i // F
            ignore = groundtruth_arrays(gt)[4]
            if len(ignore) > self.max_gt:
                raise ValueError(f"groundtruth: image {i} has {len(ignore)} persons, mpn_track_eval takes {self.max_gt}")
            for j, fid in enumerate(groundtruth_track_ids(gt, len(ignore))):
                if ignore[j]:
                    continue
                known = self._ids[s].get(fid, fresh[s].get(fid))
                if known is None:
                    known = len(self._ids[s]) + len(fresh[s])
                    if known >= self.max_identities:
                        raise ValueError(f"track_eval: stream {s} has more than max_identities = {self.max_identities} annotated "
                                         "persons; make the TrackEvaluator with a larger max_identities (at most "
                                         f"{MAX_IDENTITIES}) or reset() between videos")
                    fresh[s][fid] = known
                out[i, j] = known
        for s in range(self.streams):
            self._ids[s].update(fresh[s])
        return out

    def place(self, groundtruth, b, identities=None, rows=True):
        """This call's ground truth goes to the device: one small pinned copy on the current stream. rows=False (the Detector,
        whose `groundtruth=` buffers hold the rows already): the identity indices alone. identities: dense indices given as they
        are (b arrays [g]; a caller who maps the ids itself) in place of the mapping of 'track_ids'."""
        buf = self.buffers(b)
        if identities is None:
            dense = self.dense_identities(groundtruth, b)
        else:
            dense = np.full((b, self.max_gt), -1, np.int32)
            for i, row in enumerate(identities):
                dense[i, :len(row)] = np.asarray(row, np.int32).reshape(-1)
        if rows:
            pack_groundtruth(groundtruth, buf.rows, buf.counts)
            counts = buf.counts.copy()
        else:
            counts = np.array([len(groundtruth_arrays(gt)[0]) for gt in groundtruth], np.int32)
        buf.identity[...] = dense
        at = 0 if rows else buf.at[2]
        buf.dev[at:].copy_(buf.stage[at:], non_blocking=True)
        self._placed = (b, counts, dense)

    def launch(self, record, track_rows, out, b, gt=None, gt_counts=None):
        """record: the uint8 device tensor the tracker read; track_rows: the uint8 device tensor of mpn_pose_track's rows for it;
        out: uint8 device tensor of `out_bytes(b)`. gt / gt_counts: the device tensors of mpn_oks_match's ground truth for
        (b, max_gt) (default: what `place` uploaded). Reads `prev`, writes `next` and out; `commit()` advances the state."""
        self.check_batch(b)
        buf = self.buffers(b)
        if gt is None:
            gt, gt_counts = buf.dev[buf.at[0]:], buf.dev[buf.at[1]:]
        _lib.call("mpn_track_eval", _lib.ptr(record), _lib.ptr(track_rows), b, self.max_boxes, self.streams, _lib.ptr(gt),
                  _lib.ptr(gt_counts), _lib.ptr(buf.dev[buf.at[2]:]), self.max_gt, self.max_identities, self.threshold,
                  _lib.ptr(self.prev), _lib.ptr(self.next), self.state_bytes, _lib.ptr(out), out.numel(), _lib.stream_ptr())
        return out

    def reset(self, stream=None):
        """Forget the correspondences and the identities seen: of all streams, or of one. What was collected stays."""
        super().reset(stream)
        for s in range(self.streams) if stream is None else [int(stream)]:
            self._ids[s] = {}
            self._epoch[s] += 1

    def state(self, stream=0):
        """A host copy of one stream's current state: {'frames', 'track_ids' int32 [max_identities], 'identities' (the file's
        id -> dense index)}."""
        raw = self._raw_state(stream).view(np.int32)
        return {'frames': int(raw[0]), 'track_ids': raw[_STATE_HEADER_WORDS:].copy(), 'identities': dict(self._ids[int(stream)])}

    def unpack(self, out, counts):
        """A host copy of the output rows (uint8 array) and the record's per-image counts -> a list of b dicts, for the ground
        truth of the last `place`: the frame's 'num_gt', 'num_hyp', 'matches', 'switches', 'misses', 'false_positives',
        'ignored_hyp', 'untracked' (ints) and 'similarity_sum'; per ground truth, in the image's order, 'gt_track_ids' int32 [g]
        (0 = unmatched), 'gt_rows' int32 [g] (the matched person, -1 = none), 'gt_matched', 'gt_switch', 'gt_kept',
        'gt_ignored' bool [g], 'gt_stored' int32 [g] (the track id the identity came with), 'gt_similarity' f64 [g],
        'gt_overlaps' uint64 [g] (bit p: person p is tracked and similar enough), 'gt_identities' int32 [g] (the dense index,
        -1 = none); per person 'person_gt' int32 [n] (-1 = none), 'person_false_positive', 'person_ignored',
        'person_untracked' bool [n]; and 'stream', 'epoch' (the resets of the stream so far)."""
        b, gt_counts, dense = self._placed
        if len(counts) != b:
            raise ValueError(f"unpack: {len(counts)} images, the ground truth in place is for {b}")
        F = self.check_batch(b)
        at = b * _FRAME.itemsize
        frames = np.frombuffer(out, np.uint8, at).view(_FRAME)
        gts = np.frombuffer(out, np.uint8, b * self.max_gt * _GT.itemsize, at).view(_GT).reshape(b, self.max_gt)
        at += b * self.max_gt * _GT.itemsize
        hyps = np.frombuffer(out, np.uint8, b * self.max_boxes * _HYP.itemsize, at).view(_HYP)
        res, s = [], 0
        for i in range(b):
            n, g = int(counts[i]), min(int(gt_counts[i]), self.max_gt)
            r, h = gts[i, :g], hyps[s:s + n]
            d = {k: int(frames[i][k]) for k in _FRAME.names[:8]}
            d['similarity_sum'] = float(frames[i]['similarity_sum'])
            d.update({'gt_track_ids': r['track_id'].copy(), 'gt_rows': r['row'].copy(),
                      'gt_matched': (r['flags'] & GT_MATCHED) != 0, 'gt_switch': (r['flags'] & GT_SWITCH) != 0,
                      'gt_kept': (r['flags'] & GT_KEPT) != 0, 'gt_ignored': (r['flags'] & GT_IGNORED) != 0,
                      'gt_stored': r['stored'].copy(), 'gt_similarity': r['similarity'].copy(),
                      'gt_overlaps': r['overlaps'].copy(), 'gt_identities': dense[i, :g].copy(),
                      'person_gt': h['gt'].copy(), 'person_false_positive': (h['flags'] & HYP_FALSE_POSITIVE) != 0,
                      'person_ignored': (h['flags'] & HYP_IGNORED) != 0, 'person_untracked': (h['flags'] & HYP_UNTRACKED) != 0,
                      'stream': i // F, 'epoch': self._epoch[i // F]})
            res.append(d)
            s += n
        return res

    def update(self, outputs, groundtruth, identities=None, collect=True):
        """The same launch for host arrays: b result dicts that carry 'track_ids' ('scores', 'keypoints' and 'track_ids' as
        `Detector.predict_*(track=...)` returns them; at most max_boxes persons each) and their b ground-truth dicts are
        packed, uploaded, evaluated and committed. Returns what `unpack` returns; collect: also feeds `evaluate()`."""
        import torch
        outputs = list(outputs)
        b = len(outputs)
        nbytes = self.out_bytes(b)
        for o in outputs:
            if 'track_ids' not in o:
                raise ValueError("update: every output dict needs 'track_ids' (a tracking.PoseTracker's)")
        record, counts = fill_record(outputs, b, self.max_boxes)
        rows = np.zeros(b * self.max_boxes, _TRACK_ROW)
        rows['slot'] = -1
        ids = np.concatenate([np.asarray(o['track_ids'], np.int32).reshape(-1) for o in outputs]) if b else np.zeros(0, np.int32)
        rows['track_id'][:len(ids)] = ids
        with torch.cuda.device(self.device):
            buf = self.buffers(b)
            if buf.record is None:
                buf.record = torch.zeros(len(record), dtype=torch.uint8, device=self.device)
                buf.track_rows = torch.zeros(rows.nbytes, dtype=torch.uint8, device=self.device)
                buf.out = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
            self.place(groundtruth, b, identities)
            buf.record.copy_(torch.from_numpy(record))
            buf.track_rows.copy_(torch.from_numpy(rows.view(np.uint8)))
            self.launch(buf.record, buf.track_rows, buf.out, b)
            self.commit()
            out = buf.out.cpu().numpy()
        self.last_out = out                                         # the call's raw rows (the three tables of include/mpn.h)
        res = self.unpack(out, counts)
        if collect:
            for o, r in zip(outputs, res):
                self.add_image(r, o['track_ids'])
        return res
