"""Duplicate poses removed on the device: keypoint-similarity NMS (`mpn_pose_nms`, include/mpn.h) over the persons of a record.

The detector's box NMS cannot see poses: two boxes on one person whose IoU is below its threshold both survive - a tight box
beside a loose one - and the PRN gives both nearly the same 17 keypoints. `PoseNms` walks an image's persons by score and
drops a person whose OKS-like similarity with an already kept one is above a threshold, as top-down pose estimators do.

    detector.predict_images(frames, pose_nms=PoseNms(0.9))         # inside the captured graph, in front of everything that
                                                                   # reads the record: groundtruth=, track=, annotate=
    pose_nms(outputs, PoseNms(0.9))                                # the same launch for host dicts

Every dict then holds only the surviving persons and gains 'pose_nms_source' int32 [n] (a survivor's index among the image's
persons before the stage), 'pose_nms_absorbed' int32 [n] (how many it suppressed) and 'pose_nms_suppressed' (np.int32, the
image's number of suppressed persons). 'num_boxes' keeps its meaning: the count before the score filter.
"""
import numpy as np

from . import _lib
from .pose_metrics import SCORE_MODES, fill_record
from .tracking import _Parameters

MAX_BOXES = 64                           # persons per image: a person's suppression set is one 64-bit mask
_INFO = np.dtype([('source', np.int32), ('absorbed', np.int32)])
KEYS = ('pose_nms_source', 'pose_nms_absorbed', 'pose_nms_suppressed')


class PoseNms(_Parameters):
    """The parameters of keypoint-similarity NMS (`Detector.predict_*(pose_nms=...)`, `pose_nms`). Immutable.

    threshold: in 0..1; a person is suppressed when its similarity with a kept person is above it (strictly). 1 suppresses
    nothing. min_keypoint_score: a joint counts in a pair's similarity only where both persons score it at least this; a pair
    without such a joint has similarity 0. score: 'box' visits the persons by the detector's score, 'box*keypoints' by that
    times the mean keypoint score (`pose_metrics.SCORE_MODES`); the better-scored person of a pair is the one kept.
    The defaults are NOT tuned: there are no trained weights in this repository to tune them on."""
    __slots__ = ('threshold', 'min_keypoint_score', 'score')

    def __init__(self, threshold=0.9, min_keypoint_score=0.0, score='box'):
        super().__init__(threshold=threshold, min_keypoint_score=min_keypoint_score)
        if not isinstance(score, str) or score not in SCORE_MODES:
            raise ValueError(f"PoseNms: score must be one of {sorted(SCORE_MODES)} (got {score!r})")
        object.__setattr__(self, 'score', score)

    @staticmethod
    def _rule(name, v):
        if name == 'threshold' and not 0 <= v <= 1:
            return "in 0..1"


def add_arguments(ap):
    """The command lines' flags of the stage (evaluate_pose, track_frames)."""
    ap.add_argument("--pose-nms", type=float, nargs="?", const=True, default=None, metavar="THRESHOLD",
                    help="keypoint-similarity NMS of every image's persons on the device; THRESHOLD in 0..1 (default: PoseNms's)")
    ap.add_argument("--pose-nms-min-keypoint-score", type=float, default=0.0, metavar="X",
                    help="joints both persons score at least X count in a pair's similarity (--pose-nms)")
    ap.add_argument("--pose-nms-score", choices=tuple(SCORE_MODES), default="box",
                    help="the score the persons are visited by (--pose-nms)")


def from_arguments(ap, args):
    """The parsed flags of `add_arguments` -> None or the PoseNms; a bad value ends the program through ap.error (status 2)."""
    if args.pose_nms is None:
        return None
    given = {} if args.pose_nms is True else {'threshold': args.pose_nms}
    try:
        return PoseNms(min_keypoint_score=args.pose_nms_min_keypoint_score, score=args.pose_nms_score, **given)
    except ValueError as e:
        ap.error(str(e))


def check_max_boxes(max_boxes):
    if not 1 <= int(max_boxes) <= MAX_BOXES:
        raise ValueError(f"pose_nms: max_boxes must be in 1..{MAX_BOXES} (got {max_boxes}): mpn_pose_nms keeps a person's "
                         "suppression set in one 64-bit mask")
    return int(max_boxes)


def info_layout(b, max_boxes):
    """(bytes of mpn_pose_nms's info block, byte offset of its rows) for (b, max_boxes); raises where one launch does not
    take that many slots."""
    nbytes = _lib.lib().mpn_pose_nms_info_bytes(int(b), check_max_boxes(max_boxes))
    head = (4 * int(b) + 15) // 16 * 16
    if nbytes == 0 or nbytes != head + 2 * int(b) * int(max_boxes) * _INFO.itemsize:
        raise ValueError(f"mpn_pose_nms: {b} x {max_boxes} slots are more than one launch takes")
    return nbytes, head


def unpack_info(info, counts):
    """A host copy of the info block (uint8 array) and record_out's per-image counts -> a list of dicts, one per image, with
    the three keys of KEYS in the image's record order."""
    b = len(counts)
    head = (4 * b + 15) // 16 * 16
    suppressed = np.frombuffer(info, np.int32, b)
    rows = np.frombuffer(info, np.uint8, int(np.sum(counts)) * _INFO.itemsize, head).view(_INFO)
    res, s = [], 0
    for i, n in enumerate(counts):
        r = rows[s:s + int(n)]
        res.append({'pose_nms_source': r['source'].copy(), 'pose_nms_absorbed': r['absorbed'].copy(),
                    'pose_nms_suppressed': np.int32(suppressed[i])})
        s += int(n)
    return res


def launch(record_in, b, max_boxes, nms, record_out, info, sim_out=None):
    """One mpn_pose_nms on the current stream. record_in: the uint8 device tensor mpn_pose_gather wrote for (b, max_boxes);
    record_out: another of the same size; info: uint8 device tensor of `info_layout(b, max_boxes)[0]` bytes; sim_out: float64
    device tensor [b, max_boxes, max_boxes] or None."""
    if not isinstance(nms, PoseNms):
        raise ValueError("pose_nms must be None or an inference.PoseNms")
    _lib.call("mpn_pose_nms", _lib.ptr(record_in), int(b), int(max_boxes), nms.threshold, nms.min_keypoint_score,
              SCORE_MODES[nms.score], _lib.ptr(record_out), record_out.numel(), _lib.ptr(info), info.numel(), _lib.ptr(sim_out),
              _lib.stream_ptr())
    return record_out


class PoseNmsBuffers:
    """The device side of `mpn_pose_nms` for one (b, max_boxes) and one PoseNms: the buffer the unfiltered record lives in
    (`raw`, never copied to the host) and the launch from it. The parameters go by value and the grids depend on b alone: the
    launch can be captured, and the graph follows whatever record the gather writes later."""

    def __init__(self, b, max_boxes, nms, device=None):
        if not isinstance(nms, PoseNms):
            raise ValueError("pose_nms must be None or an inference.PoseNms")
        import torch
        self.b, self.max_boxes, self.nms = int(b), check_max_boxes(max_boxes), nms
        self.info_bytes, self.head_bytes = info_layout(self.b, self.max_boxes)
        self.record_bytes = _lib.lib().mpn_pose_gather_record_bytes(self.b, self.max_boxes)
        self.device = torch.device(device) if device is not None else _lib.current_device()
        self.raw = torch.zeros(self.record_bytes, dtype=torch.uint8, device=self.device)

    def launch(self, record_out, info):
        """`raw`, the record mpn_pose_gather wrote -> record_out (uint8 device tensor of the same size) and info (uint8 device
        tensor of `info_bytes`)."""
        return launch(self.raw, self.b, self.max_boxes, self.nms, record_out, info)

    unpack = staticmethod(unpack_info)


class PoseSuppressor:
    """`mpn_pose_nms` for host arrays, in the manner of `pose_metrics.OksMatcher`: fills a record of mpn_pose_gather's layout
    from b result dicts (`pose_metrics.fill_record`), uploads it, runs the launch and returns the filtered dicts. An image
    may have at most max_boxes <= 64 persons. `similarity` holds the last call's matrix, f64 [b, max_boxes, max_boxes]: the
    similarity of persons p != q of each image in the order they were given, zero elsewhere."""

    def __init__(self, b, max_boxes, device=None):
        import torch
        self.b, self.max_boxes = int(b), check_max_boxes(max_boxes)
        self.info_bytes, _ = info_layout(self.b, self.max_boxes)
        self.record_bytes = _lib.lib().mpn_pose_gather_record_bytes(self.b, self.max_boxes)
        self.device = torch.device(device) if device is not None else _lib.current_device()
        self.record_in = torch.zeros(self.record_bytes, dtype=torch.uint8, device=self.device)
        self.record_out = torch.zeros(self.record_bytes, dtype=torch.uint8, device=self.device)
        self.info = torch.zeros(self.info_bytes, dtype=torch.uint8, device=self.device)
        self.sim = torch.zeros((self.b, self.max_boxes, self.max_boxes), dtype=torch.float64, device=self.device)
        self.similarity = None

    def run(self, record, nms):
        """A host record (uint8 array of `record_bytes`) -> (record_out, info, similarity) as host arrays."""
        import torch
        with torch.cuda.device(self.device):
            self.record_in.copy_(torch.from_numpy(np.ascontiguousarray(record)))
            launch(self.record_in, self.b, self.max_boxes, nms, self.record_out, self.info, self.sim)
            out, info, sim = self.record_out.cpu().numpy(), self.info.cpu().numpy(), self.sim.cpu().numpy()
        self.similarity = sim
        return out, info, sim

    def __call__(self, outputs, nms):
        outputs = list(outputs)
        record, counts = fill_record(outputs, self.b, self.max_boxes)
        out, info, _ = self.run(record, nms)
        kept = out[4:4 + 4 * self.b].view(np.int32)
        persons = []
        for o, n, extra in zip(outputs, counts, unpack_info(info, kept)):
            src = extra['pose_nms_source']
            p = dict(o)                                             # the kept rows are byte copies: the survivors by their index
            for k in ('boxes', 'scores', 'keypoint_scores', 'keypoint_positions', 'keypoints'):
                if k in o and len(o[k]) == n:
                    p[k] = np.ascontiguousarray(np.asarray(o[k])[src])
            p.update(extra)
            persons.append(p)
        return persons


_suppressors = {}


def pose_nms(outputs, nms):
    """The list of result dicts of a `Detector.predict_*` call (or any dicts with 'scores' [n] and 'keypoints' [n,17,3];
    'keypoint_scores' [n,17] for score='box*keypoints') -> the dicts filtered by `nms`, a PoseNms, on the device: the
    surviving persons of 'boxes', 'scores', 'keypoint_scores', 'keypoint_positions', 'keypoints' in their order, plus
    'pose_nms_source', 'pose_nms_absorbed' and 'pose_nms_suppressed'. Other keys are passed through as they are."""
    outputs = list(outputs)
    if not isinstance(nms, PoseNms):
        raise ValueError("pose_nms must be None or an inference.PoseNms")
    most = max([len(o['scores']) for o in outputs] + [1])
    if most > MAX_BOXES:
        raise ValueError(f"pose_nms: an image has {most} persons, mpn_pose_nms takes {MAX_BOXES}")
    max_boxes = 32 if most <= 32 else MAX_BOXES
    key = (len(outputs), max_boxes, str(_lib.current_device()))
    if key not in _suppressors:
        _suppressors[key] = PoseSuppressor(len(outputs), max_boxes)
    return _suppressors[key](outputs, nms)
