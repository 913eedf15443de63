"""The bytes a `Detector.predict_*` call brings to the host in ONE copy: mpn_pose_gather's record and, behind it in the same
device buffer, the rows of every stage that ran on it. `RecordLayout` says where each part lies; `unpack_record` turns the
host copy of the record into the result dicts."""
import numpy as np

from .. import _lib

NUM_KEYPOINTS = 17
# a row of mpn_pose_gather's record (include/mpn.h names the fields in this order; offsets and stride come from the library)
_ROW = np.dtype([('image_index', np.int32), ('box', np.float32, (4,)), ('score', np.float32),
                 ('keypoint_scores', np.float32, (NUM_KEYPOINTS,)), ('keypoint_positions', np.float32, (NUM_KEYPOINTS, 2)),
                 ('keypoints', np.float32, (NUM_KEYPOINTS, 3))])


class RecordLayout:
    """Where the parts of the result buffer for b images lie, one slice of bytes each, and `nbytes`, the length of the buffer
    and of the copy. `record` is first: mpn_pose_gather's record (with pose_nms=: the filtered one mpn_pose_nms wrote in its
    place); 0 bytes: more slots than the gather packs. `oks` (a pose_metrics.OksBuffers) and then `track` (a
    tracking.PoseTracker, which lays out its own rows: `row_offsets`) follow packed. Each of `nms` (a
    pose_nms.PoseNmsBuffers: the info block), `track_eval`, `zones`, `trails` and `density` (the objects of those keywords)
    starts at the next multiple of 16 bytes behind the last byte so far. A part whose stage is None is empty, at the stop of
    the part in front of it."""
    PARTS = ('record', 'oks', 'track', 'nms', 'track_eval', 'zones', 'trails', 'density')
    __slots__ = PARTS + ('nbytes',)

    def __init__(self, b, max_boxes, oks=None, track=None, nms=None, track_eval=None, zones=None, trails=None, density=None):
        end = _lib.lib().mpn_pose_gather_record_bytes(b, max_boxes)
        self.record = slice(0, end)
        sizes = {'oks': oks.out_bytes if oks is not None else None, 'nms': nms.info_bytes if nms is not None else None}
        rows = {'track': track, 'track_eval': track_eval, 'zones': zones, 'trails': trails, 'density': density}
        sizes.update({name: stage.out_bytes(b) if stage is not None else None for name, stage in rows.items()})
        for name in self.PARTS[1:]:
            at = end if sizes[name] is None or name in ('oks', 'track') else (end + 15) // 16 * 16
            end = at + (sizes[name] or 0)
            setattr(self, name, slice(at, end))
        self.nbytes = end

    def astuple(self):
        """The eight slices, in the order of PARTS."""
        return tuple(getattr(self, name) for name in self.PARTS)


def _no_persons(num_boxes=0):
    return {'boxes': np.zeros([0, 4], np.float32), 'scores': np.zeros([0], np.float32), 'num_boxes': np.int32(num_boxes),
            'keypoint_scores': np.zeros([0, NUM_KEYPOINTS], np.float32), 'keypoint_positions': np.zeros([0, NUM_KEYPOINTS, 2], np.float32),
            'keypoints': np.zeros([0, NUM_KEYPOINTS, 3], np.float32)}


def unpack_record(record, b, max_boxes, with_keypoints=True):
    """A host copy of mpn_pose_gather's record (uint8 array) -> a list of b dicts: 'boxes' [n,4], 'scores' [n], 'num_boxes',
    'keypoint_scores' [n,17], 'keypoint_positions' [n,17,2], 'keypoints' [n,17,3] (the three keypoint arrays empty when the
    graph has no PRN). Raises like `check_nms` when the record carries a set NMS overflow word."""
    lib = _lib.lib()
    first, stride = lib.mpn_pose_gather_row_offset(b, max_boxes, 0), lib.mpn_pose_gather_row_offset(b, max_boxes, 1)
    stride -= first
    if stride != _ROW.itemsize or len(record) < RecordLayout(b, max_boxes).record.stop:
        raise _lib.MpnError("mpn_pose_gather: the record's layout is not the one this binding was written against")
    header = record[:first].view(np.int32)
    total, counts, num_boxes, overflow = int(header[0]), header[1:1 + b], header[1 + b:1 + 2 * b], int(header[1 + 2 * b])
    if overflow != 0:
        raise RuntimeError("mpn_retina_nms: a candidate list overflowed its workspace (MPN_ERR_WORKSPACE); the detections are incomplete")
    rows = record[first:first + total * stride].copy().view(_ROW)      # (the pinned buffer is reused by the next call)
    out, s = [], 0
    for i in range(b):
        e = s + int(counts[i])
        r = rows[s:e]
        p = _no_persons(num_boxes[i])
        p.update({'boxes': np.ascontiguousarray(r['box']), 'scores': np.ascontiguousarray(r['score'])})
        if with_keypoints:
            p.update({k: np.ascontiguousarray(r[k]) for k in ('keypoint_scores', 'keypoint_positions', 'keypoints')})
        out.append(p)
        s = e
    return out
