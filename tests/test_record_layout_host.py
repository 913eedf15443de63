"""CPU: `RecordLayout` - where the parts of a predict_* call's one result buffer lie - against a plain-loop restatement of the
byte rule, over every combination of the seven optional parts. The stages are stubs whose sizes are odd, so that the
alignment shows; only the record's own size comes from the library."""
import itertools

import pytest

from multiposenet_amd import _lib
from multiposenet_amd.inference.detector import RecordLayout

PACKED = ('oks', 'track')                                           # behind the record with no alignment
ALIGNED = ('nms', 'track_eval', 'zones', 'trails', 'density')       # each at the next multiple of 16 bytes
SIZES = dict(oks=4093, track=601, nms=777, track_eval=1237, zones=333, trails=7919, density=45)     # none a multiple of 16


class _Rows:
    def __init__(self, per_image):
        self.per_image = per_image

    def out_bytes(self, b):
        return self.per_image * b + 1


def _stub(name, b):
    """-> (the stage as `RecordLayout` takes it, its bytes for b images)"""
    if name == 'oks':
        return type('Oks', (), {'out_bytes': SIZES[name]})(), SIZES[name]
    if name == 'nms':
        return type('Nms', (), {'info_bytes': SIZES[name]})(), SIZES[name]
    return _Rows(SIZES[name]), SIZES[name] * b + 1


def reference_layout(record_bytes, sizes):
    """The byte rule as a loop. sizes: {part: bytes} of the parts that are there -> ({part: (start, stop)}, total bytes)."""
    spans, end = {'record': (0, record_bytes)}, record_bytes
    for name in PACKED + ALIGNED:
        start = end
        if name in sizes:
            if name in ALIGNED:
                while start % 16:
                    start += 1
            end = start + sizes[name]
        spans[name] = (start, end)
    return spans, end


@pytest.mark.parametrize("b, max_boxes", [(1, 1), (4, 25)])
def test_every_combination_follows_the_byte_rule(b, max_boxes):
    assert RecordLayout.PARTS == ('record',) + PACKED + ALIGNED and all(v % 16 for v in SIZES.values())
    record_bytes = _lib.lib().mpn_pose_gather_record_bytes(b, max_boxes)
    assert record_bytes > 0
    seen = 0
    for present in itertools.product((False, True), repeat=len(PACKED + ALIGNED)):
        stages, sizes = {}, {}
        for name, there in zip(PACKED + ALIGNED, present):
            stages[name] = None
            if there:
                stages[name], sizes[name] = _stub(name, b)
        layout = RecordLayout(b, max_boxes, **stages)
        spans, total = reference_layout(record_bytes, sizes)
        for name in RecordLayout.PARTS:
            part = getattr(layout, name)
            assert (part.start, part.stop, part.step) == spans[name] + (None,), (present, name)
        assert layout.nbytes == total and layout.astuple() == tuple(getattr(layout, n) for n in RecordLayout.PARTS)
        seen += 1
    assert seen == 128
