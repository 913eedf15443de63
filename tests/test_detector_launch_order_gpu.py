"""GPU: the order of the launches behind the gather in one `Detector.predict_batch` call with every row stage on - what
DESIGN.md's "The row stages of the Detector" states and the docstrings of the stages describe. Two images of the size and
with the random variables of tests/test_detector_batch_gpu.py, no captured graph: the device side runs once, and every
entry point the call reaches through `_lib.call` is logged by name."""
import pytest

from test_detector_batch_gpu import H, W, _detector, _images, models  # noqa: F401 (models: a fixture)
from test_detector_track_eval_gpu import _groundtruth
from test_detector_zones_gpu import _geo, _tracker

pytestmark = pytest.mark.gpu

# taken from this call on the commit before the stage table, and literal since
LAUNCHES = [
    "mpn_pose_gather",
    "mpn_pose_nms",
    "mpn_oks_match",
    "mpn_pose_track",
    "mpn_track_eval",
    "mpn_zone_events",
    "mpn_track_trails",
    "mpn_density_map",
    "mpn_anonymize",
    "mpn_draw_tracks",
    "mpn_draw_trails",
    "mpn_draw_density",
    "mpn_jpeg_forward",
    "mpn_jpeg_entropy_encode",
]


def test_the_launches_behind_the_gather_keep_their_order(cuda, models, monkeypatch):
    from multiposenet_amd import _lib
    from multiposenet_amd.inference import (Anonymize, DensityMap, PoseNms, TrackEvaluator, TrackStyle, TrackTrails,
                                            ZoneCounter)
    det = _detector(models, graph=False)
    images = _images()[:2]
    plain = det.predict_batch(images, score_threshold=0.0)
    max_boxes = det.params['max_boxes']
    stages = dict(track=_tracker(2), groundtruth=_groundtruth(plain), track_eval=TrackEvaluator(streams=2, max_boxes=max_boxes),
                  pose_nms=PoseNms(threshold=0.3), zones=ZoneCounter(streams=2, max_boxes=max_boxes, **_geo(plain)),
                  trails=TrackTrails(streams=2, max_boxes=max_boxes, frame_size=(H, W), length=5),
                  density=DensityMap(streams=2, max_boxes=max_boxes, frame_size=(H, W), cell=16), annotate='jpeg',
                  anonymize=Anonymize(), track_style=TrackStyle())
    names, call = [], _lib.call

    def logged(name, *args):
        names.append(name)
        return call(name, *args)
    monkeypatch.setattr(_lib, 'call', logged)
    outs = det.predict_batch(images, score_threshold=0.0, **stages)
    monkeypatch.undo()
    print(names)
    assert names[names.index("mpn_pose_gather"):] == LAUNCHES
    assert all(set(o) >= {'oks', 'track_ids', 'track_eval', 'pose_nms_source', 'zones', 'trails', 'density', 'annotated_jpeg'}
               for o in outs)
