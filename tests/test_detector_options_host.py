"""CPU: the keys of the Detector's entries for every option of the predict_* methods, as literal tuples - the tools and the
GPU tests find entries by these keys, so they must not move; the parameter classes of the tracker; the layout of a
tracker's rows. The Detector is `object.__new__(Detector)` with the few attributes the argument checks and the entry
builder read; its stores answer every lookup by raising the key, so that a call ends where device work would begin."""
import re
import types

import numpy as np
import pytest

from multiposenet_amd.inference import ConstantVelocity, OneEuro, PoseTracker, TrackStyle
from multiposenet_amd.inference.detector import Detector

B, H, W, THR = 2, 128, 128, 0.25
CAP = (1 << 20, 1 << 12, 1 << 20)                                  # bytes of sources, words of descriptors, bytes of intermediates
SERIAL = 7
STYLE = TrackStyle(keypoints='smoothed')


class _Key(Exception):
    pass


class _Store(dict):
    def get(self, key, default=None):
        raise _Key(key)


class _Capacity(dict):
    def get(self, key, default=None):
        return CAP


def _detector(use_graph):
    det = object.__new__(Detector)
    det.use_graph = use_graph
    det._graphs, det._eager_batches, det._image_capacity = _Store(), _Store(), _Capacity()
    if not use_graph:
        det._graphs = None                                          # the eager path must not look there
    det._has_heatmaps = lambda: True
    det.retinanet = det.assigner = object()
    det.oks_score, det.oks_max_dets = 'box', 20
    det.params = {'max_boxes': 25}
    det.net = types.SimpleNamespace(device='cpu')
    return det


def _tracker(smooth=None, motion=None, streams=1, max_boxes=25, max_tracks=32):
    t = object.__new__(PoseTracker)
    t.streams, t.max_boxes, t.max_tracks, t.similarity, t.smooth, t.motion = streams, max_boxes, max_tracks, 'oks', smooth, motion
    t.device, t.serial = 'cpu', SERIAL
    return t


def _table():
    gt, trk = [{}] * B, _tracker(smooth=OneEuro())
    return [
        (dict(), ()),
        (dict(annotate=True), ('annotate',)),
        (dict(annotate='jpeg'), ('annotate', 'jpeg', '4:2:0')),
        (dict(annotate='jpeg', jpeg_subsampling='4:4:4', jpeg_quality=90), ('annotate', 'jpeg', '4:4:4')),
        (dict(plot_maps=True), ('maps',)),
        (dict(groundtruth=gt), ('oks', 'box', 20)),
        (dict(flip=True), ('tta', True, ())),
        (dict(scales=[(256, 256)]), ('tta', False, ((256, 256),))),
        (dict(track=trk), ('track', SERIAL, B)),
        (dict(track=trk, annotate=True, track_style=STYLE), ('annotate', 'track', SERIAL, B, 'style', STYLE)),
        (dict(annotate='jpeg', jpeg_subsampling='4:2:2', plot_maps=True, groundtruth=gt, flip=True, scales=[(256, 256)], track=trk,
              track_style=STYLE, return_heatmaps=False),
         ('annotate', 'jpeg', '4:2:2', 'maps', 'oks', 'box', 20, 'tta', True, ((256, 256),), 'track', SERIAL, B, 'style', STYLE)),
    ]


def _key_of(call, *args, **kw):
    with pytest.raises(_Key) as e:
        call(*args, **kw)
    return e.value.args[0]


@pytest.mark.parametrize("use_graph", [True, False])
def test_entry_keys_are_the_literal_tuples(use_graph):
    det = _detector(use_graph)
    batch = np.zeros((B, H, W, 3), np.uint8)
    frames = [np.zeros((50, 70, 3), np.uint8), np.zeros((64, 33, 3), np.uint8)]
    for options, tail in _table():
        key = _key_of(det.predict_batch, batch, score_threshold=THR, **options)
        assert key == ((B, H, W, THR) if use_graph else ('eager', B, H, W)) + tail, options
        assert all(type(a) is type(b) for a, b in zip(key, ((B, H, W, THR) if use_graph else ('eager', B, H, W)) + tail))
        key = _key_of(det.predict_images, frames, size=(H, W), score_threshold=THR, **options)
        assert key == ('images', B, H, W, THR, CAP) + tail, options


def test_options_object_spells_the_tail_once():
    det = _detector(True)
    for options, tail in _table():
        given = dict(score_threshold=THR, return_heatmaps=True, annotate=False, jpeg_quality=75, jpeg_subsampling='4:2:0',
                     plot_maps=False, groundtruth=None, flip=False, scales=None, track=None, track_style=None)
        given.update(options)
        opts, shaped = det._options(lambda: (B, H, W), **given)
        assert shaped == (B, H, W) and opts.tail(B) == tail and opts.thr == THR and type(opts.thr) is float
        assert opts.annotate == ((given['jpeg_quality'], given['jpeg_subsampling']) if given['annotate'] == 'jpeg' else given['annotate'])
        assert opts.track is given['track'] and opts.return_heatmaps is given['return_heatmaps']
        with pytest.raises(AttributeError):
            opts.thr = 0.5


def test_one_check_order_on_every_path():
    """annotate, track_style, plot_maps; the path's shapes; groundtruth, track, flip / scales."""
    det = _detector(True)
    batch, frames = np.zeros((B, H, W, 3), np.uint8), [np.zeros((50, 70, 3), np.uint8)] * B
    bad_shape = {det.predict_batch: np.zeros((B, H, W), np.uint8), det.predict_images: [], det.predict_jpegs: []}
    for method, first in ((det.predict_batch, batch), (det.predict_images, frames)):
        with pytest.raises(ValueError, match="annotate must be"):
            method(first, annotate='png', track_style='x', plot_maps=1)
        with pytest.raises(ValueError, match="inference.TrackStyle"):
            method(first, annotate=True, track_style='x', plot_maps=1)
        with pytest.raises(ValueError, match="plot_maps must be"):
            method(bad_shape[method], plot_maps=1)
        with pytest.raises(ValueError, match="groundtruth must be a list of 2"):
            method(first, groundtruth=[{}], track='x', flip=1)
        with pytest.raises(ValueError, match="track must be a tracking.PoseTracker"):
            method(first, track='x', flip=1)
        with pytest.raises(ValueError, match="flip must be"):
            method(first, flip=1)
    for method in bad_shape:
        with pytest.raises(ValueError, match="images must be an array|empty batch"):
            method(bad_shape[method], groundtruth=[{}], track='x', flip=1)


@pytest.mark.parametrize("cls, defaults, text", [
    (OneEuro, dict(rate=30.0, min_cutoff=1.0, beta=float(np.float32(0.007)), d_cutoff=1.0, min_keypoint_score=0.0),
     "OneEuro(rate=30.0, min_cutoff=1.0, beta=0.007000000216066837, d_cutoff=1.0, min_keypoint_score=0.0)"),
    (ConstantVelocity, dict(velocity_gain=0.5, damping=1.0), "ConstantVelocity(velocity_gain=0.5, damping=1.0)"),
], ids=["OneEuro", "ConstantVelocity"])
def test_parameter_classes_keep_their_behaviour(cls, defaults, text):
    p = cls()
    assert repr(p) == text and p.astuple() == tuple(defaults.values()) and list(cls.__slots__) == list(defaults)
    assert not hasattr(p, '__dict__')
    first = next(iter(defaults))
    assert p == cls(**defaults) and hash(p) == hash(cls(**defaults)) and p != cls(**{first: 0.25}) and p != p.astuple()
    assert len({p, cls(), cls(**{first: 0.25})}) == 2
    assert cls(**{first: 0.1}).astuple()[0] == float(np.float32(0.1))           # rounded to what the launch receives
    for change in (lambda: setattr(p, first, 1.0), lambda: setattr(p, 'other', 1.0), lambda: delattr(p, first)):
        with pytest.raises(AttributeError, match=f"^{cls.__name__} is immutable$"):
            change()
    for name in defaults:
        with pytest.raises(ValueError, match=f"^{cls.__name__}: {name} must be a number \\(got 'fast'\\)$"):
            cls(**{name: 'fast'})
        for bad in (float('nan'), float('inf'), 1e39):
            with pytest.raises(ValueError, match="^" + re.escape(f"{cls.__name__}: {name} must be finite (got {bad!r})") + "$"):
                cls(**{name: bad})


def test_parameter_ranges():
    assert OneEuro() != ConstantVelocity()
    for name in ('rate', 'min_cutoff', 'd_cutoff'):
        for bad in (0, -1.5):
            with pytest.raises(ValueError, match=f"^OneEuro: {name} must be > 0 \\(got {bad!r}\\)$"):
                OneEuro(**{name: bad})
    with pytest.raises(ValueError, match=r"^OneEuro: beta must be >= 0 \(got -0.5\)$"):
        OneEuro(beta=-0.5)
    assert OneEuro(beta=0).beta == 0.0 and OneEuro(min_keypoint_score=-3).min_keypoint_score == -3.0
    for name in ('velocity_gain', 'damping'):
        for bad in (-0.25, 1.5):
            with pytest.raises(ValueError, match=f"^ConstantVelocity: {name} must be in 0..1 \\(got {bad!r}\\)$"):
                ConstantVelocity(**{name: bad})
        assert getattr(ConstantVelocity(**{name: 0}), name) == 0.0 and getattr(ConstantVelocity(**{name: 1}), name) == 1.0


@pytest.mark.parametrize("smooth", [None, OneEuro()])
@pytest.mark.parametrize("motion", [None, ConstantVelocity()])
def test_tracker_row_offsets(smooth, motion):
    """The literal layout: 24 bytes a track row, 340 a smoothed row (17 x (x, y, score) + 17 x (dx, dy), float32), 160 a
    coasting row (id, misses, box, 17 x (x, y)); the coasting rows begin at a multiple of 8 bytes."""
    for b, streams, max_boxes, max_tracks in ((1, 1, 25, 32), (4, 2, 25, 7), (6, 3, 64, 64)):
        t = _tracker(smooth, motion, streams, max_boxes, max_tracks)
        n = b * max_boxes * 24
        rows = n + (b * max_boxes * 340 if smooth is not None else 0)
        at = (rows + 7) // 8 * 8 if motion is not None else rows
        end = at + (b * max_tracks * 160 if motion is not None else 0)
        assert t.row_offsets(b) == (n, at, end)
        assert (t.track_bytes(b), t.coast_offset(b), t.out_bytes(b)) == (n, at, end)
    t = _tracker(smooth, motion)
    if smooth is not None and motion is not None:
        assert t.coast_offset(1) == 9104 and t.out_bytes(1) == 9104 + 32 * 160       # 9100 bytes of rows, padded
    with pytest.raises(ValueError, match="not a whole number of frames"):
        _tracker(smooth, motion, streams=2).row_offsets(3)
    with pytest.raises(ValueError, match="mpn_pose_track: 4096 x 64 slots are more than one launch takes"):
        _tracker(smooth, motion, max_boxes=64).row_offsets(4096)
