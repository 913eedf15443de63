"""GPU: the `crops=` paths of the Detector - `predict_batch` and `predict_images` - against the restatement tests/crops_ref.py
applied to the returned 'boxes' and the input frames, byte for byte; every other key byte-equal to the call without `crops=`;
combined with track= + pose_nms=, with anonymize= + annotate and with format='jpeg'; one graph entry serving a second batch."""
import numpy as np
import pytest

import anonymize_ref as A
import crops_ref as R
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, models  # noqa: F401 (models: a fixture)
from test_predict_images_gpu import SHAPES_A, SHAPES_B, _sources

pytestmark = pytest.mark.gpu

THR = 0.0                               # the threshold of tests/test_detector_batch_gpu.py: nothing is filtered
OWN = ('crops', 'crop_info')


def _spec(**kw):
    from multiposenet_amd.inference import PersonCrops
    return PersonCrops(**kw)


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _check(got, plain, frames, spec, msg):
    """got: the dicts of a call with crops=; plain: of the same call without; frames: what the crops are cut from."""
    persons = 0
    for i, (a, b, frame) in enumerate(zip(got, plain, frames)):
        assert set(a) == set(b) | set(OWN), (msg, i)
        _assert_same({k: v for k, v in a.items() if k not in OWN}, dict(b), f"{msg} image {i}:")
        n = len(a['boxes'])
        want, info = R.person_crops([frame], [a['boxes']], max(n, 1), spec.size, spec.pad, spec.fit, spec.fill)
        want = want[:n]
        if spec.format == 'rgb':
            assert a['crops'].dtype == np.uint8 and a['crops'].shape == (n,) + spec.size + (3,), (msg, i)
            diff = (a['crops'] != want).any(axis=(1, 2, 3)) if n else np.zeros(0, bool)
            assert not diff.any(), (msg, i, np.flatnonzero(diff).tolist(), int((a['crops'] != want).sum()))
        else:
            from multiposenet_amd.inference.jpeg import pillow_encode
            assert isinstance(a['crops'], list) and len(a['crops']) == n
            for k, (data, pixels) in enumerate(zip(a['crops'], want)):
                assert isinstance(data, bytes) and data == pillow_encode(pixels, spec.jpeg_quality, spec.jpeg_subsampling), (msg, i, k)
        assert set(a['crop_info']) == {'rect', 'placed', 'empty', 'too_large', 'clipped'}
        for key, dtype in (('rect', np.float64), ('placed', np.int32), ('empty', np.bool_), ('too_large', np.bool_), ('clipped', np.bool_)):
            value = a['crop_info'][key]
            assert value.dtype == dtype and len(value) == n and value.tobytes() == info[key][:n].astype(dtype).tobytes(), (msg, i, key)
        persons += n
    assert persons >= 1, msg
    return persons


def test_predict_batch_crops(cuda, models, det):
    eager = _detector(models, graph=False)
    images, images2 = _images(), _images((4, 5, 8, 9))
    spec = _spec(pad=0.1)                                           # the default size: tiles of more than 64 KB of LDS
    plain, plain2 = det.predict_batch(images, score_threshold=THR), det.predict_batch(images2, score_threshold=THR)
    n0 = len(det._graphs)
    got = det.predict_batch(images, score_threshold=THR, crops=spec)
    assert len(det._graphs) == n0 + 1                               # one graph more
    assert _check(got, plain, images, spec, "predict_batch") >= 12
    # a second call with another batch replays the same entry, an equal spec finds it
    _check(det.predict_batch(images2, score_threshold=THR, crops=_spec(pad=0.1)), plain2, images2, spec, "replay on other images")
    assert len(det._graphs) == n0 + 1
    for a, b in zip(got, eager.predict_batch(images, score_threshold=THR, crops=spec)):
        _assert_same({k: v for k, v in a.items() if k != 'crop_info'}, {k: v for k, v in b.items() if k != 'crop_info'}, "replay vs eager:")
        _assert_same(a['crop_info'], b['crop_info'], "replay vs eager, crop_info:")
    assert not eager._graphs
    for a, b in zip(det.predict_batch(images, score_threshold=THR), plain):      # crops=None is what it was
        _assert_same(a, b, "crops=None after crops=:")
    # a score threshold that filters: the crops follow the kept persons
    mid = float(np.median(np.concatenate([o['scores'] for o in plain])))
    small = _spec(size=(64, 32), fit='pad', fill=(9, 8, 7))
    kept = det.predict_batch(images, score_threshold=mid, crops=small)
    assert 0 < sum(len(o['boxes']) for o in kept) < sum(len(o['boxes']) for o in plain)
    _check(kept, det.predict_batch(images, score_threshold=mid), images, small, "filtered")
    with pytest.raises(ValueError, match="needs the person detector"):
        _detector(models, detector=False, prn=False).predict_batch(images, crops=spec)


@pytest.mark.parametrize("keep", [False, True])
def test_predict_images_crops(cuda, det, keep):
    a, b = _sources(SHAPES_A, (1, 2, 3), 1), _sources(SHAPES_B, (4, 5, 6), 3)
    assert len({im.shape for im in a}) >= 2                         # frames of different sizes in one batch
    spec = _spec(size=(128, 64), fit='pad' if keep else 'stretch', pad=0.05)
    plain_a = det.predict_images(a, size=(H, W), keep_aspect_ratio=keep, score_threshold=THR)
    plain_b = det.predict_images(b, size=(H, W), keep_aspect_ratio=keep, score_threshold=THR)
    n0 = len(det._graphs)
    _check(det.predict_images(a, size=(H, W), keep_aspect_ratio=keep, score_threshold=THR, crops=spec), plain_a, a, spec, f"keep={keep}")
    assert len(det._graphs) == n0 + 1
    # other sizes that fit the capacity: the same graph
    _check(det.predict_images(b, size=(H, W), keep_aspect_ratio=keep, score_threshold=THR, crops=spec), plain_b, b, spec, "second batch")
    assert len(det._graphs) == n0 + 1


def test_crops_follow_the_filtered_record_and_the_tracker(cuda, det):
    from multiposenet_amd.inference import PoseNms, PoseTracker
    images = _images()
    nms, spec = PoseNms(0.0), _spec(size=(64, 32))
    unfiltered = det.predict_batch(images, score_threshold=THR)

    def tracker():
        return PoseTracker(streams=1, max_boxes=det.params['max_boxes'], device=det.net.device)
    plain = det.predict_batch(images, score_threshold=THR, pose_nms=nms, track=tracker())
    got = det.predict_batch(images, score_threshold=THR, pose_nms=nms, track=tracker(), crops=spec)
    assert any(len(p['boxes']) < len(u['boxes']) for p, u in zip(plain, unfiltered))        # the filter removes persons
    _check(got, plain, images, spec, "pose_nms + track")
    for o in got:                                                   # order and count are those of the other per-person keys
        assert len(o['crops']) == len(o['track_ids']) == len(o['pose_nms_source']) == len(o['crop_info']['empty'])


def test_crops_read_the_anonymised_frames_never_the_overlays(cuda, det):
    from multiposenet_amd.inference import Anonymize
    images = _images()
    anon, spec = Anonymize(region='box', mode='fill', shape='rectangle', color=(0, 0, 255)), _spec(size=(64, 32), pad=0.1)
    plain = det.predict_batch(images, score_threshold=THR, annotate=True, anonymize=anon)
    got = det.predict_batch(images, score_threshold=THR, annotate=True, anonymize=anon, crops=spec)
    frames = [A.anonymize_outputs(frame, o, anon) for frame, o in zip(images, got)]
    assert all((f != im).any() for f, im in zip(frames, images))
    _check(got, plain, frames, spec, "anonymize + annotate")
    # the overlays (white skeletons, red boxes) lie over the frame in 'annotated' only
    assert any((o['annotated'][..., :3] != f).any() for o, f in zip(got, frames))


def test_jpeg_crops_are_the_files_pillow_writes(cuda, det):
    images = _images()
    spec = _spec(size=(64, 32), format='jpeg', jpeg_quality=88, jpeg_subsampling='4:2:2')
    plain = det.predict_batch(images, score_threshold=THR)
    assert _check(det.predict_batch(images, score_threshold=THR, crops=spec), plain, images, spec, "format='jpeg'") >= 12
    frames = _sources(SHAPES_A, (1, 2, 3), 1)
    _check(det.predict_images(frames, size=(H, W), score_threshold=THR, crops=spec), det.predict_images(frames, size=(H, W), score_threshold=THR),
           frames, spec, "format='jpeg', ragged")
