"""GPU: mpn_anonymize and the `anonymize=` paths of the Detector against the restatement tests/anonymize_ref.py (held against
Pillow and its own properties on the CPU, tests/test_anonymize_host.py). Equality is every byte of every frame, no tolerance:
the definition is integer arithmetic on float64 bounds the kernel computes in the same order. Run it in a process of its
own under a time limit, e.g.

    timeout -k 10 900 python -m pytest -m gpu tests/test_anonymize_gpu.py
"""
import numpy as np
import pytest
import torch

import anonymize_cases as C
import anonymize_ref as R
import draw_ref as D
import pose_gather_ref as G
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, models  # noqa: F401 (models: a fixture)
from test_predict_images_gpu import SHAPES_A, SHAPES_B, _sources

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 7                                # the output is pre-filled: an unwritten byte shows


def _spec(**kw):
    from multiposenet_amd.inference import Anonymize
    return Anonymize(**kw)


def _record(persons, max_boxes):
    """mpn_pose_gather's record for b images whose kept persons are `persons` [(boxes, keypoints)]."""
    b = len(persons)
    rec = np.zeros(G.record_bytes(b, max_boxes), np.uint8)
    header = rec[:G.header_words(b) * 4].view(np.int32)
    rows = rec[G.header_words(b) * 4:].view(G.ROW)
    at = 0
    for i, (boxes, kps) in enumerate(persons):
        n = len(boxes)
        assert n <= max_boxes
        rows["image_index"][at:at + n] = i
        rows["box"][at:at + n] = boxes
        rows["keypoints"][at:at + n] = kps
        header[1 + i] = header[1 + b + i] = n
        at += n
    header[0] = at
    return rec


def _pack(images):
    offsets = np.concatenate([[0], np.cumsum([im.size for im in images])]).astype(np.int64)
    packed = np.concatenate([im.reshape(-1) for im in images] + [np.zeros(5, np.uint8)])
    return packed, offsets[:-1].tolist()


class _Stage:
    """One Anonymizer and its inputs on the device: a launch per spec over the same batch."""

    def __init__(self, images, persons, max_boxes, capacity=None, anonymizer=None):
        from multiposenet_amd.inference import Anonymizer
        self.dev = torch.device("cuda:0")
        packed, offsets = _pack(images)
        self.a = anonymizer or Anonymizer(len(images), max_boxes, capacity or packed.size, self.dev)
        self.a.place([im.shape[:2] for im in images], offsets)
        self.sources = torch.from_numpy(packed).to(self.dev)
        self.record = torch.from_numpy(_record(persons, max_boxes)).to(self.dev)
        self.used = np.zeros(self.a.out.numel(), bool)
        for (at, h, w) in self.a.frames:
            self.used[at:at + h * w * 3] = True

    def run(self, spec, with_keypoints=True):
        self.a.out.fill_(FILL)
        out = self.a.launch(self.sources, self.record, with_keypoints, spec)
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert (host[~self.used] == FILL).all(), "a byte outside every frame was written"
        return self.a.unpack(host), host


def _compare(got, want, msg):
    assert got.dtype == np.uint8 and got.shape == want.shape, msg
    diff = (got != want).any(axis=2)
    assert not diff.any(), (msg, int(diff.sum()), np.argwhere(diff)[:5].tolist(),
                            [(got[y, x].tolist(), want[y, x].tolist()) for y, x in np.argwhere(diff)[:3]])


# ---------------------------------------------------------------------------------------------- the kernels, driven directly
@pytest.fixture(scope="module")
def handmade(cuda):
    """The handmade cases in two ragged batches - one record with keypoints, one without - and their stages."""
    cases = C.cases()
    with_kp = [c for c in cases if c[4]]
    without = [c for c in cases if not c[4]] + with_kp[:3]          # boxes only: with_keypoints = 0 for the whole launch
    return [(group, _Stage([c[1] for c in group], [(c[2], c[3]) for c in group], 25), flag)
            for group, flag in ((with_kp, True), (without, False))]


@pytest.mark.parametrize("mode,shape,region", C.GRID)
def test_kernel_equals_the_reference_on_every_handmade_case(handmade, mode, shape, region):
    spec = _spec(mode=mode, shape=shape, region=region, color=(250, 3, 77))
    changed = 0
    for group, stage, flag in handmade:
        got, _ = stage.run(spec, flag)
        for (name, image, boxes, kps, _), frame in zip(group, got):
            _compare(frame, R.anonymize(image, boxes, kps, spec, flag), (name, mode, shape, region, flag))
            changed += int((frame != image).any(axis=2).sum())
    assert changed > 5000                                           # an empty stage cannot pass


@pytest.mark.parametrize("extra", C.EXTRA, ids=lambda e: "-".join(f"{k}{v}" for k, v in e.items() if k in ('mode', 'blocks', 'radius')))
def test_kernel_at_the_ends_of_the_parameters(handmade, extra):
    spec = _spec(**extra)
    for group, stage, flag in handmade:
        got, _ = stage.run(spec, flag)
        for (name, image, boxes, kps, _), frame in zip(group, got):
            _compare(frame, R.anonymize(image, boxes, kps, spec, flag), (name, extra, flag))


def test_an_empty_image_beside_a_full_one_at_64_slots(cuda):
    cases = {c[0]: c for c in C.cases(full=64)}
    group = [cases["nobody"], cases["full"], cases["nobody"], cases["three_overlapping"]]
    assert len(group[1][2]) == 64
    stage = _Stage([c[1] for c in group], [(c[2], c[3]) for c in group], 64)
    for spec in (_spec(), _spec(mode='blur', region='box', radius=4), _spec(mode='fill', shape='rectangle', region='box')):
        got, _ = stage.run(spec)
        for (name, image, boxes, kps, _), frame in zip(group, got):
            _compare(frame, R.anonymize(image, boxes, kps, spec), (name, spec))
        np.testing.assert_array_equal(got[0], group[0][1])
    # a count above max_boxes and a total above the rows are clamped as the drawing clamps them: 64 rows, 256 rows - the
    # same persons; a count that moves an image's rows away from their image_index leaves those rows without a region
    rec = stage.record.cpu().numpy().copy()
    header = rec[:G.header_words(4) * 4].view(np.int32)
    header[0], header[2] = 1 << 20, 1000
    stage.record.copy_(torch.from_numpy(rec))
    got, _ = stage.run(_spec(mode='fill'))
    for (name, image, boxes, kps, _), frame in zip(group, got):
        _compare(frame, R.anonymize(image, boxes, kps, _spec(mode='fill')), ("clamped counts", name))
    header[1] = 2                                                   # image 0 claims rows 0 and 1; image 1's rows begin at 2
    stage.record.copy_(torch.from_numpy(rec))
    got, _ = stage.run(_spec(mode='fill'))
    np.testing.assert_array_equal(got[0], group[0][1])
    _compare(got[1], R.anonymize(group[1][1], group[1][2][2:], group[1][3][2:], _spec(mode='fill')), "rows 2 .. 63 of image 1")
    # image 3's rows lie at 64 .. 66, the header gives it 66 .. 68: its last person alone
    _compare(got[3], R.anonymize(group[3][1], group[3][2][2:], group[3][3][2:], _spec(mode='fill')), "row 66 of image 3")


def _random_persons(rng, n, h, w):
    """Boxes partly outside the frame; the face joints near the top of the box, some outside the frame, some scoring low."""
    y = np.sort(rng.uniform(-0.15, 1.15, (n, 2)), axis=1)
    x = np.sort(rng.uniform(-0.15, 1.15, (n, 2)), axis=1)
    boxes = np.stack([y[:, 0], x[:, 0], y[:, 1], x[:, 1]], axis=1).astype(F)
    kps = np.zeros((n, 17, 3), F)
    cx = (boxes[:, 1] + boxes[:, 3]) / 2 * w
    top = boxes[:, 0] * h + (boxes[:, 2] - boxes[:, 0]) * h * 0.15
    spread = np.maximum((boxes[:, 3] - boxes[:, 1]) * w * rng.uniform(0.02, 0.2, n), 0.5)
    kps[:, :, 0] = cx[:, None] + rng.uniform(-1, 1, (n, 17)) * spread[:, None]
    kps[:, :, 1] = top[:, None] + rng.uniform(-1, 1, (n, 17)) * spread[:, None]
    kps[:, :, 2] = rng.uniform(0, 1, (n, 17))
    return boxes, kps.astype(F)


RAGGED = [(1080, 1920), (97, 131), (480, 640), (1, 1), (1080, 1919), (33, 1025), (720, 1280), (5, 3),
          (300, 500), (299, 501), (64, 64), (1023, 7), (2, 2047), (121, 121), (600, 800), (17, 4099)]       # test_draw_gpu.py's


@pytest.fixture(scope="module")
def ragged(cuda):
    rng = np.random.RandomState(1)
    counts = ([0, 25, 1] + [int(v) for v in rng.randint(0, 26, len(RAGGED))])[:len(RAGGED)]
    counts[0] = 6                                                   # the 1080 x 1920 frame: a few persons keep the reference quick
    images, persons = [], []
    for (h, w), n in zip(RAGGED, counts):
        images.append(rng.randint(0, 255, (h, w, 3)).astype(np.uint8))
        persons.append(_random_persons(rng, n, h, w))
    assert any(at % 2 for at in _pack(images)[1])                   # odd source offsets
    return images, persons, _Stage(images, persons, 25)


@pytest.mark.parametrize("kw", [dict(), dict(mode='blur', radius=5, min_keypoint_score=0.5),
                                dict(mode='fill', region='box', color=(0, 255, 0)),
                                dict(mode='pixelate', region='box', shape='rectangle', blocks=5)],
                         ids=["pixelate-head", "blur-head", "fill-box", "pixelate-box"])
def test_kernel_equals_the_reference_on_a_ragged_random_batch(ragged, kw):
    images, persons, stage = ragged
    spec = _spec(**kw)
    got, host = stage.run(spec)
    for i, (image, (boxes, kps), frame) in enumerate(zip(images, persons, got)):
        _compare(frame, R.anonymize(image, boxes, kps, spec), (kw, i, image.shape, len(boxes)))
    _, again = stage.run(spec)
    assert again.tobytes() == host.tobytes()                        # bit-identical from run to run


def test_a_second_batch_through_the_same_buffers(ragged):
    """Other shapes and persons that fit the Anonymizer's buffers: `place` and the record are data, nothing else changes."""
    _, _, first = ragged
    rng = np.random.RandomState(5)
    shapes = [(64, 64), (600, 801), (3, 5), (480, 639), (1079, 1920), (7, 1023), (250, 3), (97, 131),
              (1, 33), (111, 77), (37, 53), (500, 300), (2, 2), (720, 1281), (640, 480), (31, 33)]
    images = [rng.randint(0, 255, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    persons = [_random_persons(rng, int(n), h, w) for (h, w), n in zip(shapes, rng.randint(0, 9, len(shapes)))]
    stage = _Stage(images, persons, 25, anonymizer=first.a)
    for spec in (_spec(blocks=3), _spec(mode='blur', radius=2, region='box')):
        got, _ = stage.run(spec)
        for i, (image, (boxes, kps), frame) in enumerate(zip(images, persons, got)):
            _compare(frame, R.anonymize(image, boxes, kps, spec), (spec, i, image.shape))


def test_a_descriptor_that_leaves_the_buffers_leaves_its_image_unwritten(cuda):
    cases = C.cases()[:3]
    stage = _Stage([c[1] for c in cases], [(c[2], c[3]) for c in cases], 25)
    desc = stage.a.desc.cpu().numpy().copy()
    d64 = desc.view(np.int64)
    size = stage.a.out.numel()
    d64[0, 0] = size - 10                                           # reaches past both buffers
    desc[1, 4] = 0                                                  # h = 0
    stage.a.desc.copy_(torch.from_numpy(desc))
    got, host = stage.run(_spec(mode='fill', region='box'))
    at1, h1, w1 = stage.a.frames[1]
    assert (host[:at1 + h1 * w1 * 3] == FILL).all()                 # images 0 and 1: nothing written
    name, image, boxes, kps, _ = cases[2]
    _compare(got[2], R.anonymize(image, boxes, kps, _spec(mode='fill', region='box')), name)


# ---------------------------------------------------------------------------------------------- through the Detector
THR = 0.05
MIN_CHANGED = 500                       # pixels an image's anonymised frame differs in: >= 3 persons of some 100 pixels each


@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _want(frame, o, spec):
    anon = R.anonymize_outputs(frame, o, spec)
    if not spec.overlay:
        return np.concatenate([anon, np.full(anon.shape[:2] + (1,), 255, np.uint8)], axis=2), anon
    return D.draw_everything(anon, o), anon


def _check(got, plain, frames, spec, msg, key="annotated"):
    for i, (a, b, frame) in enumerate(zip(got, plain, frames)):
        assert set(a) == set(b) | {key} and len(a["boxes"]) >= 3, (msg, i)
        _assert_same({k: v for k, v in a.items() if k != key}, dict(b), f"{msg} image {i}:")
        want, anon = _want(frame, a, spec)
        assert int((anon != frame).any(axis=2).sum()) > MIN_CHANGED, (msg, i)
        if key == "annotated":
            assert a[key].dtype == np.uint8 and a[key].shape == frame.shape[:2] + (4,)
            _compare(a[key][..., :3], want[..., :3], f"{msg} image {i}")
            assert (a[key][..., 3] == 255).all()


def test_predict_batch_anonymize(cuda, models, det):
    eager = _detector(models, graph=False)
    images, images2 = _images(), _images((4, 5, 8, 9))
    spec, bare = _spec(region='box', blocks=6), _spec(mode='blur', radius=3, overlay=False)
    plain = det.predict_batch(images, score_threshold=THR)
    plain2 = det.predict_batch(images2, score_threshold=THR)
    annotated = det.predict_batch(images, score_threshold=THR, annotate=True)
    n0 = len(det._graphs)
    got = det.predict_batch(images, score_threshold=THR, annotate=True, anonymize=spec)
    assert len(det._graphs) == n0 + 1                               # one graph more
    _check(got, plain, images, spec, "predict_batch")
    assert any((a["annotated"] != b["annotated"]).any() for a, b in zip(got, annotated))
    _check(det.predict_batch(images2, score_threshold=THR, annotate=True, anonymize=spec), plain2, images2, spec, "replay on other images")
    again = det.predict_batch(images, score_threshold=THR, annotate=True, anonymize=_spec(region='box', blocks=6))     # an equal spec
    for a, b, c in zip(got, again, eager.predict_batch(images, score_threshold=THR, annotate=True, anonymize=spec)):
        _assert_same(a, b, "replay vs replay:")
        _assert_same(a, c, "replay vs eager:")
    assert len(det._graphs) == n0 + 1 and not eager._graphs
    alone = det.predict_batch(images, score_threshold=THR, annotate=True, anonymize=bare)      # overlay=False: the frame alone
    assert len(det._graphs) == n0 + 2
    _check(alone, plain, images, bare, "overlay=False")
    for a, b in zip(det.predict_batch(images, score_threshold=THR, annotate=True), annotated):  # anonymize=None is what it was
        _assert_same(a, b, "anonymize=None after anonymize=:")
    assert len(det._graphs) == n0 + 2
    # no PRN: every person takes the fallback region
    noprn = _detector(models, prn=False)
    head = _spec(mode='fill', shape='rectangle')
    got = noprn.predict_batch(images, score_threshold=THR, annotate=True, anonymize=head)
    _check(got, noprn.predict_batch(images, score_threshold=THR), images, head, "no PRN")
    with pytest.raises(ValueError, match="needs the person detector"):
        _detector(models, detector=False, prn=False).predict_batch(images, annotate=True, anonymize=spec)


@pytest.mark.parametrize("keep", [False, True])
def test_predict_images_anonymize(cuda, det, keep):
    a, b = _sources(SHAPES_A, (1, 2, 3), 1), _sources(SHAPES_B, (4, 5, 6), 3)
    spec = _spec(mode='blur', radius=4) if keep else _spec()
    plain_a = det.predict_images(a, size=(H, W), keep_aspect_ratio=keep)
    plain_b = det.predict_images(b, size=(H, W), keep_aspect_ratio=keep)
    n0 = len(det._graphs)
    _check(det.predict_images(a, size=(H, W), keep_aspect_ratio=keep, annotate=True, anonymize=spec), plain_a, a, spec, f"keep={keep}")
    assert len(det._graphs) == n0 + 1
    # other sizes that fit the capacity: the same graph
    _check(det.predict_images(b, size=(H, W), keep_aspect_ratio=keep, annotate=True, anonymize=spec), plain_b, b, spec, "second batch")
    assert len(det._graphs) == n0 + 1


def test_predict_jpegs_anonymize(cuda, det):
    from multiposenet_amd.inference import encode_jpegs
    from multiposenet_amd.inference import jpeg as J
    sources = _sources(SHAPES_A, (1, 2, 3), 1)
    files = [J.pillow_encode(s, 92, '4:4:4') for s in sources]
    frames = [J.pillow_decode(f) for f in files]
    spec = _spec(region='box', mode='pixelate', blocks=10)
    plain = det.predict_jpegs(files, size=(H, W))
    got = det.predict_jpegs(files, size=(H, W), annotate='jpeg', jpeg_quality=90, anonymize=spec)
    _check(got, plain, frames, spec, "predict_jpegs", key="annotated_jpeg")
    want = encode_jpegs([_want(f, o, spec)[0][..., :3].copy() for f, o in zip(frames, got)], 90, '4:2:0')
    for i, (o, data) in enumerate(zip(got, want)):
        assert isinstance(o["annotated_jpeg"], bytes)
        np.testing.assert_array_equal(J.pillow_decode(o["annotated_jpeg"]), J.pillow_decode(data), err_msg=f"image {i}")


def test_the_stage_reads_the_filtered_record(cuda, det):
    from multiposenet_amd.inference import PoseNms
    images = _images()
    nms, spec = PoseNms(0.0), _spec(mode='fill', region='box', shape='rectangle', color=(0, 0, 255))
    plain = det.predict_batch(images, score_threshold=THR, pose_nms=nms)
    unfiltered = det.predict_batch(images, score_threshold=THR)
    assert any(len(p["boxes"]) < len(u["boxes"]) for p, u in zip(plain, unfiltered))        # the filter removes persons
    got = det.predict_batch(images, score_threshold=THR, annotate=True, pose_nms=nms, anonymize=spec)
    differs = 0
    for i, (a, b, u, frame) in enumerate(zip(got, plain, unfiltered, images)):
        _assert_same({k: v for k, v in a.items() if k != "annotated"}, dict(b), f"image {i}:")
        _compare(a["annotated"][..., :3], _want(frame, a, spec)[0][..., :3], f"pose_nms image {i}")     # the survivors alone
        differs += int((R.anonymize_outputs(frame, u, spec) != R.anonymize_outputs(frame, a, spec)).any())
    assert differs                                                  # the unfiltered record would have given another frame


def test_identities_lie_over_the_mosaic(cuda, det):
    import draw_tracks_ref as T
    from multiposenet_amd.inference import PoseTracker, TrackStyle
    from multiposenet_amd.inference import draw as drawing
    images = _images()
    style, spec = TrackStyle(), _spec(blocks=4)
    stamps, cell = drawing.digit_stamps(style.label_size)
    t_a, t_b = (PoseTracker(streams=4, max_tracks=32, similarity='iou', new_track_score=0.0) for _ in range(2))
    for call in range(2):
        got = det.predict_batch(images, score_threshold=THR, annotate=True, track=t_a, track_style=style, anonymize=spec)
        plain = det.predict_batch(images, score_threshold=THR, track=t_b)
        for i, (a, b, frame) in enumerate(zip(got, plain, images)):
            assert (a["track_ids"] != 0).any()
            _assert_same({k: v for k, v in a.items() if k != "annotated"}, dict(b), f"call {call} image {i}:")
            anon = R.anonymize_outputs(frame, a, spec)
            _compare(a["annotated"][..., :3], T.draw_tracks(anon, a, style, stamps, cell)[..., :3], f"call {call} image {i}")
    with pytest.raises(ValueError, match="overlay=False"):
        det.predict_batch(images, annotate=True, track=t_a, track_style=style, anonymize=_spec(overlay=False))


def test_anonymize_on_result_dicts(cuda, det):
    from multiposenet_amd.inference import anonymize
    images = _images()
    image = images[0]
    outputs = det(image, score_threshold=THR)                        # 'keypoint_positions' + 'keypoint_scores': the gather's arithmetic
    assert len(outputs["boxes"]) >= 3 and "keypoints" not in outputs
    batch = det.predict_batch(images, score_threshold=THR)[0]        # 'keypoints'
    for spec in (None, _spec(mode='blur', radius=6), _spec(region='box', mode='fill', shape='rectangle')):
        for o in (outputs, batch, {"boxes": batch["boxes"]}):
            got = anonymize(image, o, spec)
            assert got.dtype == np.uint8 and got.shape == image.shape
            _compare(got, R.anonymize_outputs(image, o, spec or _spec()), (spec, sorted(o)))
            assert (got != image).any()
    np.testing.assert_array_equal(anonymize(image, {"boxes": np.zeros((0, 4), F)}), image)
    odd = C.frame(3, 37, 53)
    o = {"boxes": np.array([[0.1, 0.2, 0.9, 0.7]], F)}
    _compare(anonymize(odd, o), R.anonymize_outputs(odd, o, _spec()), "a small odd frame")
    with pytest.raises(ValueError, match="anonymize must be None or an inference.Anonymize"):
        anonymize(image, batch, "blur")
    with pytest.raises(ValueError, match="image must be uint8"):
        anonymize(image.astype(np.float32), batch)
