"""GPU: mpn_draw_tracks and the `track_style=` paths of the Detector against the numpy restatement tests/draw_tracks_ref.py
(held against Pillow on the CPU, tests/test_draw_tracks_host.py). Equality is every byte of every frame. The digit stamps
are rendered at run time and go to both the kernel and the restatement, so equality does not depend on the font the
machine's Pillow carries. Run it in a process of its own under a time limit, e.g.

    timeout -k 10 900 python -m pytest -m gpu tests/test_draw_tracks_gpu.py
"""
import json

import numpy as np
import pytest
import torch

import draw_tracks_ref as T
import pose_gather_ref as G
from test_detector_batch_gpu import H, W, _assert_same, _detector, _images, models  # noqa: F401 (models: a fixture)
from test_draw_gpu import _draw, _random_persons, _record
from test_draw_tracks_host import INT_MAX, case_table
from test_predict_images_gpu import SHAPES_A, SHAPES_B, _sources

pytestmark = pytest.mark.gpu

F = np.float32
TRACK_ROW = np.dtype([('track_id', np.int32), ('slot', np.int32), ('hits', np.int32), ('flags', np.int32),
                      ('similarity', np.float64)])
SMOOTH_ROW = np.dtype([('keypoints', np.float32, (17, 3)), ('velocities', np.float32, (17, 2))])


def _style(**kw):
    from multiposenet_amd.inference import TrackStyle
    return TrackStyle(**kw)


def _stamps(style):
    from multiposenet_amd.inference import draw
    return draw.digit_stamps(style.label_size)


def _launch(images, rec, track_ids, style, max_boxes, with_keypoints=True, smoothed=None, tables=None):
    """The kernel on a ragged batch packed as predict_images packs it, on a handwritten record, track rows (ids in record row
    order) and smooth rows -> the frames."""
    from multiposenet_amd.inference import draw
    dev = torch.device("cuda:0")
    b = len(images)
    offsets = np.concatenate([[0], np.cumsum([im.size for im in images])]).astype(np.int64)
    packed = np.concatenate([im.reshape(-1) for im in images] + [np.zeros(4, np.uint8)])
    buffers = draw.Buffers(b, max_boxes, packed.size, dev)
    buffers.out.fill_(7)                                            # every byte of a frame is written
    buffers.place([im.shape[:2] for im in images], offsets[:-1].tolist())
    rows = np.zeros(b * max_boxes, TRACK_ROW)
    rows['track_id'][:len(track_ids)] = track_ids
    rows['slot'], rows['similarity'] = -1, 0.5                      # what the drawing must not read
    smooth = None
    if smoothed is not None:
        smooth = np.zeros(b * max_boxes, SMOOTH_ROW)
        smooth['keypoints'][:len(smoothed)] = smoothed
        smooth['velocities'] = 3.0
    up = lambda a: None if a is None else torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(dev)     # noqa: E731
    table = style.tables() if tables is None else tables
    out = buffers.launch_tracks(up(packed), up(rec), up(rows), up(smooth), up(table), with_keypoints)
    torch.cuda.synchronize()
    return buffers.unpack(out.cpu().numpy())


def _draw_tracks(images, persons, style, max_boxes=25, with_keypoints=True, smoothed=False):
    """persons: per image (boxes, keypoint_positions, track_ids[, keypoints_smoothed])."""
    rec = _record([(p[0], p[1]) for p in persons], max_boxes)
    ids = np.concatenate([np.asarray(p[2], np.int32) for p in persons])
    sm = np.concatenate([np.asarray(p[3], F).reshape(-1, 17, 3) for p in persons]) if smoothed else None
    return _launch(images, rec, ids, style, max_boxes, with_keypoints, sm)


def _want(image, person, style, with_keypoints=True):
    stamps, cell = _stamps(style)
    o = {"boxes": person[0], "keypoint_positions": person[1] if with_keypoints else np.zeros((0, 17, 2), F), "track_ids": person[2]}
    if style.keypoints == "smoothed":
        o["keypoints_smoothed"] = person[3] if with_keypoints else np.zeros((0, 17, 3), F)
    return T.draw_tracks(image, o, style, stamps, cell)


def _assert_frames(got, want, msg):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.uint8 and a.shape == b.shape, (msg, i)
        diff = (a != b).any(axis=2)
        assert not diff.any(), (msg, i, a.shape, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def test_kernel_equals_the_restatement_on_the_host_case_table(cuda):
    """The label cases of tests/test_draw_tracks_host.py: one ragged launch per (style, with keypoints)."""
    groups = {}
    for c in case_table():
        groups.setdefault((c["style"], len(c["outputs"]["keypoint_positions"]) > 0), []).append(c)
    assert len(groups) >= 8
    for (style, with_kp), cases in groups.items():
        persons = []
        for c in cases:
            o = c["outputs"]
            n = len(o["boxes"])
            persons.append((o["boxes"], o["keypoint_positions"] if with_kp else np.zeros((n, 17, 2), F), o["track_ids"],
                            o.get("keypoints_smoothed")))
        got = _draw_tracks([c["image"] for c in cases], persons, style, with_keypoints=with_kp,
                           smoothed=style.keypoints == "smoothed")
        stamps, cell = _stamps(style)
        _assert_frames(got, [T.draw_tracks(c["image"], c["outputs"], style, stamps, cell) for c in cases],
                       [c["name"] for c in cases])


def _tracked_persons(rng, n, ids=None):
    boxes, pos = _random_persons(rng, n)
    if ids is None:                                                 # 1, 2 and 10 digits, beyond the palette, and untracked
        ids = rng.choice([0, 0, 1, 7, 12, 13, 25, 96, 4096, 1000000000, INT_MAX], n)
    smoothed = np.concatenate([rng.uniform(-8, 70, (n, 17, 2)), rng.uniform(0, 1, (n, 17, 1))], axis=2).astype(F)
    return boxes, pos, np.asarray(ids, np.int32), smoothed


SIZES = [(1, 1), (5, 7), (33, 67)]


@pytest.mark.parametrize("shapes,max_boxes", [([(1, 1)], 25), ([(5, 7)], 25), ([(33, 67)], 25), (SIZES, 25), (SIZES, 1)])
@pytest.mark.parametrize("untracked", ["plain", "hide"])
def test_kernel_equals_the_restatement_on_small_frames(cuda, shapes, max_boxes, untracked):
    """1x1; 5x7 (the flat walk's tail group, an odd width); 33x67 (more than one block); the three as a ragged batch; one
    slot per image. Tracked and untracked persons mixed; smooth_rows NULL against given; boxes and labels only; twice."""
    rng = np.random.RandomState(len(shapes) * 100 + max_boxes)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    persons = [_tracked_persons(rng, min(n, max_boxes)) for n in ([6, 0, 9] if len(shapes) > 1 else [7])]
    persons[0][2][0], persons[-1][2][-1] = 0, 1000000000            # whatever the draw gave: both kinds, and ten digits
    assert any((p[2] == 0).any() for p in persons) and any((p[2] > 0).any() for p in persons)
    frame, smooth = _style(untracked=untracked), _style(untracked=untracked, keypoints="smoothed", label_size=16)
    got = _draw_tracks(images, persons, frame, max_boxes)
    _assert_frames(got, [_want(im, p, frame) for im, p in zip(images, persons)], "smooth_rows NULL")
    _assert_frames(_draw_tracks(images, persons, frame, max_boxes), got, "launched twice")
    # smooth rows given but the style draws the frame's keypoints: the Detector then passes NULL; given, they are drawn
    given = _draw_tracks(images, persons, smooth, max_boxes, smoothed=True)
    _assert_frames(given, [_want(im, p, smooth) for im, p in zip(images, persons)], "smooth_rows given")
    only = _draw_tracks(images, persons, frame, max_boxes, with_keypoints=False)
    _assert_frames(only, [_want(im, p, frame, False) for im, p in zip(images, persons)], "with_keypoints = 0")


def test_every_slot_of_the_largest_record(cuda):
    """B * max_boxes = 4096: 64 tiny frames with up to 64 persons each, every word of the wave masks in use."""
    rng = np.random.RandomState(64)
    shapes = [SIZES[i % 3] if i % 5 else (9, 14) for i in range(64)]
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    persons = [_tracked_persons(rng, 64 if i % 7 == 0 else int(rng.randint(0, 5))) for i in range(64)]
    style = _style()
    got = _draw_tracks(images, persons, style, max_boxes=64)
    _assert_frames(got, [_want(im, p, style) for im, p in zip(images, persons)], "64 x 64")


def test_glyphs_wider_than_their_cell(cuda):
    """Stamps of random bytes, each a pixel outside its cell on both sides (whatever font the machine has): where two
    neighbours overlap the pixel is blended twice, the left digit first."""
    rng = np.random.RandomState(9)
    cell = 5
    stamps = tuple((rng.randint(0, 256, (6 + d % 3, cell + 2)).astype(np.uint8), (-1, 1 + d % 2)) for d in range(10))
    style = _style(text_color=(255, 250, 3))
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in [(33, 67), (5, 7)]]
    persons = [_tracked_persons(rng, 4, ids=[1234567890, 98, 0, 7]), _tracked_persons(rng, 1, ids=[INT_MAX])]
    rec = _record([(p[0], p[1]) for p in persons], 25)
    got = _launch(images, rec, np.concatenate([p[2] for p in persons]), style, 25, tables=style.tables(stamps, cell))
    want = [T.draw_tracks(im, {"boxes": p[0], "keypoint_positions": p[1], "track_ids": p[2]}, style, stamps, cell)
            for im, p in zip(images, persons)]
    _assert_frames(got, want, "overlapping stamps")
    apart = tuple((np.where(np.arange(cell + 2) % (cell + 1) == 0, 0, m).astype(np.uint8), o) for m, o in stamps)
    other = [T.draw_tracks(im, {"boxes": p[0], "keypoint_positions": p[1], "track_ids": p[2]}, style, apart, cell)
             for im, p in zip(images, persons)]
    assert any((a != b).any() for a, b in zip(want, other))         # the columns outside the cells show in the frames


def _clamped(header, b, max_boxes):
    """The rows of each image as mpn_draw_detections clamps the record's header: [(first, count)]."""
    total = min(max(int(header[0]), 0), b * max_boxes)
    out, first = [], 0
    for i in range(b):
        first = min(first, total)
        count = min(min(max(int(header[1 + i]), 0), max_boxes), total - first)
        out.append((first, count))
        first += min(max(int(header[1 + i]), 0), max_boxes)
    return out


@pytest.mark.parametrize("total,counts", [(0, [2, 2]), (99, [7, 9]), (3, [2, 2]), (-5, [1, 1]), (4, [2, -3]), (1 << 30, [1 << 30, 1])])
def test_record_header_is_clamped_as_draw_detections_clamps_it(cuda, total, counts):
    """A header that names more rows than the record holds (or none, or a negative number): only rows inside the record are
    drawn, the same rows mpn_draw_detections draws."""
    rng = np.random.RandomState(5)
    b, max_boxes = 2, 2
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in [(33, 67), (20, 31)]]
    full = [_tracked_persons(rng, 2, ids=[3, 0]), _tracked_persons(rng, 2, ids=[44, 5])]
    rec = _record([(p[0], p[1]) for p in full], max_boxes)
    header = rec[:G.header_words(b) * 4].view(np.int32)
    header[0], header[1:1 + b] = total, counts
    rows = rec[G.header_words(b) * 4:].view(G.ROW)
    ids = np.concatenate([p[2] for p in full])
    style = _style()
    got = _launch(images, rec, ids, style, max_boxes)
    want, drawn = [], 0
    for i, (first, count) in enumerate(_clamped(header, b, max_boxes)):
        # (the sizes that scale a row are those of the image the ROW names: in every case here the image that draws it)
        sel = slice(first, first + count)
        assert (rows["image_index"][sel] == i).all()
        want.append(_want(images[i], (rows["box"][sel], rows["keypoint_positions"][sel], ids[sel]), style))
        drawn += count
    _assert_frames(got, want, (total, counts))
    assert drawn == {0: 0, 99: 4, 3: 3, -5: 0, 4: 2, 1 << 30: 3}[total]
    plain = _launch(images, rec, np.zeros(4, np.int32), style, max_boxes)
    _assert_frames(plain, _draw_with_record(images, rec, max_boxes), "all untracked: mpn_draw_detections")


def _draw_with_record(images, rec, max_boxes):
    """mpn_draw_detections on a handwritten record."""
    from multiposenet_amd.inference import draw
    dev = torch.device("cuda:0")
    offsets = np.concatenate([[0], np.cumsum([im.size for im in images])]).astype(np.int64)
    packed = np.concatenate([im.reshape(-1) for im in images] + [np.zeros(4, np.uint8)])
    buffers = draw.Buffers(len(images), max_boxes, packed.size, dev)
    buffers.place([im.shape[:2] for im in images], offsets[:-1].tolist())
    out = buffers.launch(torch.from_numpy(packed).to(dev), torch.from_numpy(rec).to(dev), True)
    torch.cuda.synchronize()
    return buffers.unpack(out.cpu().numpy())


def test_untracked_plain_equals_draw_detections(cuda):
    """Every track_id 0 and untracked='plain': the bytes of mpn_draw_detections on the same record, labels on or off; hidden:
    the frames with alpha 255."""
    rng = np.random.RandomState(11)
    shapes = [(97, 131), (1, 1), (5, 7), (33, 67), (120, 160)]
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    persons = [_tracked_persons(rng, n, ids=np.zeros(n, np.int32)) for n in (25, 3, 0, 8, 13)]
    plain = _draw(images, [(p[0], p[1]) for p in persons])
    for style in (_style(), _style(labels=False, palette=[(1, 2, 3)], line_color=(9, 9, 9))):
        _assert_frames(_draw_tracks(images, persons, style), plain, style)
    hidden = _draw_tracks(images, persons, _style(untracked="hide"))
    for im, frame in zip(images, hidden):
        np.testing.assert_array_equal(frame[..., :3], im)
        assert (frame[..., 3] == 255).all()


def test_a_bad_table_leaves_the_primitive_undrawn(cuda):
    """The table is data on the device: whatever it holds, no index derived from it leaves it and the launch succeeds. A
    palette that does not fit leaves tracked persons undrawn; sizes out of range or a digit's stamp that points outside the
    table leave the label undrawn."""
    rng = np.random.RandomState(3)
    image = rng.randint(0, 256, (33, 67, 3)).astype(np.uint8)
    person = _tracked_persons(rng, 3, ids=[5, 0, 55])               # every label holds the digit 5
    style = _style()
    good = style.tables()
    rec = _record([person[:2]], 25)

    def with_word(word, value):
        bad = good.copy()
        bad[:232].view(np.int32)[word] = value
        return _launch([image], rec, person[2], style, 25, tables=bad)

    untracked_only = tuple(a[1:2] for a in person)
    _assert_frames(with_word(3, 1 << 20), [_want(image, untracked_only, style)], "a palette beyond the table")
    _assert_frames(with_word(3, 0), [_want(image, untracked_only, style)], "an empty palette")
    no_labels = [_want(image, person, _style(labels=False))]
    stamp5 = 8 + 5 * 5                                              # digit 5's descriptor: w, h, ox, oy, byte offset
    for word, value in ((stamp5 + 4, 1 << 30), (stamp5 + 4, -4), (stamp5 + 4, 0), (stamp5 + 1, 1 << 20), (stamp5, 9), (stamp5 + 2, -2), (stamp5 + 2, 3),
                        (4, 0), (4, 33), (6, 1000), (5, -1000)):
        _assert_frames(with_word(word, value), no_labels, ("bad table word", word, value))
    _assert_frames(with_word(7, 12345), [_want(image, person, style)], "the reserved word is not read")


# ---------------------------------------------------------------------------------------------- through the Detector
@pytest.fixture(scope="module")
def det(cuda, models):
    return _detector(models)


def _tracker(streams, **kw):
    from multiposenet_amd.inference import PoseTracker
    return PoseTracker(streams=streams, max_tracks=32, similarity='iou', new_track_score=0.0, **kw)


def _restated(frames, outs, style):
    stamps, cell = _stamps(style)
    return [T.draw_tracks(f, o, style, stamps, cell) for f, o in zip(frames, outs)]


def _check_call(got, plain, frames, style, msg, key="annotated"):
    """got: a call with track_style; plain: the same call on a tracker in the same state without it."""
    for i, (a, b) in enumerate(zip(got, plain)):
        assert (a["track_ids"] != 0).any(), (msg, i)                # identities to draw
        assert set(a) == set(b)
        _assert_same({k: v for k, v in a.items() if k != key}, {k: v for k, v in b.items() if k != key}, msg)
    if key == "annotated":
        _assert_frames([o["annotated"] for o in got], _restated(frames, got, style), msg)
        assert all((a["annotated"] != b["annotated"]).any() for a, b in zip(got, plain)), msg   # not the red and white picture


@pytest.mark.parametrize("graph", [True, False])
def test_predict_batch_track_style(cuda, models, det, graph):
    d = det if graph else _detector(models, graph=False)
    images, images2 = _images(), _images((4, 5, 8, 9))
    style = _style()
    t_style, t_plain = _tracker(4), _tracker(4)
    n0 = len(d._graphs)
    for c, batch in enumerate((images, images, images2)):          # the first call, a replay, a replay on other frames
        got = d.predict_batch(batch, score_threshold=0.05, annotate=True, track=t_style, track_style=style)
        plain = d.predict_batch(batch, score_threshold=0.05, annotate=True, track=t_plain)
        _check_call(got, plain, batch, style, f"predict_batch graph={graph} call {c}")
    assert len(d._graphs) == (n0 + 2 if graph else 0)               # one entry with the style, one without
    hidden = _style(untracked="hide", labels=False)
    got = d.predict_batch(images, score_threshold=0.05, annotate=True, track=_tracker(4, max_misses=0), track_style=hidden)
    _assert_frames([o["annotated"] for o in got], _restated(images, got, hidden), "another style: another entry")
    assert len(d._graphs) == (n0 + 3 if graph else 0)


def test_predict_images_track_style_and_smoothed(cuda, det):
    from multiposenet_amd.inference import OneEuro
    a, b = _sources(SHAPES_A, (1, 2, 3), 1), _sources(SHAPES_B, (4, 5, 6), 3)
    style = _style(keypoints="smoothed", label_size=16)
    t_style, t_plain = _tracker(4, smooth=OneEuro(rate=30.0)), _tracker(4, smooth=OneEuro(rate=30.0))
    n0 = len(det._graphs)
    for c, frames in enumerate((a, a, b)):
        got = det.predict_images(frames, size=(H, W), annotate=True, track=t_style, track_style=style)
        plain = det.predict_images(frames, size=(H, W), annotate=True, track=t_plain)
        assert all("keypoints_smoothed" in o for o in got)
        _check_call(got, plain, frames, style, f"predict_images smoothed call {c}")
    assert len(det._graphs) == n0 + 2
    frame_style = _style()
    got = det.predict_images(a, size=(H, W), annotate=True, track=t_style, track_style=frame_style)
    _assert_frames([o["annotated"] for o in got], _restated(a, got, frame_style), "the frame's keypoints, the same tracker")
    with pytest.raises(ValueError, match="without smooth="):
        det.predict_images(a, size=(H, W), annotate=True, track=_tracker(4), track_style=style)


def test_annotate_jpeg_carries_the_identities(cuda, det):
    from multiposenet_amd.inference import jpeg as J
    sources = _sources(SHAPES_A, (1, 2, 3), 1)
    style = _style()
    t_jpeg, t_drawn = _tracker(4), _tracker(4)
    for c in range(2):
        got = det.predict_images(sources, size=(H, W), annotate='jpeg', jpeg_quality=90, track=t_jpeg, track_style=style)
        drawn = det.predict_images(sources, size=(H, W), annotate=True, track=t_drawn, track_style=style)
        for i, (a, frame) in enumerate(zip(got, _restated(sources, drawn, style))):
            assert (a["track_ids"] != 0).any() and set(a) == (set(drawn[i]) - {"annotated"}) | {"annotated_jpeg"}
            assert a["annotated_jpeg"] == J.pillow_encode(frame, 90, '4:2:0'), (c, i)
            _assert_same({k: v for k, v in a.items() if k != "annotated_jpeg"},
                         {k: v for k, v in drawn[i].items() if k != "annotated"}, "annotate='jpeg' vs True")


def test_draw_tracks_on_a_call_result(cuda, det):
    from multiposenet_amd.inference import draw_tracks
    images = _images()
    outs = det.predict_batch(images, score_threshold=0.05, track=_tracker(4, smooth=None))
    style = _style(label_size=16)
    for im, o in zip(images[:2], outs[:2]):
        assert (o["track_ids"] != 0).any()
        _assert_frames([draw_tracks(im, o, style)], _restated([im], [o], style), "draw_tracks")
    _assert_frames([draw_tracks(images[0], outs[0])], _restated([images[0]], [outs[0]], _style()), "the default style")


def test_track_frames_writes_the_frames(cuda, models, tmp_path):
    """--frames-out: four small JPEGs in, four decodable JPEGs of the frames' sizes out; the JSON lines are those of a run
    without the switch."""
    import io
    from PIL import Image
    from multiposenet_amd import track_frames
    frames = tmp_path / "frames"
    frames.mkdir()
    sizes = [(96, 128), (120, 100), (97, 131), (96, 128)]
    for i, (h, w) in enumerate(sizes):
        buf = io.BytesIO()
        Image.fromarray(np.random.RandomState(i).randint(0, 256, (h, w, 3)).astype(np.uint8)).save(buf, "JPEG", quality=90)
        (frames / f"frame_{i:03d}.jpg").write_bytes(buf.getvalue())
    paths = models["paths"]
    common = ["--images", str(frames), "--model", paths["k"], "--detector", paths["d"], "--prn", paths["p"], "--size", str(W), str(H),
              "--batch", "4", "--dtype", "f32", "--similarity", "iou", "--score-threshold", "0.0", "--new-track-score", "0.0"]
    track_frames.main(common + ["--out", str(tmp_path / "plain.jsonl")])
    out = tmp_path / "drawn"
    track_frames.main(common + ["--out", str(tmp_path / "drawn.jsonl"), "--frames-out", str(out), "--label-size", "12"])
    assert (tmp_path / "plain.jsonl").read_text() == (tmp_path / "drawn.jsonl").read_text()
    lines = [json.loads(ln) for ln in (tmp_path / "drawn.jsonl").read_text().splitlines()]
    assert len(lines) == 4 and all(any(ln["ids"]) for ln in lines)
    assert sorted(p.name for p in out.iterdir()) == [f"frame_{i:03d}.jpg" for i in range(4)]
    for i, (h, w) in enumerate(sizes):
        im = Image.open(out / f"frame_{i:03d}.jpg")
        im.load()
        assert im.format == "JPEG" and im.size == (w, h) and im.mode == "RGB"
