"""CPU: the picture of `mpn_draw_tracks` - the numpy restatement tests/draw_tracks_ref.py against Pillow itself
(`ImageDraw.rectangle` / `line` / `ellipse` / `text` with `ImageFont.load_default(size)`), byte for byte, over a table of
cases; `TrackStyle`, its table for the kernels, and every argument check that needs no device. `case_table` is also the
input of tests/test_draw_tracks_gpu.py."""
import ctypes
import functools
import inspect

import numpy as np
import pytest

import draw_ref as R
import draw_tracks_ref as T
from multiposenet_amd import _lib
from multiposenet_amd.inference import TrackStyle, draw

F = np.float32
INT_MAX = 2147483647


def _box(h, w, x0, y0, x1, y1):
    """A normalised float32 box whose integer corners are exactly (x0, y0)-(x1, y1) in an h x w frame: every edge lies half
    a pixel inside its cell, toward zero."""
    half = lambda v: v + 0.5 if v >= 0 else v - 0.5                                          # noqa: E731
    return [F(half(y0) / h), F(half(x0) / w), F(half(y1) / h), F(half(x1) / w)]


def _case(name, rng, h, w, corners, ids, label=True, smoothed=None, positions=True, **style):
    boxes = np.array([_box(h, w, *c) for c in corners], F).reshape(-1, 4)
    n = len(boxes)
    outputs = {"boxes": boxes, "track_ids": np.array(ids, np.int32),
               "keypoint_positions": rng.uniform(-0.2, 1.2, (n, 17, 2)).astype(F) if positions else np.zeros((0, 17, 2), F)}
    if smoothed is not None:
        outputs["keypoints_smoothed"] = np.asarray(smoothed, F)
    image = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    return {"name": name, "image": image, "outputs": outputs, "style": TrackStyle(**style), "label": label}


@functools.lru_cache(maxsize=1)
def case_table():
    """The cases, from one seed. 'label': the case must show blended digit pixels inside the frame."""
    rng = np.random.RandomState(20240)
    wide = lambda lo, hi, n=1: np.concatenate([rng.uniform(lo, hi, (n, 17, 2)), rng.uniform(0, 1, (n, 17, 1))], axis=2)   # noqa: E731
    cases = []
    for size in (10, 16, 12):                                       # (at 12 the default font's 4 is wider than its advance)
        tag = f"size{size}"
        cases += [
            # one box per id length, each label above its box; the last is clipped at the right edge
            _case(f"{tag}/ids_above", rng, 120, 200, [(4, 30, 40, 60), (60, 30, 90, 70), (100, 90, 150, 110), (8, 90, 60, 118)],
                  [1, 10, 4096, INT_MAX], label_size=size),
            _case(f"{tag}/inside_at_top", rng, 64, 96, [(10, 3, 50, 40), (30, 0, 90, 30)], [7, 4096], label_size=size),
            _case(f"{tag}/clipped_left", rng, 64, 96, [(-9, 30, 40, 60)], [4096], label_size=size),
            _case(f"{tag}/clipped_right", rng, 64, 96, [(85, 30, 95, 60)], [INT_MAX], label_size=size),
            _case(f"{tag}/clipped_bottom", rng, 64, 96, [(20, 70, 60, 90), (50, 62, 80, 63)], [10, 1], label_size=size),
            # the second person's box and skeleton run through the first person's label
            _case(f"{tag}/crossed_by_later", rng, 90, 120, [(20, 40, 100, 80), (10, 20, 60, 36)], [4096, 2], label_size=size),
            _case(f"{tag}/untracked_plain", rng, 64, 96, [(10, 30, 50, 60), (40, 25, 90, 50)], [0, 3], label_size=size),
            _case(f"{tag}/untracked_hidden", rng, 64, 96, [(10, 30, 50, 60), (40, 25, 90, 50)], [0, 3], label_size=size,
                  untracked="hide"),
            _case(f"{tag}/flat_and_inverted", rng, 64, 96, [(10, 30, 50, 30), (60, 50, 40, 60), (20, 50, 50, 45)], [5, 6, 7],
                  label_size=size),
            _case(f"{tag}/smoothed", rng, 64, 96, [(10, 30, 50, 60), (40, 25, 90, 50)], [12, 0], label_size=size,
                  smoothed=np.concatenate([wide(-6.75, 40.0), wide(20.0, 99.5)]), keypoints="smoothed"),
            _case(f"{tag}/styled", rng, 64, 96, [(10, 30, 50, 60), (40, 33, 90, 50)], [3, 2], label_size=size,
                  palette=[(1, 2, 3), (250, 240, 0)], line_color=(0, 255, 0), text_color=(10, 20, 30)),
        ]
    cases += [
        _case("no_labels", rng, 64, 96, [(10, 30, 50, 60)], [9], label=False, labels=False),
        _case("all_untracked", rng, 64, 96, [(10, 30, 50, 60), (40, 25, 90, 50)], [0, 0], label=False),
        _case("boxes_only", rng, 64, 96, [(10, 30, 50, 60), (40, 25, 90, 50)], [13, 0], positions=False),
        _case("palette_wrap", rng, 40, 200, [(4, 20, 30, 30), (60, 20, 90, 30), (120, 20, 150, 30)], [12, 13, 25]),
        _case("tiny_frame", rng, 5, 7, [(1, 1, 5, 3)], [8]),
        _case("one_pixel", rng, 1, 1, [(0, 0, 0, 0)], [1], label=False),
    ]
    return cases


def _pillow(case):
    """The picture as Pillow draws it: rectangle / line / ellipse as the notebook calls them, the label as the issue's
    definition: a filled rectangle, then one `draw.text` per digit."""
    from PIL import Image, ImageDraw, ImageFont
    image, o, style = case["image"], case["outputs"], case["style"]
    h, w = image.shape[:2]
    font = ImageFont.load_default(size=style.label_size)
    stamps, cell = draw.digit_stamps(style.label_size)
    top, bot = draw.label_metrics(stamps, cell)
    assert cell == max(int(np.ceil(font.getlength(d))) for d in "0123456789")
    im = Image.fromarray(np.concatenate([image, np.full((h, w, 1), 255, np.uint8)], axis=2), "RGBA")
    d = ImageDraw.Draw(im)
    n = len(o["boxes"])
    for i, track_id in enumerate(int(t) for t in o["track_ids"]):
        if track_id == 0 and style.untracked == "hide":
            continue
        colour = style.palette[(track_id - 1) % len(style.palette)] if track_id else (255, 0, 0)
        line = style.line_color if track_id else (255, 255, 255)
        pos = o["keypoint_positions"][i:i + 1] if len(o["keypoint_positions"]) == n else np.zeros((0, 17, 2), F)
        (_, x0, y0, x1, y1), *rest = R.primitives(o["boxes"][i:i + 1], pos, h, w)
        try:
            d.rectangle([(x0, y0), (x1, y1)], outline=colour + (255,))
            drawn = True
        except ValueError:                                          # an inverted box: Pillow refuses it
            drawn = False
        if style.keypoints == "smoothed":                           # floats, as they are: Pillow truncates them
            kp = o["keypoints_smoothed"][i]
            for a, b in R.EDGES:
                d.line([(float(kp[a, 0]), float(kp[a, 1])), (float(kp[b, 0]), float(kp[b, 1]))], fill=line + (255,))
            for x, y in kp[:, :2]:
                d.ellipse([(float(F(x) - F(2)), float(F(y) - F(2))), (float(F(x) + F(2)), float(F(y) + F(2)))], fill=colour + (255,))
        else:
            for kind, *c in rest:
                if kind == R.LINE:
                    d.line([tuple(c[:2]), tuple(c[2:])], fill=line + (255,))
                else:
                    d.ellipse([tuple(c[:2]), tuple(c[2:])], fill=colour + (255,))
        if track_id and style.labels and drawn:
            digits = str(track_id)
            lw, lh = 2 + len(digits) * cell, 2 + (bot - top)
            lx0, ly0 = x0, (y0 - lh if y0 - lh >= 0 else y0)
            d.rectangle([lx0, ly0, lx0 + lw - 1, ly0 + lh - 1], fill=colour + (255,))
            for k, ch in enumerate(digits):
                d.text((lx0 + 1 + k * cell, ly0 + 1 - top), ch, fill=style.text_color + (255,), font=font)
    return np.asarray(im)


def _restated(case):
    stamps, cell = draw.digit_stamps(case["style"].label_size)
    return T.draw_tracks(case["image"], case["outputs"], case["style"], stamps, cell)


def test_restatement_equals_pillow_on_every_case():
    cases = case_table()
    assert len(cases) >= 25 and {c["style"].label_size for c in cases} >= {10, 16}
    for case in cases:
        got, want = _restated(case), _pillow(case)
        assert got.dtype == np.uint8 and got.shape == want.shape and (want[..., 3] == 255).all()
        diff = (got != want).any(axis=2)
        assert not diff.any(), (case["name"], int(diff.sum()), np.argwhere(diff)[:5].tolist())


def test_case_table_covers_what_it_claims():
    cases = {c["name"]: c for c in case_table()}
    ids = {int(t) for c in cases.values() for t in c["outputs"]["track_ids"]}
    assert {0, 1, 10, 4096, INT_MAX} <= ids
    for c in cases.values():                                        # no label case is vacuous: blended pixels inside the frame
        stamps, cell = draw.digit_stamps(c["style"].label_size)
        h, w = c["image"].shape[:2]
        blended = T.blended_label_pixels(c["outputs"], h, w, c["style"], stamps, cell)
        assert (blended > 0) == c["label"], (c["name"], blended)
    for size in (10, 16, 12):
        stamps, cell = draw.digit_stamps(size)
        _, _, _, lh = T.label_box(0, 0, 1, stamps, cell)

        def labels(name):
            c = cases[f"size{size}/{name}"]
            h, w = c["image"].shape[:2]
            prims = T.primitives(c["outputs"], h, w, c["style"], stamps, cell)
            return h, w, prims, [T.label_box(p[1], p[2], p[7], stamps, cell) for p in prims if p[0] == T.FILL]
        _, _, _, boxes = labels("ids_above")
        assert len(boxes) == 4 and all(ly0 >= 0 and ly0 + lh <= y0 for (_, ly0, _, _), y0 in zip(boxes, (30, 30, 90, 90)))
        _, _, prims, boxes = labels("inside_at_top")
        assert [b[1] for b in boxes] == [3, 0]                       # forced inside: the label starts on the box's top row
        _, w, _, boxes = labels("clipped_left")
        assert boxes[0][0] < 0 < boxes[0][0] + boxes[0][2]
        _, w, _, boxes = labels("clipped_right")
        assert boxes[0][0] < w < boxes[0][0] + boxes[0][2]
        h, _, _, boxes = labels("clipped_bottom")
        assert any(ly0 < h < ly0 + lh_ for _, ly0, _, lh_ in boxes)
        h, w, prims, boxes = labels("crossed_by_later")
        first = {(x, y) for x, y, _, _ in T.label_pixels(*[p for p in prims if p[0] == T.FILL][0][1:3], 4096, stamps, cell, T.RED, T.WHITE)}
        later = [p for p in prims if p[7] == 2]
        assert first & set(R.rect_pixels(*later[0][1:5])) and any(first & set(R.line_pixels(*p[1:5])) for p in later if p[0] == R.LINE)
        _, _, prims, boxes = labels("untracked_hidden")
        assert {p[7] for p in prims} == {3}
        _, _, prims, _ = labels("untracked_plain")
        assert {p[5] for p in prims if p[7] == 0} == {T.RED, T.WHITE}
        _, _, prims, boxes = labels("flat_and_inverted")
        rects = [p for p in prims if p[0] == R.RECT]
        assert len(rects) == 1 and rects[0][2] == rects[0][4] and len(boxes) == 1     # y1 == y0 drawn; both inverted ones not
        kp = cases[f"size{size}/smoothed"]["outputs"]["keypoints_smoothed"]
        assert (kp[..., :2] < 0).any() and (kp[..., :2] % 1 != 0).any()
    assert len(TrackStyle().palette) == 12 and {int(t) for t in cases["palette_wrap"]["outputs"]["track_ids"]} == {12, 13, 25}


def test_track_style_validates_and_is_immutable():
    s = TrackStyle()
    assert s.palette == draw.DEFAULT_PALETTE and len(s.palette) == 12 and (255, 0, 0) not in s.palette and (255, 255, 255) not in s.palette
    assert (s.labels, s.label_size, s.keypoints, s.untracked, s.line_color, s.text_color) == \
        (True, 10, "frame", "plain", (255, 255, 255), (255, 255, 255))
    assert list(inspect.signature(TrackStyle).parameters) == ["palette", "labels", "label_size", "keypoints", "untracked",
                                                              "line_color", "text_color"]
    assert s == TrackStyle(palette=list(draw.DEFAULT_PALETTE)) and hash(s) == hash(TrackStyle()) and s != TrackStyle(labels=False)
    assert len({TrackStyle(), TrackStyle(label_size=16), TrackStyle(untracked="hide"), TrackStyle()}) == 3
    for name in ("labels", "palette", "anything"):
        with pytest.raises(AttributeError):
            setattr(s, name, 1)
    with pytest.raises(AttributeError):
        del s.labels
    for bad, match in ((dict(palette=[]), "palette"), (dict(palette=[(0, 0, 0)] * 257), "palette"), (dict(palette=[(0, 0)]), "palette"),
                       (dict(palette=[(0, 0, 256)]), "palette"), (dict(palette=7), "palette"), (dict(labels="yes"), "labels"),
                       (dict(label_size=0), "label_size"), (dict(label_size=10.5), "label_size"), (dict(keypoints="raw"), "keypoints"),
                       (dict(untracked="show"), "untracked"), (dict(line_color=(1, 2)), "line_color"),
                       (dict(text_color=(-1, 0, 0)), "text_color"), (dict(text_color=(0.5, 0, 0)), "text_color")):
        with pytest.raises(ValueError, match=match):
            TrackStyle(**bad)
    with pytest.raises(ValueError, match="label_size"):              # digit cells beyond what the kernels take
        TrackStyle(label_size=200).tables()


def test_tables_layout():
    lib = _lib.lib()
    assert lib.mpn_draw_tracks_tables_bytes(12, 6, 8) == (232 + 48 + 10 * (6 + 2) * 8 + 15) // 16 * 16   # a glyph may be 2 wider than its cell
    for bad in ((0, 6, 8), (257, 6, 8), (12, 0, 8), (12, 33, 8), (12, 6, -1), (12, 6, 49)):
        assert lib.mpn_draw_tracks_tables_bytes(*bad) == 0
    assert lib.mpn_draw_tracks_tables_bytes(256, 32, 48) > 0
    for style in (TrackStyle(), TrackStyle(label_size=16, labels=False, untracked="hide", palette=[(1, 2, 3)], line_color=(4, 5, 6),
                                           text_color=(7, 8, 9))):
        stamps, cell = draw.digit_stamps(style.label_size)
        assert draw.digit_stamps(style.label_size)[0] is stamps      # rendered once per size
        top, bot = draw.label_metrics(stamps, cell)
        assert (top, bot) == T.metrics(stamps, cell) and 1 <= cell <= draw.MAX_CELL and 0 < bot - top <= draw.MAX_STAMP_H
        table = style.tables()
        assert table.dtype == np.uint8 and table.size == lib.mpn_draw_tracks_tables_bytes(len(style.palette), cell, bot - top)
        assert not table.flags.writeable
        words = table[:(draw.TABLE_HEADER_WORDS + len(style.palette)) * 4].view(np.int32)
        pack = lambda c: c[0] | c[1] << 8 | c[2] << 16                                          # noqa: E731
        assert words[0] == (1 if style.labels else 0) | (2 if style.untracked == "hide" else 0)
        assert words[1:8].tolist() == [pack(style.line_color), pack(style.text_color), len(style.palette), cell, top, bot, 0]
        assert words[58:].tolist() == [pack(c) for c in style.palette]
        end = words.nbytes
        for d, (mask, (ox, oy)) in enumerate(stamps):
            w_, h_, ox_, oy_, at = words[8 + 5 * d:13 + 5 * d].tolist()
            assert (w_, h_, ox_, oy_) == (mask.shape[1], mask.shape[0], ox, oy) and at == end
            np.testing.assert_array_equal(table[at:at + w_ * h_].reshape(h_, w_), mask)
            assert -1 <= ox_ and ox_ + w_ <= cell + 1 and top <= oy_ and oy_ + h_ <= bot       # inside the label's rectangle
            end = at + w_ * h_
        assert end <= table.size and not table[end:].any()
    with pytest.raises(ValueError, match="leaves its cell"):         # the builder refuses a stamp its label would not enclose
        draw.label_metrics([(np.zeros((8, 6), np.uint8), (2, 2))] * 10, 6)
    assert draw.label_metrics([(np.zeros((8, 8), np.uint8), (-1, 2))] * 10, 6) == (2, 10)    # the padding's width outside: enclosed


def test_draw_tracks_entry_point_validates_before_any_hip_call():
    lib = _lib.lib()
    P16 = ctypes.c_void_p(4096)
    call = _lib.call
    assert lib.mpn_draw_tracks_workspace_bytes(16, 25) == 16 * 25 * (35 * 32 + 16)             # + the label; 16 bytes of inks
    assert lib.mpn_draw_tracks_workspace_bytes(16, 25) > lib.mpn_draw_detections_workspace_bytes(16, 25)
    assert lib.mpn_draw_tracks_workspace_bytes(0, 25) == 0 and lib.mpn_draw_tracks_workspace_bytes(1, draw.MAX_BOXES + 1) == 0
    assert lib.mpn_draw_tracks_workspace_bytes(200, 25) == 0
    rec, work = lib.mpn_pose_gather_record_bytes(2, 25), lib.mpn_draw_tracks_workspace_bytes(2, 25)
    #       0    1        2    3    4    5    6     7    8    9  10  11 12   13       14   15    16
    good = [P16, 1 << 20, P16, P16, rec, P16, None, P16, 768, 2, 25, 1, P16, 1 << 20, P16, work, None]

    def args(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return a

    for i in (0, 2, 3, 5, 7, 12, 14):                                 # sources, descs, record, track_rows, tables, out, workspace
        with pytest.raises(ValueError, match="null"):
            call("mpn_draw_tracks", *args(**{f"a{i}": None}))
    with pytest.raises(ValueError, match="B must"):
        call("mpn_draw_tracks", *args(a9=0))
    with pytest.raises(ValueError, match="max_boxes must"):
        call("mpn_draw_tracks", *args(a10=0))
    with pytest.raises(ValueError, match="max_boxes must"):
        call("mpn_draw_tracks", *args(a10=draw.MAX_BOXES + 1))
    with pytest.raises(ValueError, match="rows"):
        call("mpn_draw_tracks", *args(a9=200))
    for i in (2, 3, 12, 14):
        with pytest.raises(ValueError, match="16-byte aligned"):
            call("mpn_draw_tracks", *args(**{f"a{i}": ctypes.c_void_p(4100)}))
    for i in (5, 6, 7):                                               # track_rows, smooth_rows, tables
        with pytest.raises(ValueError, match="4-byte aligned"):
            call("mpn_draw_tracks", *args(**{f"a{i}": ctypes.c_void_p(4098)}))
    with pytest.raises(_lib.MpnError, match="record of"):
        call("mpn_draw_tracks", *args(a4=rec - 1))
    with pytest.raises(_lib.MpnError, match="workspace of"):
        call("mpn_draw_tracks", *args(a15=lib.mpn_draw_detections_workspace_bytes(2, 25)))
    with pytest.raises(_lib.MpnError, match="out_rgba of"):
        call("mpn_draw_tracks", *args(a13=0))
    with pytest.raises(_lib.MpnError, match="tables of"):
        call("mpn_draw_tracks", *args(a8=231))


def test_detector_arguments_raise_before_any_device_work():
    from multiposenet_amd.inference import PoseTracker
    from multiposenet_amd.inference.detector import Detector, check_track_style
    det = object.__new__(Detector)
    tracker = object.__new__(PoseTracker)
    tracker.smooth = None
    batch = np.zeros((1, 128, 128, 3), np.uint8)
    style = TrackStyle()
    for method, first in ((det.predict_batch, batch), (det.predict_images, list(batch)), (det.predict_jpegs, [b"\xff\xd8"])):
        assert inspect.signature(method).parameters["track_style"].default is None
        with pytest.raises(ValueError, match="needs annotate"):
            method(first, track=tracker, track_style=style)
        with pytest.raises(ValueError, match="needs track="):
            method(first, annotate=True, track_style=style)
        with pytest.raises(ValueError, match="without smooth="):
            method(first, annotate="jpeg", track=tracker, track_style=TrackStyle(keypoints="smoothed"))
        with pytest.raises(ValueError, match="inference.TrackStyle"):
            method(first, annotate=True, track=tracker, track_style="colours")
    assert check_track_style(None, False, None) == () and check_track_style(style, True, tracker) == ("style", style)
    from multiposenet_amd.inference import draw_tracks
    ok = {"boxes": np.zeros((2, 4), F), "keypoint_positions": np.zeros((2, 17, 2), F), "track_ids": np.zeros(2, np.int32)}
    with pytest.raises(ValueError, match="image must be"):
        draw_tracks(np.zeros((4, 4), np.uint8), ok)
    with pytest.raises(ValueError, match="track_ids"):
        draw_tracks(np.zeros((4, 4, 3), np.uint8), dict(ok, track_ids=np.zeros(3, np.int32)))
    with pytest.raises(ValueError, match="keypoints_smoothed"):
        draw_tracks(np.zeros((4, 4, 3), np.uint8), ok, TrackStyle(keypoints="smoothed"))
    with pytest.raises(ValueError, match="TrackStyle"):
        draw_tracks(np.zeros((4, 4, 3), np.uint8), ok, style="red")


def test_track_frames_help_lists_the_new_switches(capsys):
    from multiposenet_amd import track_frames
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for switch in ("--frames-out", "--jpeg-quality", "--label-size", "--draw-smoothed", "--hide-untracked"):
        assert switch in text, switch
