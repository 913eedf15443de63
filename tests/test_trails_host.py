"""CPU: the definition tests/trails_ref.py against results worked out by hand and, for the picture, against Pillow; the argument
checks of `trails.TrackTrails`; the size formulas and launcher checks of mpn_track_trails and mpn_draw_trails; and what `trails=`
adds to the Detector's signatures, keys and result layout."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import trails_cases as cases
import trails_ref as ref
from test_detector_options_host import B, H, W, THR, _detector, _key_of, _tracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, A, P, R = ref.FLAG_TRACKED, ref.FLAG_ANKLES, ref.FLAG_APPENDED, ref.FLAG_RESTARTED


def _run(name, streams=1):
    c = cases.BY_NAME[name]
    state = ref.new_state(streams, c['params']['length'])
    rows = ref.run(cases.reference_params(c['params']), cases.outputs_of(c['frames']), state, c['max_boxes'], c['total'])
    return c, rows, state


def _xs(row):
    return row['points'][:int(row['n']), 0].tolist()


# ---------------------------------------------------------------- the history, by hand
def test_every_and_the_gap_by_hand():
    """Person 1 stands at (20 + 5i, 40) in frame i + 1 and is not seen in frames 4 and 5; the counts of the frames are
    2 2 2 1 1 2 2 2 2 2, so its rows are 0, 2, 4, 8, 10, 12, 14, 16. every = 2: frame 1 keeps (20), frame 2 does not (2 - 1 < 2):
    C = 25 in front of the ring; frame 3 keeps 30 (3 - 1 >= 2); frame 6 keeps 45 (6 - 3 >= 2); frame 7 does not; frame 8 keeps 55."""
    _, rows, state = _run('every_2')
    mine = rows[[0, 2, 4, 8, 10, 12, 14, 16]]
    assert [_xs(r) for r in mine[:6]] == [[20], [25, 20], [30, 20], [45, 30, 20], [50, 45, 30, 20], [55, 45, 30, 20]]
    assert mine['flags'].tolist() == [T | A | P, T | A, T | A | P, T | A | P, T | A, T | A | P, T | A, T | A | P]
    assert (mine['points'][:, :, 1][mine['points'][:, :, 0] != 0] == 40).all()
    slot = state[0]['slots'][0]
    assert (int(slot['id']), int(slot['last']), int(slot['last_append']), int(slot['count']), int(slot['head'])) == (1, 10, 10, 5, 4)
    assert int(state[0]['frames']) == 10
    _, rows, _ = _run('every_1')                                    # every frame is kept: 8 observations, a ring of 5
    assert _xs(rows[16]) == [65, 60, 55, 50, 45] and (rows['flags'][[0, 2, 4, 8, 10, 12, 14, 16]] == T | A | P).all()
    _, rows, _ = _run('every_5')                                    # length 2: frames 1 and 6 are kept, frame 10 is C + both
    assert _xs(rows[16]) == [65, 45, 20] and int(rows[16]['flags']) == T | A


def test_the_ring_wraps_by_hand():
    """12 observations at x = 20 + 7i through a ring of 5: head = 11 % 5 = 1 and the ring holds the last five, newest first."""
    _, rows, state = _run('wrap_twice')
    assert _xs(rows[11]) == [97, 90, 83, 76, 69] and rows['n'][:12].tolist() == [1, 2, 3, 4, 5] + [5] * 7
    slot = state[0]['slots'][0]
    assert (int(slot['count']), int(slot['head'])) == (5, 1) and slot['ring'][:, 0].tolist() == [90, 97, 69, 76, 83]
    _, rows, state = _run('length_1')
    assert [_xs(r) for r in rows[:4]] == [[20], [27], [34], [41]] and int(state[0]['slots'][0]['head']) == 0
    _, rows, _ = _run('length_64')
    assert rows['n'][:8].tolist() == [1, 2, 3, 4, 5, 6, 7, 1] and rows.dtype.itemsize == 8 * 66


def test_max_gap_by_hand():
    """max_gap = 2. Rows: frame 1: persons 1, 2, 3; frame 2: 3; frame 3: 1, 3; frame 4: 2, 1; frame 5: 2, 1, 3. Person 1 is back
    in frame 3, now - last = 2: no restart. Person 2 is back in frame 4, now - last = 3 > 2: its trail starts anew."""
    _, rows, _ = _run('max_gap_2')
    assert rows['n'][:11].tolist() == [1, 1, 1, 2, 2, 3, 1, 3, 2, 4, 4]
    assert int(rows[4]['flags']) == T | A | P and int(rows[6]['flags']) == T | A | P | R and _xs(rows[6]) == [64]
    assert _xs(rows[8]) == [68, 64] and not (rows['flags'][[0, 1, 2, 3, 4, 5, 7, 8, 9, 10]] & R).any()
    _, rows, _ = _run('max_gap_0')                                  # never
    assert rows['n'][:11].tolist() == [1, 1, 1, 2, 2, 3, 2, 3, 3, 4, 4] and not (rows['flags'] & R).any()
    assert _xs(rows[8]) == [68, 64, 60]


def test_anchors_and_untracked_rows_by_hand():
    """zones_cases' persons: the ankles at (x, y), the box's bottom centre at (x + 4, y + 8), its centre at (x + 4, y - 16)."""
    _, rows, _ = _run('ankles')     # the right ankle alone (30, 30); the box (64, 58); the mean of both (30, 40)
    assert rows['points'][:3, 0].tolist() == [[30, 30], [64, 58], [30, 40]] and rows['flags'][:3].tolist() == [T | A | P, T | P, T | A | P]
    _, rows, _ = _run('box_centre')
    assert rows['points'][:2, 0].tolist() == [[34, 24], [34, 64]] and (rows['flags'][:4] == T | P).all()
    _, rows, _ = _run('box_bottom')
    assert rows['points'][:2, 0].tolist() == [[34, 48], [34, 88]]
    _, rows, state = _run('nan_keypoint')                           # frame 2: person 1 has no anchor and its slot is not touched
    assert int(rows[2]['flags']) == ref.FLAG_NO_ANCHOR and int(rows[2]['n']) == 0 and not rows[2]['points'].any()
    assert _xs(rows[4]) == [410, 390] and int(state[0]['slots'][0]['count']) == 3
    _, rows, state = _run('f32_overflow')                           # finite in f64, infinite in f32: no anchor either
    assert rows['flags'][:4].tolist() == [T | P, ref.FLAG_NO_ANCHOR, T | A | P, T | P] and _xs(rows[3]) == [44, 24]
    _, rows, state = _run('untracked')                              # ids 0 and -1: one point, no state; id 5 has a trail
    assert rows['n'][:6].tolist() == [1, 1, 1, 1, 1, 2] and rows['flags'][:6].tolist() == [A, A, T | A | P, A, A, T | A | P]
    assert [int(s['id']) for s in state[0]['slots'][:2]] == [5, 0]
    _, rows, _ = _run('duplicate_id')                               # the second row with the id is untracked
    assert rows['flags'][:4].tolist() == [T | A | P, A, T | A | P, A] and rows['n'][:4].tolist() == [1, 1, 2, 1]
    _, rows, state = _run('empty_frame')
    assert int(state[0]['frames']) == 4 and rows['n'][:3].tolist() == [1, 2, 0]
    _, rows, _ = _run('total_clamped')                              # total 4 of 3 + 3 rows: the second frame has one
    assert rows['n'][:6].tolist() == [1, 1, 1, 2, 0, 0]


def test_eviction_follows_the_zones_rule():
    _, rows, state = _run('evict_all')
    ids = [int(s['id']) for s in state[0]['slots']]
    assert sorted(ids)[:10] == [1, 8, 15, 22, 29, 36, 43, 50, 57, 64] and (rows['n'][:64 + 64 + 10] == 1).all()
    _, rows, state = _run('evict_stale')
    last = rows[20 + 25 + 30:20 + 25 + 30 + 5]                      # frame 4: 12 known, 6 new, 13 new (its slot went to 6), 1 known (a ring of 2), 231 new
    assert last['n'].tolist() == [2, 1, 1, 2, 1]


def test_two_calls_are_one():
    """The reference itself carries its state: the frames in two calls give the rows and the state of one call."""
    c, rows, state = _run('every_2')
    outputs = cases.outputs_of(c['frames'])
    again = ref.new_state(1, c['params']['length'])
    p = cases.reference_params(c['params'])
    first, second = ref.run(p, outputs[:4], again, c['max_boxes']), ref.run(p, outputs[4:], again, c['max_boxes'])
    got = np.concatenate([first[:7], second[:11]])
    assert got.tobytes() == rows[:18].tobytes() and again.tobytes() == state.tobytes()


# ---------------------------------------------------------------- the picture against Pillow
def _pillow(rgba, image, setting):
    from PIL import Image, ImageDraw
    im = Image.fromarray(rgba[..., :3].copy(), 'RGB')
    draw = ImageDraw.Draw(im, 'RGBA')
    t = image['trails']
    K = setting['length']
    for pts, n, tracked, tid in zip(t['points'], t['count'], t['tracked'], image['track_ids']):
        if not tracked or n < 2 or tid <= 0:
            continue
        ink = cases.palette_of(setting)[(int(tid) - 1) % len(cases.palette_of(setting))]
        for s in range(int(n) - 2, -1, -1):
            older, newer = (float(pts[s + 1][0]), float(pts[s + 1][1])), (float(pts[s][0]), float(pts[s][1]))
            draw.line([older, newer], fill=tuple(ink) + (ref.segment_alpha(s, K, setting['fade'], setting['min_alpha']),), width=1)
    out = np.full(rgba.shape, 255, np.uint8)
    out[..., :3] = np.asarray(im)
    return out


@pytest.mark.parametrize("index", range(len(cases.SETTINGS)))
def test_the_restatement_draws_what_pillow_draws(index):
    setting = cases.SETTINGS[index]
    drawn = 0
    for k, image in enumerate(cases.draw_images(setting)):
        before = cases.background(image['h'], image['w'], k)
        got = ref.draw(before.copy(), image['trails'], image['track_ids'], setting['length'], cases.palette_of(setting),
                       setting['fade'], setting['min_alpha'])
        want = _pillow(before, image, setting)
        np.testing.assert_array_equal(got, want, err_msg=f"{setting} {image['name']}")
        drawn += int((got != before).any())
    assert drawn >= 6                                               # the cases do draw


def test_every_fade_case_blends_a_pixel_twice():
    """Segments are applied in order: the joint pixel of two neighbours, and every crossing, is blended once per segment. With
    a ring of one point a trail is one segment: there the two crossing trails of the handmade set share a pixel."""
    for setting in cases.SETTINGS:
        for image in cases.draw_images(setting):
            if not image['name'].endswith('#0'):
                continue
            touched = {}
            ref.draw(cases.background(image['h'], image['w']), image['trails'], image['track_ids'], setting['length'],
                     cases.palette_of(setting), setting['fade'], setting['min_alpha'], touched)
            assert max(touched.values()) >= 2, (setting, image['name'])
    # and twice is not once: BLEND8(64, BLEND8(64, 200, 0), 0) = 112, BLEND8(64, 200, 0) = 150
    once = ref.blend8(64, 200, 0)
    assert (once, ref.blend8(64, once, 0)) == (150, 112)
    assert [ref.segment_alpha(s, 5, True, 64) for s in range(5)] == [255, 208, 160, 112, 64]
    assert [ref.segment_alpha(s, 1, True, 0) for s in range(2)] == [255, 0] and ref.segment_alpha(3, 5, False, 0) == 255
    assert ref.trunc(-0.9) == 0 and ref.trunc(1e12) == 1 << 29 and ref.trunc(float('nan')) == -(1 << 29) and ref.trunc(-7.5) == -7


# ---------------------------------------------------------------- the front end
def test_every_refusal_of_the_class():
    from multiposenet_amd.trails import TrackTrails
    ok = dict(frame_size=(480, 640))
    for bad, message in ((dict(streams=0), "streams must be an integer >= 1"),
                         (dict(streams=True), "streams must be an integer >= 1"),
                         (dict(max_boxes=65), "max_boxes must be an integer in 1..64 \\(got 65\\)"),
                         (dict(max_boxes=0), "max_boxes must be an integer in 1..64"),
                         (dict(frame_size=None), "frame_size must be \\(height, width\\)"),
                         (dict(frame_size=(0, 640)), "frame_size must be two positive numbers"),
                         (dict(frame_size=(480, float('inf'))), "frame_size must be two positive numbers"),
                         (dict(length=0), "length must be an integer in 1..64 \\(got 0\\)"),
                         (dict(length=65), "length must be an integer in 1..64"),
                         (dict(length=2.5), "length must be an integer"),
                         (dict(every=0), "every must be an integer in 1..255"),
                         (dict(every=256), "every must be an integer in 1..255"),
                         (dict(max_gap=-1), "max_gap must be an integer in 0..65535"),
                         (dict(max_gap=65536), "max_gap must be an integer in 0..65535"),
                         (dict(anchor='head'), "anchor must be one of \\['feet', 'box_bottom', 'box_centre'\\] \\(got 'head'\\)"),
                         (dict(min_keypoint_score=float('nan')), "min_keypoint_score must be finite"),
                         (dict(min_keypoint_score='x'), "min_keypoint_score must be a number"),
                         (dict(draw=1), "draw must be False or True"),
                         (dict(fade='yes'), "fade must be False or True"),
                         (dict(min_alpha=-1), "min_alpha must be an integer in 0..255"),
                         (dict(min_alpha=256), "min_alpha must be an integer in 0..255"),
                         (dict(palette=5), "palette must be a sequence"),
                         (dict(palette=[]), "palette must hold 1..256 colours \\(got 0\\)"),
                         (dict(palette=[(0, 0, 0)] * 257), "palette must hold 1..256 colours"),
                         (dict(palette=[(0, 0, 256)]), "palette\\[0\\] must lie in 0..255"),
                         (dict(palette=[(0, 0.5, 0)]), "palette\\[0\\] must be \\(r, g, b\\) integers")):
        with pytest.raises(ValueError, match="TrackTrails: " + message):
            TrackTrails(**dict(ok, **bad))


def test_abi_sizes_and_the_table():
    from multiposenet_amd import _lib, trails
    lib = _lib.lib()
    for K in (1, 2, 5, 32, 64):
        assert lib.mpn_track_trails_state_bytes(1, K) == trails.state_dtype(K).itemsize == 16 + 64 * (32 + 8 * K)
        assert lib.mpn_track_trails_state_bytes(3, K) == 3 * (16 + 64 * (32 + 8 * K))
        assert lib.mpn_track_trails_out_bytes(4, 25, K) == 4 * 25 * trails.row_dtype(K).itemsize == 4 * 25 * 8 * (K + 2)
        assert trails.state_dtype(K) == ref.state_dtype(K) and trails.row_dtype(K) == ref.row_dtype(K)
        assert lib.mpn_draw_trails_workspace_bytes(4, 25, K) == 4 * 25 * (48 * K + 32)
    assert lib.mpn_track_trails_out_bytes(64, 64, 64) == 4096 * 8 * 66 and lib.mpn_draw_trails_workspace_bytes(32, 128, 64) > 0
    for bad in ((0, 5), (4097, 5), (1, 0), (1, 65)):
        assert lib.mpn_track_trails_state_bytes(*bad) == 0
    for bad in ((0, 8, 5), (4, 0, 5), (4, 65, 5), (128, 64, 5), (4, 8, 0), (4, 8, 65)):
        assert lib.mpn_track_trails_out_bytes(*bad) == 0
    for bad in ((0, 8, 5), (4, 0, 5), (4, 129, 5), (64, 128, 5), (4, 8, 0), (4, 8, 65)):
        assert lib.mpn_draw_trails_workspace_bytes(*bad) == 0
    assert [lib.mpn_draw_trails_tables_bytes(p) for p in (0, 1, 4, 5, 256, 257)] == [0, 32, 32, 48, 16 + 1024, 0]
    table = trails.draw_table(((1, 2, 3), (255, 0, 128)), True, 64, 5).view(np.int32)
    assert table[:6].tolist() == [1, 64, 5, 2, 1 | 2 << 8 | 3 << 16, 255 | 128 << 16] and table.nbytes == 32
    assert trails.draw_table(((1, 2, 3),), False, 0, 64).view(np.int32)[:4].tolist() == [0, 0, 64, 1]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    for name, count in (("mpn_track_trails", 17), ("mpn_draw_trails", 15)):
        decl = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl and len(decl.group(1).split(",")) == count == len(_lib.SIGNATURES[name][1])
    assert "#define MPN_DRAW_TRAILS_TABLE_HEADER_BYTES 16" in text


def test_the_history_launcher_checks_before_any_hip_call():
    from multiposenet_amd import _lib
    V = ctypes.c_void_p
    good = dict(record=V(0x1000), track_rows=V(0x2000), B=4, max_boxes=8, streams=2, length=5, every=1, max_gap=30, anchor=0,
                score=0.0, height=480.0, width=640.0, with_keypoints=1, prev=V(0x4000), next=V(0x5000), out=V(0x6000))

    def call(**change):
        a = dict(good, **change)
        return _lib.call("mpn_track_trails", a['record'], a['track_rows'], a['B'], a['max_boxes'], a['streams'], a['length'],
                         a['every'], a['max_gap'], a['anchor'], a['score'], a['height'], a['width'], a['with_keypoints'], a['prev'],
                         a['next'], a['out'], None)
    for name in ('record', 'track_rows', 'prev', 'next', 'out'):
        with pytest.raises(ValueError, match="BAD_ARG.*track_trails: null pointer"):
            call(**{name: None})
    with pytest.raises(ValueError, match="BAD_ARG.*track_trails:.*pure function"):
        call(next=V(0x4000))
    for bad, message in ((dict(length=0), "length"), (dict(length=65), "length"), (dict(every=0), "every"), (dict(every=256), "every"),
                         (dict(max_gap=-1), "max_gap"), (dict(max_gap=65536), "max_gap"),
                         (dict(height=float('nan')), "finite"), (dict(width=float('inf')), "finite"), (dict(score=float('-inf')), "finite")):
        with pytest.raises(ValueError, match="BAD_ARG.*track_trails: .*" + message):
            call(**bad)
    for bad in (dict(streams=0), dict(streams=3), dict(B=0)):
        with pytest.raises(ValueError, match="BAD_SHAPE.*track_trails:.*whole number of frames"):
            call(**bad)
    for bad in (dict(max_boxes=0), dict(max_boxes=65), dict(B=128, max_boxes=64)):
        with pytest.raises(ValueError, match="BAD_SHAPE.*track_trails: B = "):
            call(**bad)
    for bad in (dict(record=V(0x1008)), dict(track_rows=V(0x2004)), dict(prev=V(0x4004)), dict(next=V(0x5004)), dict(out=V(0x6004))):
        with pytest.raises(ValueError, match="BAD_ALIGN.*track_trails:"):
            call(**bad)


def test_the_drawing_launcher_checks_before_any_hip_call():
    from multiposenet_amd import _lib
    V = ctypes.c_void_p
    lib = _lib.lib()
    record_bytes, work_bytes = lib.mpn_pose_gather_record_bytes(4, 8), lib.mpn_draw_trails_workspace_bytes(4, 8, 5)
    good = dict(descs=V(0x1000), record=V(0x2000), record_bytes=record_bytes, track_rows=V(0x3000), trail_rows=V(0x4000),
                tables=V(0x5000), tables_bytes=64, B=4, max_boxes=8, length=5, out=V(0x6000), out_bytes=1 << 20, work=V(0x7000),
                work_bytes=work_bytes)

    def call(**change):
        a = dict(good, **change)
        return _lib.call("mpn_draw_trails", a['descs'], a['record'], a['record_bytes'], a['track_rows'], a['trail_rows'], a['tables'],
                         a['tables_bytes'], a['B'], a['max_boxes'], a['length'], a['out'], a['out_bytes'], a['work'], a['work_bytes'],
                         None)
    for name in ('descs', 'record', 'track_rows', 'trail_rows', 'tables', 'out', 'work'):
        with pytest.raises(ValueError, match="BAD_ARG.*draw_trails: null pointer"):
            call(**{name: None})
    for bad in (dict(B=0), dict(B=65536), dict(max_boxes=0), dict(max_boxes=129), dict(B=64, max_boxes=128), dict(length=0),
                dict(length=65)):
        with pytest.raises(ValueError, match="BAD_SHAPE.*draw_trails:"):
            call(**bad)
    for bad in (dict(descs=V(0x1008)), dict(record=V(0x2008)), dict(out=V(0x6008)), dict(work=V(0x7008)), dict(track_rows=V(0x3002)),
                dict(trail_rows=V(0x4002)), dict(tables=V(0x5002))):
        with pytest.raises(ValueError, match="BAD_ALIGN.*draw_trails:"):
            call(**bad)
    for bad in (dict(record_bytes=record_bytes - 1), dict(work_bytes=work_bytes - 1), dict(out_bytes=15), dict(tables_bytes=15)):
        with pytest.raises(_lib.MpnError, match="WORKSPACE.*draw_trails:"):
            call(**bad)


# ---------------------------------------------------------------- the Detector
def _trails(streams=1, max_boxes=25, frame_size=(H, W), serial=13, length=32):
    from multiposenet_amd import trails
    t = object.__new__(trails.TrackTrails)
    t.streams, t.max_boxes, t.device, t.serial, t.length = streams, max_boxes, 'cpu', serial, length
    t.frame_size = (float(frame_size[0]), float(frame_size[1]))
    t.row = trails.row_dtype(length)
    return t


def _counter(serial=11):
    from multiposenet_amd.zones import ZoneCounter
    c = object.__new__(ZoneCounter)
    c.streams, c.max_boxes, c.device, c.serial, c.frame_size = 1, 25, 'cpu', serial, (float(H), float(W))
    return c


def test_public_names_and_keywords():
    from multiposenet_amd import inference
    from multiposenet_amd.inference.detector import _Options
    from multiposenet_amd.trails import TrackTrails, draw_trails
    assert inference.TrackTrails is TrackTrails and inference.draw_trails is draw_trails
    parameters = inspect.signature(TrackTrails).parameters
    assert list(parameters) == ['streams', 'frame_size', 'length', 'every', 'max_gap', 'anchor', 'min_keypoint_score', 'draw', 'fade',
                                'min_alpha', 'palette', 'max_boxes', 'device']
    assert [parameters[k].default for k in parameters] == [1, None, 32, 1, 30, 'feet', 0.0, True, True, 64, None, 25, None]
    for method in ('predict_batch', 'predict_images', 'predict_jpegs'):
        sig = inspect.signature(getattr(inference.Detector, method)).parameters
        assert list(sig)[-3:] == ['trails', 'zones', 'track_eval'] and sig['trails'].default is None, method
    assert 'trails' not in inspect.signature(inference.Detector.__call__).parameters
    assert _Options._fields[-4:] == ('trails', 'zones', 'anonymize', 'pose_nms')
    for name in ('check_batch', 'out_bytes', 'launch', 'launch_draw', 'commit', 'reset', 'unpack', 'update'):
        assert callable(getattr(TrackTrails, name))
    with pytest.raises(ValueError, match="draw_trails: trails must be a trails.TrackTrails"):
        draw_trails(np.zeros((4, 4, 3), np.uint8), {}, None)


@pytest.mark.parametrize("use_graph", [True, False])
def test_entry_keys_with_trails_and_without(use_graph):
    from multiposenet_amd.inference import Anonymize
    det = _detector(use_graph)
    trk, trails, counter = _tracker(), _trails(), _counter()
    batch = np.zeros((B, H, W, 3), np.uint8)
    frames = [np.zeros((H, W, 3), np.uint8)] * B
    base = (B, H, W, THR) if use_graph else ('eager', B, H, W)
    assert _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, trails=None) == base + ('track', 7, B)
    assert _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, trails=trails) == base + ('track', 7, B, 'trails', 13)
    spec = Anonymize()
    key = _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, trails=trails, zones=counter, annotate=True, anonymize=spec)
    assert key == base + ('annotate', 'track', 7, B, 'zones', 11, 'trails', 13, 'anonymize', spec)
    key = _key_of(det.predict_images, frames, size=(H, W), score_threshold=THR, track=trk, trails=trails)
    assert key[:5] == ('images', B, H, W, THR) and key[6:] == ('track', 7, B, 'trails', 13)
    with pytest.raises(ValueError, match="trails= follows the tracker's identities: it needs track="):
        det.predict_batch(batch, trails=trails)
    with pytest.raises(ValueError, match="must be None or a trails.TrackTrails"):
        det.predict_batch(batch, track=trk, trails=object())
    with pytest.raises(ValueError, match="trails were made for 2 streams, the tracker for 1"):
        det.predict_batch(batch, track=trk, trails=_trails(streams=2))
    with pytest.raises(ValueError, match="trails were made for max_boxes = 20, this Detector's is 25"):
        det.predict_batch(batch, track=trk, trails=_trails(max_boxes=20))
    with pytest.raises(ValueError, match=f"pixels of 480 x 640 frames.*a frame of {H} x {W}"):
        det.predict_batch(batch, track=trk, trails=_trails(frame_size=(480, 640)))
    odd = [np.zeros((H, W, 3), np.uint8), np.zeros((H, W + 2, 3), np.uint8)]
    with pytest.raises(ValueError, match=f"pixels of {H} x {W} frames.*a frame of {H} x {W + 2}"):
        det.predict_images(odd, size=(H, W), track=trk, trails=trails)
    # trails is checked before zones and before anonymize
    with pytest.raises(ValueError, match="trails="):
        det.predict_batch(batch, trails=trails, zones=counter)
    with pytest.raises(ValueError, match="trails="):
        det.predict_batch(batch, trails=trails, anonymize=spec)


def test_record_layout_ends_with_the_trail_rows():
    from multiposenet_amd.inference.detector import RecordLayout
    trails, counter = _trails(length=5), _counter()
    base = lambda layout: (layout.record, layout.oks, layout.track, layout.nms)     # noqa: E731
    four = RecordLayout(4, 25)
    assert RecordLayout(4, 25, trails=None).astuple() == four.astuple()
    five = RecordLayout(4, 25, trails=trails)
    assert base(five) == base(four) and (five.track_eval, five.zones) == (four.track_eval, four.zones)
    assert five.trails.start % 16 == 0 and five.trails.start >= four.nms.stop
    assert five.trails.stop - five.trails.start == trails.out_bytes(4) == 4 * 25 * 8 * 7 and five.nbytes == five.trails.stop
    with_zones = RecordLayout(4, 25, zones=counter)
    six = RecordLayout(4, 25, zones=counter, trails=trails)
    assert base(six) + (six.track_eval, six.zones) == base(with_zones) + (with_zones.track_eval, with_zones.zones)
    assert six.trails.start % 16 == 0 and six.trails.start >= with_zones.zones.stop
    assert six.trails.stop - six.trails.start == trails.out_bytes(4)


def test_track_frames_has_the_switches(capsys):
    from multiposenet_amd import track_frames
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--help"])
    text = capsys.readouterr().out
    assert e.value.code == 0
    for switch in ("--trails [LENGTH]", "--trail-every N", "--trail-max-gap N", "--trail-anchor {feet,box_bottom,box_centre}",
                   "--no-trail-fade", "--no-trail-draw"):
        assert switch in text, switch
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--images", ".", "--trail-every", "2"])
    assert e.value.code == 2 and "need --trails" in capsys.readouterr().err
