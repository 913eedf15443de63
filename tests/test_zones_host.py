"""CPU: the definition tests/zones_ref.py against results worked out by hand, the argument checks of `zones.ZoneCounter`, the size
formulas and launcher checks of mpn_zone_events, and what `zones=` adds to the Detector's signatures, keys and result layout."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import zones_cases as cases
import zones_ref as ref
from test_detector_options_host import B, H, W, THR, _detector, _key_of, _tracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(name, streams=1):
    c = cases.BY_NAME[name]
    state = ref.new_state(streams)
    persons, images = ref.run(cases.geometry(c['geo']), cases.outputs_of(c['frames']), state, c['max_boxes'], c['total'])
    return c, persons, images, state


# ---------------------------------------------------------------- the reference, by hand
def test_the_crossing_rule_on_boundaries_by_hand():
    """The square (10,10)-(50,50): for (30, 10) only the vertical edges count ((y1 > 10) != (y2 > 10)); the edge (50,10)->(50,50)
    goes down (y2 > y1) with t = 0 * (10 - 10) - (30 - 50) * 40 = 800 > 0: crossed; the edge (10,50)->(10,10) goes up with
    t = 0 - (30 - 10) * (-40) = 800, not < 0: not crossed. One crossing: inside. For (30, 50) no edge has an end with y > 50:
    outside. For (50, 30) the edge at x = 50 has t = 0: not crossed; the one at x = 10 has t = 1600, not < 0: outside."""
    sq = [(ref.f64(x), ref.f64(y)) for x, y in cases.SQUARE]
    inside = lambda x, y, poly=sq: ref.inside(poly, ref.f64(x), ref.f64(y))
    assert inside(30, 10) and not inside(30, 50) and inside(10, 30) and not inside(50, 30)
    assert inside(10, 10) and not inside(50, 10) and not inside(10, 50) and not inside(50, 50)      # the vertices
    assert inside(30, 30) and not inside(0, 10) and not inside(60, 50) and not inside(30, 9.5)
    tri = [(ref.f64(x), ref.f64(y)) for x, y in cases.TRIANGLE]
    # on the sloped edge (140,100)->(100,140), going down: t = -40 * (120 - 100) - (120 - 140) * 40 = 0: not crossed; the edge
    # (100,140)->(100,100), going up: t = 0 - 20 * (-40) = 800, not < 0: outside. Half a pixel to the left the first edge has
    # t = -800 - (119.5 - 140) * 40 = 20 > 0: crossed, inside
    assert not inside(120, 120, tri) and inside(119.5, 120, tri) and inside(100, 120, tri) and inside(100, 100, tri)
    u = [(ref.f64(x), ref.f64(y)) for x, y in cases.CONCAVE]
    assert not inside(250, 70, u) and inside(220, 70, u) and inside(280, 70, u) and inside(250, 20, u) and inside(250, 39, u)
    _, persons, images, _ = _run('boundary')
    assert persons['inside'][:14].tolist() == [1, 0, 1, 0, 0, 0, 0, 1, 0, 2, 2, 0, 0, 2]
    assert images['occupancy'][0][:3].tolist() == [3, 3, 0]


def test_line_crossings_by_hand():
    """The gate from (400, 0) to (400, 100): d(X) = 0 * (Xy - 0) - 100 * (Xx - 400), positive left of x = 400."""
    gate = ((ref.f64(400), ref.f64(0)), (ref.f64(400), ref.f64(100)))
    cross = lambda a, c: ref.crossing(gate, tuple(map(ref.f64, a)), tuple(map(ref.f64, c)))
    assert cross((390, 50), (410, 50)) == -1 and cross((410, 50), (390, 50)) == 1
    assert cross((390, 50), (400, 50)) == -1 and cross((400, 50), (410, 50)) == 0      # ends on it: once, on arrival
    assert cross((410, 50), (400, 50)) == 0 and cross((400, 50), (390, 50)) == 1       # from the other side: once, on leaving
    assert cross((390, 100), (410, 100)) == 0 and cross((390, 0), (410, 0)) == -1      # through Q: e(Q) = 0; through P: e(P) = 0
    assert cross((400, 20), (400, 80)) == 0 and cross((390, 20), (390, 80)) == 0       # parallel
    assert cross((390, 150), (410, 150)) == 0 and cross((390, 50), (390, 50)) == 0     # past its end; no movement
    _, persons, images, state = _run('line_end_on')
    assert persons['crossed_negative'][:3].tolist() == [0, 1, 0] and not persons['crossed_positive'].any()
    assert int(state[0]['line_negative'][0]) == 1 and int(state[0]['line_positive'][0]) == 0
    _, persons, images, _ = _run('line_gap')                        # rows: frame 1 (2), frame 2 (1), frame 4 (1)
    assert persons['crossed_positive'][:4].tolist() == [0, 0, 0, 1] and images['total_positive'][:, 0].tolist() == [0, 0, 0, 1]


def test_debounce_and_dwell_by_hand():
    """The anchor of one person over 8 frames: in in in out in out out out."""
    rows = {n: _run(f'flicker_{n}')[1][:8] for n in (1, 2, 3)}
    bit = lambda field, n: [int(v) & 1 for v in rows[n][field]]
    assert bit('inside', 1) == [1, 1, 1, 0, 1, 0, 0, 0] and bit('entered', 1) == [1, 0, 0, 0, 1, 0, 0, 0]
    assert bit('exited', 1) == [0, 0, 0, 1, 0, 1, 0, 0] and rows[1]['dwell'][:, 0].tolist() == [1, 2, 3, 0, 1, 0, 0, 0]
    assert bit('inside', 2) == [0, 1, 1, 1, 1, 1, 0, 0] and bit('entered', 2) == [0, 1, 0, 0, 0, 0, 0, 0]
    assert bit('exited', 2) == [0, 0, 0, 0, 0, 0, 1, 0] and rows[2]['dwell'][:, 0].tolist() == [0, 1, 2, 3, 4, 5, 0, 0]
    assert bit('inside', 3) == [0, 0, 1, 1, 1, 1, 1, 0] and bit('entered', 3) == [0, 0, 1, 0, 0, 0, 0, 0]
    assert bit('exited', 3) == [0, 0, 0, 0, 0, 0, 0, 1] and rows[3]['dwell'][:, 0].tolist() == [0, 0, 1, 2, 3, 4, 5, 0]


def test_anchors_identities_and_eviction_by_hand():
    _, persons, _, _ = _run('ankles')
    assert persons['flags'][:3].tolist() == [3, 1, 3] and persons['anchor'][0].tolist() == [30.0, 30.0]
    assert persons['anchor'][2].tolist() == [30.0, 40.0] and np.abs(persons['anchor'][1] - (64, 58)).max() < 1e-5
    _, persons, images, state = _run('nan_keypoint')                # rows: 2, 2, 2, 1
    assert persons['flags'][2] == ref.FLAG_NO_ANCHOR and not persons[2]['anchor'].any() and persons['inside'][2] == 0
    assert persons['crossed_negative'][4] == 1 and persons['crossed_positive'][6] == 1      # frame 3 against frame 1's anchor
    _, persons, images, state = _run('id_change')
    assert [int(v) for v in persons['entered'][:4]] == [1, 0, 1, 0] and not persons['exited'].any()
    assert persons['dwell'][:4, 0].tolist() == [1, 2, 1, 2] and int(state[0]['zone_entries'][0]) == 2
    _, persons, images, state = _run('untracked')
    assert persons['flags'][:3].tolist() == [2, 2, 3] and persons['inside'][:3].tolist() == [1, 2, 1]
    assert not persons['dwell'][:2].any() and images['occupancy'][0][:2].tolist() == [2, 1] and images['entries'][0][0] == 1
    _, persons, images, state = _run('empty_frame')
    assert int(state[0]['frames']) == 4 and images['total_exits'][:, 0].tolist() == [0, 0, 1, 1]
    _, persons, images, state = _run('duplicate_id')
    assert persons['flags'][:4].tolist() == [3, 2, 3, 2]
    _, persons, images, state = _run('total_clamped')               # the second frame has one row: person 1, who left
    assert persons['flags'][:5].tolist() == [3, 3, 3, 3, 0] and images['occupancy'][1][0] == 0 and images['exits'][1][0] == 1
    _, persons, images, state = _run('evict_all')
    slots = state[0]['slots']
    assert sorted(slots['id'].tolist()) == sorted(list(range(1, 65, 7)) + [101 + i for i in range(10, 64)])
    assert slots['id'][:10].tolist() == list(range(1, 65, 7))       # the third frame's ids took the lowest of 64 equally stale slots
    assert images['entries'][:, 0].tolist() == [32, 64, 10, 0]
    _, persons, images, state = _run('evict_stale')
    slots = state[0]['slots']
    assert slots['id'][:5].tolist() == [1, 2, 3, 4, 5] and slots['id'][5:11].tolist() == [225, 226, 227, 228, 229, 230]
    assert slots['id'][40:64].tolist() == list(range(201, 225))     # the unused slots went first
    assert slots['id'][11:15].tolist() == [12, 6, 13, 231] and slots['last'][11:15].tolist() == [4, 4, 4, 4]
    full = _run('full')
    assert full[1]['inside'].any() and full[3][0]['line_positive'].sum() + full[3][0]['line_negative'].sum() > 0
    assert full[3][0]['zone_entries'].sum() > 0 and len(full[0]['geo']['zones']) == 16 and len(full[0]['geo']['lines']) == 16
    assert all(len(v) == 16 for v in full[0]['geo']['zones'].values())


def test_splitting_the_frames_changes_nothing():
    for name in ('flicker_2', 'line_gap', 'evict_stale'):
        c, persons, images, state = _run(name)
        outputs, geo = cases.outputs_of(c['frames']), cases.geometry(c['geo'])
        parts = ref.new_state(1)
        first = ref.run(geo, outputs[:2], parts, c['max_boxes'])
        second = ref.run(geo, outputs[2:], parts, c['max_boxes'])
        assert ref.pack_state(parts) == ref.pack_state(state)
        assert np.concatenate([first[1], second[1]]).tobytes() == images.tobytes()


# ---------------------------------------------------------------- the front end
def test_every_refusal_of_the_counter():
    from multiposenet_amd.zones import ZoneCounter, build_table
    ok = dict(frame_size=(480, 640), zones={'a': cases.SQUARE})
    tri = [(0, 0), (1, 0), (0, 1)]
    for bad, message in ((dict(zones=[tri] * 17), "zones must hold at most 16 entries \\(got 17\\)"),
                         (dict(zones=None, lines=[cases.GATE] * 17), "lines must hold at most 16"),
                         (dict(zones=None), "zones or lines must be given"),
                         (dict(zones={}, lines=[]), "zones or lines must be given"),
                         (dict(zones={'a': [(0, 0), (1, float('nan')), (0, 1)]}), "zone 'a' must have finite coordinates"),
                         (dict(lines={'g': ((0, 0), (float('inf'), 1))}), "line 'g' must have finite coordinates"),
                         (dict(lines={'g': ((5, 5), (5, 5))}), "line 'g' must have two different end points"),
                         (dict(zones={'a': tri[:2]}), "zone 'a' must be 3..16 \\(x, y\\) points"),
                         (dict(zones={'a': [(i, i * i) for i in range(17)]}), "zone 'a' must be 3..16"),
                         (dict(lines={'g': tri}), "line 'g' must be 2 \\(x, y\\) points"),
                         (dict(min_frames=0), "min_frames must be an integer in 1..255 \\(got 0\\)"),
                         (dict(min_frames=256), "min_frames must be an integer in 1..255"),
                         (dict(min_frames=1.5), "min_frames must be an integer"),
                         (dict(anchor='head'), "anchor must be one of \\['feet', 'box_bottom', 'box_centre'\\] \\(got 'head'\\)"),
                         (dict(min_keypoint_score=float('nan')), "min_keypoint_score must be finite"),
                         (dict(frame_size=None), "frame_size must be \\(height, width\\)"),
                         (dict(frame_size=(0, 640)), "frame_size must be two positive numbers"),
                         (dict(streams=0), "streams must be an integer >= 1"),
                         (dict(max_boxes=65), "max_boxes must be an integer in 1..64")):
        with pytest.raises(ValueError, match="ZoneCounter: " + message):
            ZoneCounter(**dict(ok, **bad))
    table, zone_names, line_names = build_table((480, 640), {'a': cases.SQUARE, 'b': cases.CONCAVE}, [cases.GATE], 'box_centre', 3, 0.25)
    t = table[0]
    assert (t['num_zones'], t['num_lines'], t['min_frames'], t['anchor']) == (2, 1, 3, 2) and zone_names == ['a', 'b'] and line_names == ['0']
    assert (t['height'], t['width'], t['min_keypoint_score']) == (480.0, 640.0, 0.25) and t['vertex_count'][:3].tolist() == [4, 8, 3]
    assert t['vertices'][1, 7].tolist() == [200.0, 100.0] and t['lines'][0].tolist() == [[400.0, 0.0], [400.0, 100.0]]


def test_abi_sizes():
    from multiposenet_amd import _lib, zones
    lib = _lib.lib()
    assert lib.mpn_zone_table_bytes() == zones.TABLE.itemsize == 16 + 24 + 64 + 16 * 16 * 16 + 16 * 32
    assert lib.mpn_zone_state_bytes(1) == zones.STATE.itemsize == 4 * (4 + 64 + 64 * 28) and lib.mpn_zone_state_bytes(3) == 3 * 7440
    assert zones.SLOT.itemsize == 112 and lib.mpn_zone_state_bytes(0) == 0 and lib.mpn_zone_state_bytes(4097) == 0
    assert lib.mpn_zone_out_bytes(4, 25) == 4 * 25 * zones.PERSON.itemsize + 4 * zones.IMAGE.itemsize
    assert lib.mpn_zone_out_bytes(1, 1) == 104 + 576 and lib.mpn_zone_out_bytes(64, 64) == 64 * 64 * 104 + 64 * 576
    for bad in ((0, 8), (4, 0), (4, 65), (128, 64)):
        assert lib.mpn_zone_out_bytes(*bad) == 0
    assert zones.PERSON == ref.PERSON and zones.IMAGE == ref.IMAGE and zones.STATE == ref.STATE and zones.SLOT == ref.SLOT
    assert (zones.PERSON.itemsize * 25 * 4) % 8 == 0 and zones.TABLE.fields['vertices'][1] == 104 and zones.TABLE.fields['lines'][1] == 4200
    assert len(_lib.SIGNATURES["mpn_zone_events"][1]) == 10 and _lib.MPN_VERSION == 600
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    decl = re.search(r"\bint mpn_zone_events\s*\(([^)]*)\)\s*;", text)
    assert decl and len(decl.group(1).split(",")) == 10


def test_launcher_checks_before_any_hip_call():
    from multiposenet_amd import _lib
    P = ctypes.c_void_p
    good = dict(record=P(0x1000), track_rows=P(0x2000), B=4, max_boxes=8, streams=2, table=P(0x3000), prev=P(0x4000), next=P(0x5000),
                out=P(0x6000))

    def call(**change):
        a = dict(good, **change)
        return _lib.call("mpn_zone_events", a['record'], a['track_rows'], a['B'], a['max_boxes'], a['streams'], a['table'], a['prev'],
                         a['next'], a['out'], None)
    for name in ('record', 'track_rows', 'table', 'prev', 'next', 'out'):
        with pytest.raises(ValueError, match="BAD_ARG.*zone_events: null pointer"):
            call(**{name: None})
    with pytest.raises(ValueError, match="BAD_ARG.*zone_events:.*pure function"):
        call(next=P(0x4000))
    for bad in (dict(streams=0), dict(streams=3), dict(B=0)):
        with pytest.raises(ValueError, match="BAD_SHAPE.*zone_events:.*whole number of frames"):
            call(**bad)
    for bad in (dict(max_boxes=0), dict(max_boxes=65), dict(B=128, max_boxes=64)):
        with pytest.raises(ValueError, match="BAD_SHAPE.*zone_events: B = "):
            call(**bad)
    for bad in (dict(record=P(0x1008)), dict(track_rows=P(0x2004)), dict(table=P(0x3004)), dict(prev=P(0x4004)), dict(next=P(0x5004)),
                dict(out=P(0x6004))):
        with pytest.raises(ValueError, match="BAD_ALIGN.*zone_events:"):
            call(**bad)


# ---------------------------------------------------------------- the Detector
def _counter(streams=1, max_boxes=25, frame_size=(H, W), serial=11):
    from multiposenet_amd.zones import ZoneCounter
    c = object.__new__(ZoneCounter)
    c.streams, c.max_boxes, c.device, c.serial = streams, max_boxes, 'cpu', serial
    c.frame_size = (float(frame_size[0]), float(frame_size[1]))
    return c


def test_public_names_and_keywords():
    from multiposenet_amd import inference
    from multiposenet_amd.inference.detector import _Options
    from multiposenet_amd.zones import ZoneCounter
    assert inference.ZoneCounter is ZoneCounter
    parameters = inspect.signature(ZoneCounter).parameters
    assert list(parameters) == ['streams', 'frame_size', 'zones', 'lines', 'anchor', 'min_frames', 'min_keypoint_score', 'max_boxes',
                                'device']
    assert [parameters[k].default for k in parameters] == [1, None, None, None, 'feet', 1, 0.0, 25, None]
    for method in ('predict_batch', 'predict_images', 'predict_jpegs'):
        sig = inspect.signature(getattr(inference.Detector, method)).parameters
        assert list(sig)[-2:] == ['zones', 'track_eval'] and sig['zones'].default is None, method
    assert 'zones' not in inspect.signature(inference.Detector.__call__).parameters
    assert _Options._fields[-3:] == ('zones', 'anonymize', 'pose_nms')
    for name in ('check_batch', 'out_bytes', 'launch', 'commit', 'reset', 'unpack', 'totals', 'update'):
        assert callable(getattr(ZoneCounter, name))


@pytest.mark.parametrize("use_graph", [True, False])
def test_entry_keys_with_a_counter_and_without(use_graph):
    det = _detector(use_graph)
    trk, counter = _tracker(), _counter()
    batch = np.zeros((B, H, W, 3), np.uint8)
    frames = [np.zeros((H, W, 3), np.uint8)] * B
    base = (B, H, W, THR) if use_graph else ('eager', B, H, W)
    assert _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, zones=None) == base + ('track', 7, B)
    assert _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, zones=counter) == base + ('track', 7, B, 'zones', 11)
    key = _key_of(det.predict_images, frames, size=(H, W), score_threshold=THR, track=trk, zones=counter)
    assert key[:5] == ('images', B, H, W, THR) and key[6:] == ('track', 7, B, 'zones', 11)
    with pytest.raises(ValueError, match="zones= counts the tracker's identities: it needs track="):
        det.predict_batch(batch, zones=counter)
    with pytest.raises(ValueError, match="must be None or a zones.ZoneCounter"):
        det.predict_batch(batch, track=trk, zones=object())
    with pytest.raises(ValueError, match="counter was made for 2 streams, the tracker for 1"):
        det.predict_batch(batch, track=trk, zones=_counter(streams=2))
    with pytest.raises(ValueError, match="counter was made for max_boxes = 20, this Detector's is 25"):
        det.predict_batch(batch, track=trk, zones=_counter(max_boxes=20))
    with pytest.raises(ValueError, match=f"pixels of 480 x 640 frames.*a frame of {H} x {W}"):
        det.predict_batch(batch, track=trk, zones=_counter(frame_size=(480, 640)))
    odd = [np.zeros((H, W, 3), np.uint8), np.zeros((H, W + 2, 3), np.uint8)]
    with pytest.raises(ValueError, match=f"pixels of {H} x {W} frames.*a frame of {H} x {W + 2}"):
        det.predict_images(odd, size=(H, W), track=trk, zones=counter)
    # zones is checked before anonymize
    from multiposenet_amd.inference import Anonymize
    with pytest.raises(ValueError, match="zones="):
        det.predict_batch(batch, zones=counter, anonymize=Anonymize())


def test_record_layout_ends_with_the_zone_rows():
    from multiposenet_amd.inference.detector import RecordLayout

    class Rows:
        def out_bytes(self, b):
            return 1000 + b
    counter = _counter()
    base = lambda layout: (layout.record, layout.oks, layout.track, layout.nms)     # noqa: E731
    four = RecordLayout(4, 25)
    assert RecordLayout(4, 25, zones=None).astuple() == four.astuple()
    five = RecordLayout(4, 25, zones=counter)
    assert base(five) == base(four) and five.track_eval == four.track_eval
    assert five.zones.start % 16 == 0 and five.zones.start >= four.nms.stop
    assert five.zones.stop - five.zones.start == counter.out_bytes(4) == 4 * (25 * 104 + 576) and five.nbytes == five.zones.stop
    with_eval = RecordLayout(4, 25, track_eval=Rows())
    six = RecordLayout(4, 25, track_eval=Rows(), zones=counter)
    assert base(six) + (six.track_eval,) == base(with_eval) + (with_eval.track_eval,)
    assert six.zones.start % 16 == 0 and six.zones.start >= with_eval.track_eval.stop
    assert six.zones.stop - six.zones.start == counter.out_bytes(4)


def test_track_frames_has_the_switch(capsys):
    from multiposenet_amd import track_frames
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--help"])
    text = capsys.readouterr().out
    assert e.value.code == 0 and "--zones FILE.json" in text
