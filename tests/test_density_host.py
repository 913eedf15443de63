"""CPU: the definition tests/density_ref.py against grids worked out by hand and, for the picture, against Pillow; the argument
checks of `density.DensityMap`; the size formulas and launcher checks of mpn_density_map and mpn_draw_density; and what `density=`
adds to the Detector's signatures, keys and result layout."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import density_cases as cases
import density_ref as ref
from test_detector_options_host import B, H, W, THR, _detector, _key_of, _tracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, A, N, O, V = ref.FLAG_TRACKED, ref.FLAG_ANKLES, ref.FLAG_NO_ANCHOR, ref.FLAG_OUTSIDE, ref.FLAG_VISIT
FULL = ref.SATURATED


def _run(name):
    c = cases.BY_NAME[name]
    state = cases.preloaded(c)
    outputs = cases.outputs_of(c['frames'])
    rows, images, snaps = ref.run(cases.reference_params(c['params']), outputs, state, c['max_boxes'], c['total'], c['tracked'])
    return c, rows, images, snaps, state[0]


def _nonzero(plane):
    return {(int(r), int(c)): int(plane[r, c]) for r, c in zip(*np.nonzero(plane))}


# ---------------------------------------------------------------- the map, by hand
def test_halving_by_hand():
    """half_life = 2, one person in cell (2, 2) for four frames. dwell: 1; frame 2 halves to 0 and adds: 1; 2; frame 4 halves to
    1 and adds: 2. visits: the arrival in frame 1, halved away in frame 2, and never another."""
    _, rows, images, snaps, st = _run('halving')
    assert images['max_dwell'].tolist() == [1, 1, 2, 2] and images['max_visits'].tolist() == [1, 0, 0, 0]
    assert _nonzero(st['dwell']) == {(2, 2): 2} and not st['visits'].any() and int(st['frames']) == 4
    assert rows['flags'][:4].tolist() == [T | A | V, T | A, T | A, T | A] and rows['cells'][:4].tolist() == [1] * 4
    assert rows['row'][:4].tolist() == [2] * 4 and rows['col'][:4].tolist() == [2] * 4
    assert [int(s[2, 2]) for s in snaps] == [1, 1, 2, 2] and images['counted'].tolist() == [1] * 4 and images['visits'].tolist() == [1, 0, 0, 0]
    # half_life = 3 and the visits shown: (2, 2) visited in frame 1, (2, 3) in frame 3 after the halving, (2, 2) again in frame 4
    _, rows, images, snaps, st = _run('halving_visits_shown')
    assert [_nonzero(s) for s in snaps] == [{(2, 2): 1}, {(2, 2): 1}, {(2, 3): 1}, {(2, 3): 1, (2, 2): 1}]
    assert _nonzero(st['dwell']) == {(2, 2): 2, (2, 3): 1} and images['max_dwell'].tolist() == [1, 2, 1, 2]


def test_saturation_by_hand():
    _, rows, images, snaps, st = _run('saturate')
    assert _nonzero(st['dwell']) == {(0, 0): 7, (2, 2): FULL} and _nonzero(st['visits']) == {(2, 2): FULL}
    assert images['max_dwell'].tolist() == [FULL] * 3 and images['max_visits'].tolist() == [FULL, FULL, FULL]
    assert rows['flags'][:3].tolist() == [T | A | V, T | A, T | A]
    _, _, images, _, st = _run('saturate_then_halve')               # frame 3: 2^32 - 1 >> 1 = 2^31 - 1, + 1
    assert int(st['dwell'][2, 2]) == 2 ** 31 and int(st['visits'][2, 2]) == 2 ** 31 - 1
    assert images['max_dwell'].tolist() == [FULL, FULL, 2 ** 31] and images['max_visits'].tolist() == [FULL, FULL, 2 ** 31 - 1]


def test_visits_by_hand():
    _, rows, images, _, st = _run('wander')
    assert rows['flags'][:4].tolist() == [T | A | V, T | A, T | A | V, T | A | V]
    assert _nonzero(st['visits']) == {(2, 2): 2, (2, 3): 1} and _nonzero(st['dwell']) == {(2, 2): 3, (2, 3): 1}
    assert images['max_visits'].tolist() == [1, 1, 1, 2] and int(st['slots'][0]['cell1']) == 2 * 10 + 2 + 1
    _, rows, images, _, st = _run('leave_and_reenter')              # outside in frame 2: the old cell is a visit again in frame 3
    assert rows['flags'][:4].tolist() == [T | A | V, T | A | O, T | A | V, T | A]
    assert rows['row'][:4].tolist() == [2, -1, 2, 2] and rows['cells'][:4].tolist() == [1, 0, 1, 1]
    assert _nonzero(st['visits']) == {(2, 2): 2} and _nonzero(st['dwell']) == {(2, 2): 3} and images['counted'].tolist() == [1, 0, 1, 1]
    _, rows, _, _, st = _run('duplicate_id')                        # the second row of an id dwells and does not visit
    assert rows['flags'][:5].tolist() == [T | A | V, A, T | A | V, A, T | A | V]
    assert _nonzero(st['dwell']) == {(2, 2): 3, (3, 6): 2} and _nonzero(st['visits']) == {(2, 2): 2, (3, 6): 1}
    _, rows, _, _, st = _run('untracked_launch')                    # without track rows: dwell alone
    assert rows['flags'][:4].tolist() == [A] * 4 and not st['visits'].any() and not st['slots']['id'].any()
    assert _nonzero(st['dwell']) == {(2, 2): 3, (2, 3): 1}


def test_eviction_by_hand():
    _, rows, images, _, st = _run('evict')
    ids = st['slots']['id'].tolist()
    assert ids[:3] == [65, 1, 2] and ids[3:] == list(range(4, 65))  # 65 took slot 0; 1 came back into slot 1; 2 into slot 2
    assert (rows['flags'][:67] == T | A | V).all() and images['visits'].tolist() == [64, 1, 2]
    # cell (0, 0): ids 1 and 61 in frame 1, id 1 anew in frame 3; (0, 1): 2, 62, 2 anew; (2, 2): id 23, then 65
    assert int(st['visits'][0, 0]) == 3 and int(st['visits'][0, 1]) == 3 and int(st['visits'][2, 2]) == 2


def test_anchors_and_rows_without_one_by_hand():
    _, rows, images, _, st = _run('no_anchor')
    assert rows['flags'][:7].tolist() == [T | A | V, T | A | V, N, T | A, A, A, T | A]
    assert rows[2].tolist() == (-1, -1, N, 0) and images['counted'].tolist() == [2, 1, 3]
    assert _nonzero(st['dwell']) == {(2, 2): 3, (5, 7): 3} and int(st['slots'][0]['last']) == 3
    _, rows, _, _, _ = _run('ankles')       # the right ankle alone (30, 30); the box's bottom (61, 32); the mean of both (30, 32)
    assert [tuple(r)[:3] for r in rows[:3].tolist()] == [(3, 3, T | A | V), (4, 7, T | V), (4, 3, T | A | V)]
    _, rows, _, _, _ = _run('box_centre')   # (31, 15) and (31, 35)
    assert [tuple(r)[:3] for r in rows[:2].tolist()] == [(1, 3, T | V), (4, 3, T | V)]
    _, rows, _, _, st = _run('box_bottom')  # (31, 22); (31, 48) is below the frame
    assert [tuple(r) for r in rows[:2].tolist()] == [(2, 3, T | V, 1), (-1, -1, T | O, 0)] and _nonzero(st['dwell']) == {(2, 3): 3}
    _, rows, images, _, st = _run('empty_frame')
    assert int(st['frames']) == 4 and images['counted'].tolist() == [1, 0, 1, 0] and images['max_dwell'].tolist() == [1, 1, 1, 1]
    _, rows, images, _, _ = _run('total_clamped')                   # total 4 of 3 + 3 rows: the second frame has one
    assert images['counted'].tolist() == [3, 1, 0] and not rows[4:].view(np.uint8).any()


def test_box_footprint_by_hand():
    c, rows, images, _, st = _run('box_footprint')
    assert rows['cells'][:6].tolist() == [2, 0, 60, 1 * 2, 0, 2 * 3]
    assert images['counted'].tolist() == [2, 1, 1]
    want = np.ones((6, 10), np.int64)
    want[4:6, 9] += 1                                               # x 75..83, y 34..48
    want[1:3, 2] += 1                                               # the default box of (20, 20): x 17..25, y 8..22
    want[0:3, 2:4] += 1                                             # x 16..30, y 2..21
    np.testing.assert_array_equal(st['dwell'], want)
    assert rows['flags'][:3].tolist() == [T | A | V, T | A | V, T | A | V] and int(rows[4]['flags']) == T | A | V
    _, rows, _, _, st = _run('ragged')                              # cell = 7: (79, 47) is cell (6, 11), the ragged corner
    assert [tuple(r)[:2] for r in rows[:5].tolist()] == [(6, 11), (5, 10), (6, 11), (0, 0), (1, 0)] and st['dwell'].shape == (7, 12)
    assert int(rows[2]['flags']) == T | A                           # (77, 42) is the same cell: no visit
    _, rows, _, _, st = _run('ragged_box')                          # x 60..90, y 30..60: centres 66.5 .. 80.5 (3), 31.5 .. 45.5 (3)
    assert rows['cells'][:4].tolist() == [2, 9, 2, 1] and int(st['dwell'][6, 11]) == 2


def test_the_case_table_holds_every_kind_of_frame():
    """What the issue asks of the handmade cases, read off the reference's own results."""
    seen = set()
    for c in cases.CASES:
        p = cases.reference_params(c['params'])
        state = cases.preloaded(c)
        before = state.copy()
        rows, images, _ = ref.run(p, cases.outputs_of(c['frames']), state, c['max_boxes'], c['total'], c['tracked'])
        F = len(c['frames'])
        assert F in (3, 4) and c['params']['frame_size'] == (48, 80) and (p.gh, p.gw) in ((6, 10), (7, 12))
        if p.half_life and any(now % p.half_life == 0 for now in range(1, F + 1)):
            seen.add('halving')
        full = before[0]['dwell'] == FULL
        if full.any() and (state[0]['dwell'][full] == FULL).all() and not p.half_life:
            seen.add('saturates')
        flags, at = rows['flags'], 0
        by_id = {}
        for f, persons in enumerate(c['frames']):
            ids = [q['track_id'] for q in persons]
            if len(ids) != len(set(ids)):
                seen.add('two rows with one id')
            if not persons:
                seen.add('empty frame')
            for r, q in enumerate(persons):
                if c['total'] is None and c['tracked'] and flags[at + r] & T:
                    by_id.setdefault(q['track_id'], []).append((f, int(flags[at + r]), int(rows[at + r]['row']), int(rows[at + r]['col'])))
                if flags[at + r] & N:
                    seen.add('no anchor')
                if p.footprint == ref.BOX and not flags[at + r] & N:
                    y0, x0, y1, x1 = (float(v) for v in q['box'] * np.array([48, 80, 48, 80], np.float32))
                    if (x1 > 80 or y1 > 48 or x0 < 0 or y0 < 0) and rows[at + r]['cells'] > 0:
                        seen.add('box past the frame')
                    if rows[at + r]['cells'] == 0 and np.isfinite([x0, x1, y0, y1]).all():
                        seen.add('box over no centre')
            at += len(persons)
        for history in by_id.values():
            if any(fl & V for _, fl, _, _ in history) and any(not fl & V and not fl & O for _, fl, _, _ in history):
                seen.add('visit and non-visit')
            for (f0, fl0, r0, c0), (f1, fl1, _, _), (f2, fl2, r2, c2) in zip(history, history[1:], history[2:]):
                if fl1 & O and fl2 & V and (r0, c0) == (r2, c2):
                    seen.add('outside, then the old cell: a visit')
        if len({q['track_id'] for persons in c['frames'] for q in persons if q['track_id'] > 0}) >= 65:
            seen.add('a 65th id')
    assert seen == {'halving', 'saturates', 'visit and non-visit', 'outside, then the old cell: a visit', 'two rows with one id',
                    'a 65th id', 'no anchor', 'box past the frame', 'box over no centre', 'empty frame'}


def test_two_calls_are_one():
    """The reference itself carries its state: the frames in two calls give the rows and the state of one call."""
    c, rows, images, snaps, st = _run('wander')
    outputs, p = cases.outputs_of(c['frames']), cases.reference_params(c['params'])
    again = cases.preloaded(c)
    first, second = ref.run(p, outputs[:1], again, c['max_boxes']), ref.run(p, outputs[1:], again, c['max_boxes'])
    assert np.concatenate([first[0][:1], second[0][:3]]).tobytes() == rows[:4].tobytes()
    assert np.concatenate([first[1], second[1]]).tobytes() == images.tobytes() and again[0].tobytes() == st.tobytes()
    assert np.concatenate([first[2], second[2]]).tobytes() == snaps.tobytes()


# ---------------------------------------------------------------- the picture against Pillow
def _pillow(rgba, levels, setting):
    from PIL import Image
    frame = Image.fromarray(rgba[..., :3].copy(), 'RGB')
    colours = Image.fromarray(np.asarray(cases.colormap_of(setting), np.uint8)[levels], 'RGB')
    alpha = Image.fromarray(np.array(ref.alpha_table(setting['opacity']), np.uint8)[levels], 'L')
    frame.paste(colours, (0, 0), mask=alpha)
    out = np.full(rgba.shape, 255, np.uint8)
    out[..., :3] = np.asarray(frame)
    return out


@pytest.mark.parametrize("setting", cases.SETTINGS + cases.ONE_CELL, ids=lambda s: f"{s['size'][0]}x{s['size'][1]}-{s['cell']}-{s['smooth']}")
def test_the_restatement_draws_what_pillow_draws(setting):
    """Every grid that counts anything blends at least one pixel and leaves at least one alone; the empty grid leaves its frame
    alone. With ONE cell over the frame every pixel has one level: there a grid that counts blends every pixel, and the test says
    so."""
    h, w = setting['size']
    one_cell = setting in cases.ONE_CELL
    for k, (name, grid, most) in enumerate(cases.draw_grids(setting)):
        before = cases.background(h, w, k)
        args = (grid, most, setting['cell'], setting['smooth'], setting['full_scale'], setting['opacity'], cases.colormap_of(setting))
        got = ref.draw(before.copy(), *args)
        levels = ref.level_image(grid, setting['full_scale'] or most, h, w, setting['cell'], setting['smooth'])
        want = _pillow(before, levels, setting) if levels is not None else before
        np.testing.assert_array_equal(got, want, err_msg=f"{setting} {name}")
        np.testing.assert_array_equal(ref.draw_arrays(before, *args), got, err_msg=f"{setting} {name}: the array form")
        alpha = np.array(ref.alpha_table(setting['opacity']))[levels] if levels is not None else np.zeros((h, w), int)
        blended, untouched = int((alpha > 0).sum()), int((alpha == 0).sum())
        assert (got[alpha == 0] == before[alpha == 0]).all()
        if not most:
            assert blended == 0 and got.tobytes() == before.tobytes(), (setting, name)
        elif one_cell:
            assert blended == h * w and untouched == 0 and grid.shape == (1, 1), (setting, name)
        else:
            assert blended >= 1 and untouched >= 1, (setting, name)


def test_levels_and_the_smooth_weights_by_hand():
    assert ref.cell_levels([[0, 1, 20, 40, 41, 5000]], 40) == [[0, 6, 128, 255, 255, 255]] and ref.cell_levels([[3]], 0) is None
    assert ref.cell_levels([[FULL]], 2 ** 31 - 1) == [[255]] and ref.cell_levels([[1]], 2 ** 31 - 1) == [[0]]
    assert ref.alpha_table(160)[:3] == [0, 1, 1] and ref.alpha_table(160)[255] == 160 and ref.alpha_table(255)[128] == 128
    assert ref.alpha_table(0) == [0] * 256
    levels = [[0, 200]]                                             # s = 4: centres at x = 1.5 and 5.5 (u = 0 and 8)
    assert [ref.pixel_level(levels, 0, x, 4, True) for x in range(8)] == [0, 0, 25, 75, 125, 175, 200, 200]
    assert [ref.pixel_level(levels, 0, x, 4, False) for x in range(8)] == [0] * 4 + [200] * 4
    assert ref.blend8(64, 200, 0) == 150 and ref.blend8(255, 7, 99) == 99 and ref.blend8(1, 0, 255) == 1


# ---------------------------------------------------------------- the front end
def test_every_refusal_of_the_class():
    from multiposenet_amd.density import DensityMap
    ok = dict(frame_size=(480, 640))
    for bad, message in ((dict(streams=0), "streams must be an integer >= 1"),
                         (dict(streams=True), "streams must be an integer >= 1"),
                         (dict(max_boxes=65), "max_boxes must be an integer in 1..64 \\(got 65\\)"),
                         (dict(max_boxes=0), "max_boxes must be an integer in 1..64"),
                         (dict(frame_size=None), "frame_size must be \\(height, width\\)"),
                         (dict(frame_size=(0, 640)), "frame_size must be two integers"),
                         (dict(frame_size=(480.0, 640)), "frame_size must be two integers"),
                         (dict(frame_size=(480, 8193)), "frame_size must be two integers \\(height, width\\) in 1..8192"),
                         (dict(cell=3), "cell must be an integer in 4..256 \\(got 3\\)"),
                         (dict(cell=257), "cell must be an integer in 4..256"),
                         (dict(cell=8.0), "cell must be an integer"),
                         (dict(cell=4), "a grid of 120 x 160 cells has more than 16384"),
                         (dict(footprint='feet'), "footprint must be one of \\['anchor', 'box'\\] \\(got 'feet'\\)"),
                         (dict(anchor='head'), "anchor must be one of \\['feet', 'box_bottom', 'box_centre'\\] \\(got 'head'\\)"),
                         (dict(min_keypoint_score=float('nan')), "min_keypoint_score must be finite"),
                         (dict(min_keypoint_score='x'), "min_keypoint_score must be a number"),
                         (dict(half_life=-1), "half_life must be an integer in 0..65535"),
                         (dict(half_life=65536), "half_life must be an integer in 0..65535"),
                         (dict(show='both'), "show must be one of \\['dwell', 'visits'\\]"),
                         (dict(draw=1), "draw must be False or True"),
                         (dict(smooth='yes'), "smooth must be False or True"),
                         (dict(full_scale=-1), "full_scale must be an integer in 0..2147483647"),
                         (dict(full_scale=2 ** 31), "full_scale must be an integer in 0..2147483647"),
                         (dict(opacity=-1), "opacity must be an integer in 0..255"),
                         (dict(opacity=256), "opacity must be an integer in 0..255"),
                         (dict(colormap=np.zeros((256, 4), np.uint8)), "colormap must be None or uint8 \\[256, 3\\]"),
                         (dict(colormap=np.zeros((256, 3), np.int32)), "colormap must be None or uint8 \\[256, 3\\]")):
        with pytest.raises(ValueError, match="DensityMap: " + message):
            DensityMap(**dict(ok, **bad))


def test_abi_sizes_and_the_table():
    from multiposenet_amd import _lib, density
    lib = _lib.lib()
    for gh, gw in ((1, 1), (6, 10), (7, 12), (128, 128), (1, 16384)):
        G = gh * gw
        assert lib.mpn_density_state_bytes(1, gh, gw) == density.state_dtype(gh, gw).itemsize == 32 + 64 * 16 + 8 * G
        assert lib.mpn_density_state_bytes(3, gh, gw) == 3 * (32 + 64 * 16 + 8 * G)
        assert density.state_dtype(gh, gw) == ref.state_dtype(gh, gw)
        assert lib.mpn_density_snapshot_bytes(4, gh, gw) == 4 * G * 4
        assert lib.mpn_draw_density_workspace_bytes(3, gh, gw) == (3 * G + 15) // 16 * 16
    assert (density.ROW, density.IMAGE, density.SLOT) == (ref.ROW, ref.IMAGE, ref.SLOT)
    assert lib.mpn_density_out_bytes(4, 25) == 4 * 25 * 16 + 4 * 16 and lib.mpn_density_out_bytes(64, 64) == 4096 * 16 + 64 * 16
    for bad in ((0, 6, 10), (1, 0, 10), (1, 6, 0), (1, 129, 128), (1, 1, 16385), (4097, 6, 10)):
        assert lib.mpn_density_state_bytes(*bad) == 0 and lib.mpn_density_snapshot_bytes(*bad) == 0
    for bad in ((0, 6, 10), (1, 0, 10), (1, 129, 128), (65536, 6, 10)):
        assert lib.mpn_draw_density_workspace_bytes(*bad) == 0
    for bad in ((0, 8), (4, 0), (4, 65), (128, 64)):
        assert lib.mpn_density_out_bytes(*bad) == 0
    assert lib.mpn_draw_density_tables_bytes() == 32 + 1024
    colours = cases.RAINBOW
    table = density.draw_table(colours, 160, True, 40, 'visits').view(np.uint32)
    assert table[:8].tolist() == [3, 40, 0, 0, 0, 0, 0, 0] and table.nbytes == 1056
    for level in (0, 1, 128, 255):
        r, g, b = (int(v) for v in colours[level])
        assert int(table[8 + level]) == r | g << 8 | b << 16 | ref.alpha_table(160)[level] << 24
    assert density.draw_table(colours, 255, False, 0, 'dwell').view(np.uint32)[:2].tolist() == [0, 0]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    for name, count in (("mpn_density_map", 19), ("mpn_draw_density", 15)):
        decl = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl and len(decl.group(1).split(",")) == count == len(_lib.SIGNATURES[name][1])
    assert "#define MPN_DRAW_DENSITY_TABLE_BYTES 1056" in text
    for source in ("zone_events.hip", "trails.hip", "density.hip"):     # one rule for the anchor, in one header
        body = open(os.path.join(ROOT, "multiposenet_amd", "csrc", source)).read()
        assert '#include "person_anchor.h"' in body and "mpn_anchor::person_anchor(" in body and "kLeftAnkle" not in body


def test_the_map_launcher_checks_before_any_hip_call():
    from multiposenet_amd import _lib
    V_ = ctypes.c_void_p
    good = dict(record=V_(0x1000), track_rows=V_(0x2000), B=4, max_boxes=8, streams=2, height=48, width=80, cell=8, footprint=0,
                anchor=0, score=0.0, with_keypoints=1, half_life=0, show=0, prev=V_(0x4000), next=V_(0x5000), out=V_(0x6000),
                snapshots=V_(0x7000))

    def call(**change):
        a = dict(good, **change)
        return _lib.call("mpn_density_map", a['record'], a['track_rows'], a['B'], a['max_boxes'], a['streams'], a['height'], a['width'],
                         a['cell'], a['footprint'], a['anchor'], a['score'], a['with_keypoints'], a['half_life'], a['show'], a['prev'],
                         a['next'], a['out'], a['snapshots'], None)
    for name in ('record', 'prev', 'next', 'out'):
        with pytest.raises(ValueError, match="BAD_ARG.*density_map: null pointer"):
            call(**{name: None})
    with pytest.raises(ValueError, match="BAD_ARG.*density_map:.*pure function"):
        call(next=V_(0x4000))
    for bad, message in ((dict(cell=3), "cell"), (dict(cell=257), "cell"), (dict(height=0), "height"), (dict(height=8193), "height"),
                         (dict(width=0), "width"), (dict(width=8193), "width"), (dict(height=1024, width=1032), "cells"),
                         (dict(footprint=2), "footprint"), (dict(half_life=-1), "half_life"), (dict(half_life=65536), "half_life"),
                         (dict(show=2), "show"), (dict(show=1, track_rows=None), "show"),
                         (dict(score=float('nan')), "finite"), (dict(score=float('inf')), "finite")):
        with pytest.raises(ValueError, match="BAD_ARG.*density_map: .*" + message):
            call(**bad)
    for bad in (dict(streams=0), dict(streams=3), dict(B=0)):
        with pytest.raises(ValueError, match="BAD_SHAPE.*density_map:.*whole number of frames"):
            call(**bad)
    for bad in (dict(max_boxes=0), dict(max_boxes=65), dict(B=128, max_boxes=64)):
        with pytest.raises(ValueError, match="BAD_SHAPE.*density_map: B = "):
            call(**bad)
    for bad in (dict(record=V_(0x1008)), dict(out=V_(0x6008)), dict(track_rows=V_(0x2004)), dict(prev=V_(0x4004)), dict(next=V_(0x5004)),
                dict(snapshots=V_(0x7004))):
        with pytest.raises(ValueError, match="BAD_ALIGN.*density_map:"):
            call(**bad)


def test_the_drawing_launcher_checks_before_any_hip_call():
    from multiposenet_amd import _lib
    V_ = ctypes.c_void_p
    work_bytes = _lib.lib().mpn_draw_density_workspace_bytes(4, 6, 10)
    good = dict(descs=V_(0x1000), snapshots=V_(0x2000), rows=V_(0x3000), tables=V_(0x5000), tables_bytes=1056, B=4, max_boxes=8,
                height=48, width=80, cell=8, out=V_(0x6000), out_bytes=1 << 20, work=V_(0x7000), work_bytes=work_bytes)

    def call(**change):
        a = dict(good, **change)
        return _lib.call("mpn_draw_density", a['descs'], a['snapshots'], a['rows'], a['tables'], a['tables_bytes'], a['B'], a['max_boxes'],
                         a['height'], a['width'], a['cell'], a['out'], a['out_bytes'], a['work'], a['work_bytes'], None)
    for name in ('descs', 'snapshots', 'rows', 'tables', 'out', 'work'):
        with pytest.raises(ValueError, match="BAD_ARG.*draw_density: null pointer"):
            call(**{name: None})
    for bad in (dict(B=0), dict(B=65536), dict(max_boxes=0), dict(max_boxes=65), dict(B=128, max_boxes=64), dict(cell=3), dict(cell=257),
                dict(height=0), dict(width=8193), dict(height=1024, width=1032)):
        with pytest.raises(ValueError, match="BAD_SHAPE.*draw_density:"):
            call(**bad)
    for bad in (dict(descs=V_(0x1008)), dict(rows=V_(0x3008)), dict(out=V_(0x6008)), dict(work=V_(0x7008)), dict(snapshots=V_(0x2002)),
                dict(tables=V_(0x5002))):
        with pytest.raises(ValueError, match="BAD_ALIGN.*draw_density:"):
            call(**bad)
    for bad in (dict(work_bytes=work_bytes - 1), dict(out_bytes=15), dict(tables_bytes=1055)):
        with pytest.raises(_lib.MpnError, match="WORKSPACE.*draw_density:"):
            call(**bad)


# ---------------------------------------------------------------- the Detector
def _density(streams=1, max_boxes=25, frame_size=(H, W), serial=17, show='dwell'):
    from multiposenet_amd import density
    d = object.__new__(density.DensityMap)
    d.streams, d.max_boxes, d.device, d.serial, d.show = streams, max_boxes, 'cpu', serial, show
    d.frame_size = (int(frame_size[0]), int(frame_size[1]))
    return d


def _trails(serial=13):
    from multiposenet_amd import trails
    t = object.__new__(trails.TrackTrails)
    t.streams, t.max_boxes, t.device, t.serial, t.length = 1, 25, 'cpu', serial, 5
    t.frame_size, t.row = (float(H), float(W)), trails.row_dtype(5)
    return t


def test_public_names_and_keywords():
    from multiposenet_amd import inference
    from multiposenet_amd.inference.detector import _Options
    from multiposenet_amd.density import DensityMap, draw_density
    assert inference.DensityMap is DensityMap and inference.draw_density is draw_density
    parameters = inspect.signature(DensityMap).parameters
    assert list(parameters) == ['streams', 'frame_size', 'cell', 'footprint', 'anchor', 'min_keypoint_score', 'half_life', 'show', 'draw',
                                'smooth', 'full_scale', 'opacity', 'colormap', 'max_boxes', 'device']
    assert [parameters[k].default for k in parameters] == [1, None, 16, 'anchor', 'feet', 0.0, 0, 'dwell', True, True, 0, 160, None, 25,
                                                           None]
    for method in ('predict_batch', 'predict_images', 'predict_jpegs'):
        sig = inspect.signature(getattr(inference.Detector, method)).parameters
        assert list(sig)[-4:] == ['density', 'trails', 'zones', 'track_eval'] and sig['density'].default is None, method
    assert 'density' not in inspect.signature(inference.Detector.__call__).parameters
    assert _Options._fields[-5:] == ('density', 'trails', 'zones', 'anonymize', 'pose_nms')
    for name in ('check_batch', 'check_frame_sizes', 'out_bytes', 'launch', 'launch_draw', 'commit', 'reset', 'state', 'grid', 'unpack',
                 'update'):
        assert callable(getattr(DensityMap, name))
    assert list(inspect.signature(draw_density).parameters) == ['image', 'density', 'stream']
    with pytest.raises(ValueError, match="draw_density: density must be a density.DensityMap"):
        draw_density(np.zeros((4, 4, 3), np.uint8), None)


@pytest.mark.parametrize("use_graph", [True, False])
def test_entry_keys_with_density_and_without(use_graph):
    from multiposenet_amd.inference import Anonymize
    det = _detector(use_graph)
    trk, density, trails = _tracker(), _density(), _trails()
    batch = np.zeros((B, H, W, 3), np.uint8)
    frames = [np.zeros((H, W, 3), np.uint8)] * B
    base = (B, H, W, THR) if use_graph else ('eager', B, H, W)
    assert _key_of(det.predict_batch, batch, score_threshold=THR, density=None) == base
    assert _key_of(det.predict_batch, batch, score_threshold=THR, density=density) == base + ('density', 17)
    assert _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, density=None) == base + ('track', 7, B)
    assert _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, density=density) == base + ('track', 7, B, 'density', 17)
    spec = Anonymize()
    key = _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, trails=trails, density=density, annotate=True, anonymize=spec)
    assert key == base + ('annotate', 'track', 7, B, 'trails', 13, 'density', 17, 'anonymize', spec)
    key = _key_of(det.predict_images, frames, size=(H, W), score_threshold=THR, density=density)
    assert key[:5] == ('images', B, H, W, THR) and key[6:] == ('density', 17)
    with pytest.raises(ValueError, match="must be None or a density.DensityMap"):
        det.predict_batch(batch, density=object())
    with pytest.raises(ValueError, match="show='visits' counts the arrivals of identities: it needs track="):
        det.predict_batch(batch, density=_density(show='visits'))
    assert _key_of(det.predict_batch, batch, score_threshold=THR, track=trk, density=_density(show='visits'))[-2:] == ('density', 17)
    with pytest.raises(ValueError, match="map was made for 2 streams, the tracker for 1"):
        det.predict_batch(batch, track=trk, density=_density(streams=2))
    with pytest.raises(ValueError, match="map was made for max_boxes = 20, this Detector's is 25"):
        det.predict_batch(batch, density=_density(max_boxes=20))
    with pytest.raises(ValueError, match=f"grid covers 480 x 640 frames.*a frame of {H} x {W}"):
        det.predict_batch(batch, density=_density(frame_size=(480, 640)))
    odd = [np.zeros((H, W, 3), np.uint8), np.zeros((H, W + 2, 3), np.uint8)]
    with pytest.raises(ValueError, match=f"grid covers {H} x {W} frames.*a frame of {H} x {W + 2}"):
        det.predict_images(odd, size=(H, W), density=density)
    with pytest.raises(ValueError, match="2 images are not a whole number of frames for each of 4 streams"):
        det.predict_batch(batch, density=_density(streams=4))
    # density is checked before trails, zones and anonymize
    with pytest.raises(ValueError, match="density"):
        det.predict_batch(batch, density=object(), trails=trails)
    with pytest.raises(ValueError, match="density"):
        det.predict_batch(batch, density=object(), anonymize=spec)


def test_record_layout_ends_with_the_density_rows():
    from multiposenet_amd.inference.detector import RecordLayout
    density, trails = _density(), _trails()
    four = RecordLayout(4, 25)
    assert RecordLayout(4, 25, density=None).astuple() == four.astuple()
    five = RecordLayout(4, 25, density=density)
    assert five.astuple()[:-1] == four.astuple()[:-1] and five.density.start % 16 == 0 and five.density.start >= four.nms.stop
    assert five.density.stop - five.density.start == density.out_bytes(4) == 4 * 25 * 16 + 4 * 16 and five.nbytes == five.density.stop
    with_trails = RecordLayout(4, 25, trails=trails)
    six = RecordLayout(4, 25, trails=trails, density=density)
    assert six.astuple()[:-1] == with_trails.astuple()[:-1] and RecordLayout.PARTS[-1] == 'density'
    assert six.density.start % 16 == 0 and six.density.start >= with_trails.trails.stop
    assert six.density.stop - six.density.start == density.out_bytes(4)


def test_track_frames_has_the_switches(capsys):
    from multiposenet_amd import track_frames
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--help"])
    text = capsys.readouterr().out
    assert e.value.code == 0
    for switch in ("--density [CELL]", "--density-footprint {anchor,box}", "--density-half-life N", "--density-show {dwell,visits}",
                   "--density-full-scale N", "--density-opacity A", "--no-density-smooth", "--no-density-draw",
                   "--density-out FILE.npz"):
        assert switch in text, switch
    for switches in (["--density-half-life", "2"], ["--no-density-draw"], ["--density-out", "x.npz"], ["--density-footprint", "box"]):
        with pytest.raises(SystemExit) as e:
            track_frames.main(["--images", "."] + switches)
        assert e.value.code == 2 and "need --density" in capsys.readouterr().err
