"""GPU: mpn_track_trails through `trails.TrackTrails.launch` on the handmade cases of tests/trails_cases.py, against the
plain-loop definition tests/trails_ref.py: rows and state byte for byte. No tolerance: the anchor is IEEE f64 operations with one
rounding to f32, the rest is integers."""
import numpy as np
import pytest

import trails_cases as cases
import trails_ref as ref

pytestmark = pytest.mark.gpu

SINGLE = [c['name'] for c in cases.CASES]
PAIRED = ['+'.join(p) for p in cases.PAIRS]


def _case(name):
    return cases.pair(*name.split('+')) if '+' in name else cases.BY_NAME[name]


def _streams(name):
    return 2 if '+' in name else 1


@pytest.fixture(scope="module")
def reference():
    """name -> (rows, state bytes) of the definition over the whole case, computed once."""
    out = {}
    for name in SINGLE + PAIRED:
        c = _case(name)
        state = ref.new_state(_streams(name), c['params']['length'])
        rows = ref.run(cases.reference_params(c['params']), cases.outputs_of(c['frames']), state, c['max_boxes'], c['total'])
        out[name] = rows, state.tobytes()
    return out


def _trails(c, streams):
    from multiposenet_amd.trails import TrackTrails
    return TrackTrails(streams=streams, max_boxes=c['max_boxes'], **c['params'])


def _device_inputs(trails, outputs, total, cuda):
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    from multiposenet_amd.zones import track_rows_of
    b = len(outputs)
    record, counts = fill_record(outputs, b, trails.max_boxes)
    if total is not None:
        record[:4].view(np.int32)[0] = total
    rows = track_rows_of(outputs, b, trails.max_boxes)
    return torch.from_numpy(record).to(cuda), torch.from_numpy(rows).to(cuda), counts


def _launch(trails, outputs, total, cuda, fill=0xAB):
    import torch
    b = len(outputs)
    record, rows, _ = _device_inputs(trails, outputs, total, cuda)
    out = torch.full((trails.out_bytes(b),), fill, dtype=torch.uint8, device=cuda)
    trails.launch(record, rows, out, b)
    return out.cpu().numpy()


def _same(out, rows, what):
    got = out.view(rows.dtype)
    for name in rows.dtype.names:
        field = (lambda a: a[name].view(np.uint32)) if name == 'points' else (lambda a: a[name])
        np.testing.assert_array_equal(field(got), field(rows), err_msg=f"{what}: rows, {name}")
    assert out.tobytes() == rows.tobytes(), what


def _same_state(got, want, K, what):
    g, w = np.frombuffer(got, ref.state_dtype(K)), np.frombuffer(want, ref.state_dtype(K))
    np.testing.assert_array_equal(g['frames'], w['frames'], err_msg=f"{what}: state, frames")
    for name in ref.slot_dtype(K).names:
        field = (lambda a: a['slots'][name].view(np.uint32)) if name == 'ring' else (lambda a: a['slots'][name])
        np.testing.assert_array_equal(field(g), field(w), err_msg=f"{what}: state slots, {name}")
    assert got == want, what


@pytest.mark.parametrize("name", SINGLE + PAIRED)
def test_rows_and_state_equal_the_reference(cuda, reference, name):
    c, streams = _case(name), _streams(name)
    rows, state = reference[name]
    trails = _trails(c, streams)
    out = _launch(trails, cases.outputs_of(c['frames']), c['total'], cuda)
    _same(out, rows, name)
    assert not trails.prev.cpu().numpy().any()                      # the launch alone advances nothing
    trails.commit()
    _same_state(trails.prev.cpu().numpy().tobytes(), state, c['params']['length'], name)


@pytest.mark.parametrize("name", [n for n in SINGLE + PAIRED if _case(n)['total'] is None])
def test_the_state_carries_over_every_cut(cuda, reference, name):
    """The frames of every stream split over two calls, at every cut, with a commit between: the rows and the final state of the
    one call."""
    c, streams = _case(name), _streams(name)
    rows, state = reference[name]
    outputs = cases.outputs_of(c['frames'])
    F, mb = len(outputs) // streams, c['max_boxes']
    counts = [len(f) for f in c['frames']]
    starts = np.concatenate([[0], np.cumsum(counts)])
    for cut in range(1, F):
        trails = _trails(c, streams)
        for part in (range(0, cut), range(cut, F)):
            which = [s * F + f for s in range(streams) for f in part]
            out = _launch(trails, [outputs[i] for i in which], None, cuda)
            trails.commit()
            want = np.zeros(len(which) * mb, rows.dtype)            # the rows of these images, dense, as a record of them has them
            at = 0
            for i in which:
                want[at:at + counts[i]] = rows[starts[i]:starts[i] + counts[i]]
                at += counts[i]
            _same(out, want, f"{name} cut {cut} frames {list(part)}")
        _same_state(trails.prev.cpu().numpy().tobytes(), state, c['params']['length'], f"{name} cut {cut}")


def test_the_launch_is_pure(cuda, reference):
    """Two launches before the commit write the same bytes, whatever the buffers held, and leave prev alone."""
    import torch
    from multiposenet_amd import _lib
    name = 'every_2'
    c = cases.BY_NAME[name]
    outputs = cases.outputs_of(c['frames'])
    trails = _trails(c, 1)
    _launch(trails, outputs[:4], None, cuda)
    trails.commit()
    before = trails.prev.cpu().numpy().tobytes()
    outs, states = [], []
    for fill in (0xAB, 0x00):
        trails.next.fill_(fill)
        outs.append(_launch(trails, outputs[4:], None, cuda, fill).tobytes())
        states.append(trails.next.cpu().numpy().tobytes())
        assert trails.prev.cpu().numpy().tobytes() == before
    assert outs[0] == outs[1] and states[0] == states[1] == reference[name][1]
    record, rows, _ = _device_inputs(trails, outputs[4:], None, cuda)
    out = torch.zeros(trails.out_bytes(6), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match="track_trails: prev and next are one buffer"):
        _lib.call("mpn_track_trails", _lib.ptr(record), _lib.ptr(rows), 6, trails.max_boxes, 1, 5, 2, 30, 0, 0.0, 480.0, 640.0, 1,
                  _lib.ptr(trails.prev), _lib.ptr(trails.prev), _lib.ptr(out), None)


def test_update_unpack_and_reset(cuda, reference):
    """`update` is the launch plus the commit for host dicts; `unpack` names the rows."""
    name = 'wrap_twice+every_1'
    c = _case(name)
    rows, state = reference[name]
    trails = _trails(c, 2)
    outputs = cases.outputs_of(c['frames'])
    got = trails.update(outputs)
    _same(trails.last_out, rows, name)
    _same_state(trails.prev.cpu().numpy().tobytes(), state, 5, name)
    want = ref.unpacked(rows, [len(f) for f in c['frames']])
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key, value in w.items():
            assert g[key].dtype == value.dtype and g[key].shape == value.shape, key
            np.testing.assert_array_equal(g[key], value, err_msg=key)
    assert got[0]['points'].shape == (1, 6, 2) and got[13]['points'].shape == (2, 6, 2) and got[23]['count'].shape == (0,)
    assert int(trails.state(0)['frames']) == 12 and int(trails.state(1)['frames']) == 12
    trails.reset(stream=1)
    assert int(trails.state(1)['frames']) == 0 and not trails.state(1)['slots']['id'].any() and int(trails.state(0)['frames']) == 12
    with pytest.raises(ValueError, match="track_ids"):
        trails.update([{k: v for k, v in o.items() if k != 'track_ids'} for o in outputs])


def test_records_without_keypoints_take_the_box(cuda):
    """Dicts without 'keypoints' (a Detector without the PRN): the zeros of the record do not pass for ankles."""
    c = cases.BY_NAME['box_bottom']
    feet = _trails(dict(c, params=cases.params()), 1)
    got = feet.update(cases.outputs_of(c['frames'], keypoints=False))
    state = ref.new_state(1, 5)
    rows = ref.run(cases.reference_params(c['params']), cases.outputs_of(c['frames'], keypoints=False), state, c['max_boxes'])
    _same(feet.last_out, rows, "no keypoints")
    assert not got[0]['anchor_from_keypoints'].any() and got[0]['tracked'].all() and got[1]['count'].tolist() == [2, 2]
