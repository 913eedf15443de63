"""GPU: mpn_zone_events through `zones.ZoneCounter.launch` on the handmade cases of tests/zones_cases.py, against the plain-loop
definition tests/zones_ref.py: person rows, image rows and state byte for byte. No tolerance: the arithmetic has no
transcendental and every operation is one IEEE f64 operation."""
import numpy as np
import pytest

import zones_cases as cases
import zones_ref as ref

pytestmark = pytest.mark.gpu

SINGLE = [c['name'] for c in cases.CASES]
PAIRED = ['+'.join(p) for p in cases.PAIRS]


def _case(name):
    return cases.pair(*name.split('+')) if '+' in name else cases.BY_NAME[name]


def _streams(name):
    return 2 if '+' in name else 1


@pytest.fixture(scope="module")
def reference():
    """name -> (person rows, image rows, state bytes) of the definition over the whole case, computed once."""
    out = {}
    for name in SINGLE + PAIRED:
        c = _case(name)
        state = ref.new_state(_streams(name))
        persons, images = ref.run(cases.geometry(c['geo']), cases.outputs_of(c['frames']), state, c['max_boxes'], c['total'])
        out[name] = persons, images, ref.pack_state(state)
    return out


def _counter(c, streams):
    from multiposenet_amd.zones import ZoneCounter
    return ZoneCounter(streams=streams, max_boxes=c['max_boxes'], **c['geo'])


def _device_inputs(counter, outputs, total, cuda):
    """(record, track rows) of the frames on the device, the record's total overwritten where the case says so."""
    import torch
    from multiposenet_amd.tracking import fill_record
    from multiposenet_amd.zones import track_rows_of
    b = len(outputs)
    record, counts = fill_record(outputs, b, counter.max_boxes)
    if total is not None:
        record[:4].view(np.int32)[0] = total
    rows = track_rows_of(outputs, b, counter.max_boxes)
    return torch.from_numpy(record).to(cuda), torch.from_numpy(rows).to(cuda), counts


def _launch(counter, outputs, total, cuda, fill=0xAB):
    import torch
    b = len(outputs)
    record, rows, _ = _device_inputs(counter, outputs, total, cuda)
    out = torch.full((counter.out_bytes(b),), fill, dtype=torch.uint8, device=cuda)
    counter.launch(record, rows, out, b)
    return out.cpu().numpy()


def _split(out, b, max_boxes):
    at = b * max_boxes * ref.PERSON.itemsize
    return out[:at].view(ref.PERSON), out[at:].view(ref.IMAGE)


def _same(out, persons, images, max_boxes, what):
    got_p, got_i = _split(out, len(images), max_boxes)
    for name in ref.PERSON.names:
        np.testing.assert_array_equal(got_p[name].view(np.uint64) if name == 'anchor' else got_p[name],
                                      persons[name].view(np.uint64) if name == 'anchor' else persons[name],
                                      err_msg=f"{what}: person rows, {name}")
    for name in ref.IMAGE.names:
        np.testing.assert_array_equal(got_i[name], images[name], err_msg=f"{what}: image rows, {name}")
    assert out.tobytes() == persons.tobytes() + images.tobytes(), what


def _same_state(got, want, what):
    g, w = np.frombuffer(got, ref.STATE), np.frombuffer(want, ref.STATE)
    for name in ('frames', 'zone_entries', 'zone_exits', 'line_positive', 'line_negative'):
        np.testing.assert_array_equal(g[name], w[name], err_msg=f"{what}: state, {name}")
    for name in ref.SLOT.names:
        np.testing.assert_array_equal(g['slots'][name], w['slots'][name], err_msg=f"{what}: state slots, {name}")
    assert got == want, what


@pytest.mark.parametrize("name", SINGLE + PAIRED)
def test_rows_and_state_equal_the_reference(cuda, reference, name):
    c, streams = _case(name), _streams(name)
    persons, images, state = reference[name]
    assert 2 <= len(images) <= 8
    counter = _counter(c, streams)
    out = _launch(counter, cases.outputs_of(c['frames']), c['total'], cuda)
    _same(out, persons, images, c['max_boxes'], name)
    assert not counter.prev.cpu().numpy().any()                     # the launch alone advances nothing
    counter.commit()
    _same_state(counter.prev.cpu().numpy().tobytes(), state, name)


@pytest.mark.parametrize("name", [n for n in SINGLE + PAIRED if _case(n)['total'] is None])
def test_the_state_carries_over_every_cut(cuda, reference, name):
    """The frames of every stream split over two calls, at every cut, with a commit between: the rows and the final state of the
    one call."""
    c, streams = _case(name), _streams(name)
    persons, images, state = reference[name]
    outputs = cases.outputs_of(c['frames'])
    F, mb = len(outputs) // streams, c['max_boxes']
    counts = [len(f) for f in c['frames']]
    starts = np.concatenate([[0], np.cumsum(counts)])
    for cut in range(1, F):
        counter = _counter(c, streams)
        for part in (range(0, cut), range(cut, F)):
            which = [s * F + f for s in range(streams) for f in part]
            out = _launch(counter, [outputs[i] for i in which], None, cuda)
            counter.commit()
            want_p = np.zeros(len(which) * mb, ref.PERSON)          # the rows of these images, dense, as a record of them has them
            at = 0
            for i in which:
                want_p[at:at + counts[i]] = persons[starts[i]:starts[i] + counts[i]]
                at += counts[i]
            _same(out, want_p, images[which], mb, f"{name} cut {cut} frames {list(part)}")
        _same_state(counter.prev.cpu().numpy().tobytes(), state, f"{name} cut {cut}")


def test_the_launch_is_pure(cuda, reference):
    """Two launches before the commit write the same bytes, whatever the buffers held, and leave prev alone."""
    import torch
    from multiposenet_amd import _lib
    name = 'line_gap'
    c = cases.BY_NAME[name]
    outputs = cases.outputs_of(c['frames'])
    counter = _counter(c, 1)
    _launch(counter, outputs[:2], None, cuda)
    counter.commit()
    before = counter.prev.cpu().numpy().tobytes()
    outs, states = [], []
    for fill in (0xAB, 0x00):
        counter.next.fill_(fill)
        outs.append(_launch(counter, outputs[2:], None, cuda, fill).tobytes())
        states.append(counter.next.cpu().numpy().tobytes())
        assert counter.prev.cpu().numpy().tobytes() == before
    assert outs[0] == outs[1] and states[0] == states[1] == reference[name][2]
    record, rows, _ = _device_inputs(counter, outputs[2:], None, cuda)
    out = torch.zeros(counter.out_bytes(2), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match="zone_events: prev and next are one buffer"):
        _lib.call("mpn_zone_events", _lib.ptr(record), _lib.ptr(rows), 2, counter.max_boxes, 1, _lib.ptr(counter.table),
                  _lib.ptr(counter.prev), _lib.ptr(counter.prev), _lib.ptr(out), None)


def test_update_unpack_totals_and_reset(cuda, reference):
    """`update` is the launch plus the commit for host dicts; `unpack` names the rows; `totals` reads the counters by name."""
    name = 'line_gap+id_change'
    c = _case(name)
    persons, images, state = reference[name]
    counter = _counter(c, 2)
    outputs = cases.outputs_of(c['frames'])
    got = counter.update(outputs)
    _same(counter.last_out, persons, images, c['max_boxes'], name)
    _same_state(counter.prev.cpu().numpy().tobytes(), state, name)
    counts = [len(f) for f in c['frames']]
    want = ref.unpacked(cases.geometry(c['geo']), persons, images, counts, c['max_boxes'])
    for g, w in zip(got, want):
        for key, value in w.items():
            assert g[key].dtype == value.dtype and g[key].shape == value.shape, key
            np.testing.assert_array_equal(g[key], value, err_msg=key)
    assert got[0]['inside'].shape == (2, 3) and got[0]['crossed_positive'].shape == (2, 1) and got[2]['inside'].shape == (0, 3)
    assert counter.totals(0) == {'frames': 4, 'entries': {'square': 1, 'triangle': 0, 'concave': 0},
                                 'exits': {'square': 0, 'triangle': 0, 'concave': 0}, 'line_positive': {'gate': 1},
                                 'line_negative': {'gate': 0}}
    assert counter.totals(1)['entries'] == {'square': 2, 'triangle': 0, 'concave': 0}
    counter.reset(stream=1)
    assert counter.totals(1)['frames'] == 0 and counter.totals(0)['frames'] == 4
    with pytest.raises(ValueError, match="track_ids"):
        counter.update([{k: v for k, v in o.items() if k != 'track_ids'} for o in outputs])


def test_records_without_keypoints_take_the_box(cuda):
    """Dicts without 'keypoints' (a Detector without the PRN): the zeros of the record do not pass for ankles."""
    c = cases.BY_NAME['box_bottom']
    feet = _counter(dict(c, geo=dict(cases.STANDARD)), 1)
    got = feet.update(cases.outputs_of(c['frames'], keypoints=False))
    state = ref.new_state(1)
    persons, images = ref.run(cases.geometry(c['geo']), cases.outputs_of(c['frames'], keypoints=False), state, c['max_boxes'])
    _same(feet.last_out, persons, images, c['max_boxes'], "no keypoints")
    assert not got[0]['anchor_from_keypoints'].any() and got[0]['tracked'].all()
