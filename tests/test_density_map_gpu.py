"""GPU: mpn_density_map through `density.DensityMap.launch` on the handmade cases of tests/density_cases.py, against the
plain-loop definition tests/density_ref.py: rows, state and snapshots byte for byte. No tolerance: the anchor is IEEE f64
operations, the rest is integers."""
import numpy as np
import pytest

import density_cases as cases
import density_ref as ref

pytestmark = pytest.mark.gpu

SINGLE = [c['name'] for c in cases.CASES]
PAIRED = ['+'.join(p) for p in cases.PAIRS]


def _case(name):
    return cases.pair(*name.split('+')) if '+' in name else cases.BY_NAME[name]


def _streams(name):
    return 2 if '+' in name else 1


def _start(name):
    return cases.pair_state(*name.split('+')) if '+' in name else cases.preloaded(cases.BY_NAME[name])


@pytest.fixture(scope="module")
def reference():
    """name -> (out bytes, snapshots, state bytes) of the definition over the whole case, computed once."""
    out = {}
    for name in SINGLE + PAIRED:
        c = _case(name)
        state = _start(name)
        rows, images, snaps = ref.run(cases.reference_params(c['params']), cases.outputs_of(c['frames']), state, c['max_boxes'],
                                      c['total'], c['tracked'])
        out[name] = rows, images, snaps, state.tobytes()
    return out


def _density(c, streams, start=None):
    import torch
    from multiposenet_amd.density import DensityMap
    d = DensityMap(streams=streams, max_boxes=c['max_boxes'], **c['params'])
    if start is not None:
        d.prev.copy_(torch.from_numpy(np.frombuffer(start.tobytes(), np.uint8).copy()))
    return d


def _device_inputs(density, outputs, total, cuda, tracked=True):
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    from multiposenet_amd.zones import track_rows_of
    b = len(outputs)
    record, counts = fill_record(outputs, b, density.max_boxes)
    if total is not None:
        record[:4].view(np.int32)[0] = total
    rows = torch.from_numpy(track_rows_of(outputs, b, density.max_boxes)).to(cuda) if tracked else None
    return torch.from_numpy(record).to(cuda), rows, counts


def _launch(density, outputs, total, cuda, fill=0xAB, tracked=True):
    """-> (out bytes, snapshots uint32 [b, gh, gw])."""
    import torch
    b = len(outputs)
    record, rows, _ = _device_inputs(density, outputs, total, cuda, tracked)
    out = torch.full((density.out_bytes(b),), fill, dtype=torch.uint8, device=cuda)
    snaps = density.snapshots(b)
    snaps.fill_(fill)
    density.launch(record, rows, out, b, snapshots=snaps)
    return out.cpu().numpy(), snaps.cpu().numpy().view(np.uint32).reshape(b, density.gh, density.gw)


def _same(got, rows, images, what):
    out, snaps = got
    b = len(images)
    got_rows = out[:rows.nbytes].view(ref.ROW)
    got_images = out[rows.nbytes:].view(ref.IMAGE)
    assert len(got_images) == b
    for name in ref.ROW.names:
        np.testing.assert_array_equal(got_rows[name], rows[name], err_msg=f"{what}: rows, {name}")
    for name in ref.IMAGE.names:
        np.testing.assert_array_equal(got_images[name], images[name], err_msg=f"{what}: image rows, {name}")
    assert out.tobytes() == ref.packed(rows, images).tobytes(), what


def _same_state(got, want, gh, gw, what):
    g, w = np.frombuffer(got, ref.state_dtype(gh, gw)), np.frombuffer(want, ref.state_dtype(gh, gw))
    for name in ('frames', 'max_dwell', 'max_visits', 'pad', 'dwell', 'visits'):
        np.testing.assert_array_equal(g[name], w[name], err_msg=f"{what}: state, {name}")
    for name in ref.SLOT.names:
        np.testing.assert_array_equal(g['slots'][name], w['slots'][name], err_msg=f"{what}: state slots, {name}")
    assert got == want, what


@pytest.mark.parametrize("name", SINGLE + PAIRED)
def test_rows_state_and_snapshots_equal_the_reference(cuda, reference, name):
    c, streams = _case(name), _streams(name)
    rows, images, snaps, state = reference[name]
    start = _start(name)
    density = _density(c, streams, start)
    got = _launch(density, cases.outputs_of(c['frames']), c['total'], cuda, tracked=c['tracked'])
    _same(got, rows, images, name)
    np.testing.assert_array_equal(got[1], snaps, err_msg=f"{name}: snapshots")
    assert density.prev.cpu().numpy().tobytes() == start.tobytes()  # the launch alone advances nothing
    density.commit()
    _same_state(density.prev.cpu().numpy().tobytes(), state, density.gh, density.gw, name)


@pytest.mark.parametrize("name", [n for n in SINGLE + PAIRED if _case(n)['total'] is None])
def test_the_state_carries_over_every_cut(cuda, reference, name):
    """The frames of every stream split over two calls, at every cut, with a commit between: the rows, the snapshots and the
    final state of the one call."""
    c, streams = _case(name), _streams(name)
    rows, images, snaps, state = reference[name]
    outputs = cases.outputs_of(c['frames'])
    F, mb = len(outputs) // streams, c['max_boxes']
    counts = [len(f) for f in c['frames']]
    starts = np.concatenate([[0], np.cumsum(counts)])
    for cut in range(1, F):
        density = _density(c, streams, _start(name))
        for part in (range(0, cut), range(cut, F)):
            which = [s * F + f for s in range(streams) for f in part]
            got = _launch(density, [outputs[i] for i in which], None, cuda, tracked=c['tracked'])
            density.commit()
            want = np.zeros(len(which) * mb, ref.ROW)               # the rows of these images, dense, as a record of them has them
            at = 0
            for i in which:
                want[at:at + counts[i]] = rows[starts[i]:starts[i] + counts[i]]
                at += counts[i]
            _same(got, want, images[which], f"{name} cut {cut} frames {list(part)}")
            np.testing.assert_array_equal(got[1], snaps[which], err_msg=f"{name} cut {cut}: snapshots")
        _same_state(density.prev.cpu().numpy().tobytes(), state, density.gh, density.gw, f"{name} cut {cut}")


def test_the_launch_is_pure(cuda, reference):
    """Two launches before the commit write the same bytes, whatever the buffers held, and leave prev alone; without snapshots
    the rows and the state are the same."""
    import torch
    from multiposenet_amd import _lib
    name = 'wander'
    c = cases.BY_NAME[name]
    outputs = cases.outputs_of(c['frames'])
    density = _density(c, 1)
    _launch(density, outputs[:2], None, cuda)
    density.commit()
    before = density.prev.cpu().numpy().tobytes()
    outs, states = [], []
    for fill in (0xAB, 0x00):
        density.next.fill_(fill)
        got = _launch(density, outputs[2:], None, cuda, fill)
        outs.append(got[0].tobytes() + got[1].tobytes())
        states.append(density.next.cpu().numpy().tobytes())
        assert density.prev.cpu().numpy().tobytes() == before
    assert outs[0] == outs[1] and states[0] == states[1] == reference[name][3]
    record, rows, _ = _device_inputs(density, outputs[2:], None, cuda)
    out = torch.zeros(density.out_bytes(2), dtype=torch.uint8, device=cuda)
    density.next.fill_(0x5A)
    density.launch(record, rows, out, 2)                            # no snapshots
    assert out.cpu().numpy().tobytes() + outs[0][len(out):] == outs[0] and density.next.cpu().numpy().tobytes() == states[0]
    with pytest.raises(ValueError, match="density_map: prev and next are one buffer"):
        _lib.call("mpn_density_map", _lib.ptr(record), _lib.ptr(rows), 2, density.max_boxes, 1, 48, 80, 8, 0, 0, 0.0, 1, 0, 0,
                  _lib.ptr(density.prev), _lib.ptr(density.prev), _lib.ptr(out), None, None)


def test_update_grid_unpack_and_reset(cuda, reference):
    """`update` is the launch plus the commit for host dicts; `unpack` names the rows; `grid` reads a plane."""
    name = 'wander+leave_and_reenter'
    c = _case(name)
    rows, images, _, state = reference[name]
    density = _density(c, 2)
    outputs = cases.outputs_of(c['frames'])
    got = density.update(outputs)
    assert density.last_out.tobytes() == ref.packed(rows, images).tobytes()
    _same_state(density.prev.cpu().numpy().tobytes(), state, 6, 10, name)
    want = ref.unpacked(rows, images, [len(f) for f in c['frames']])
    for g, w in zip(got, want):
        assert set(g) == set(w) == {'cell', 'cells', 'tracked', 'visit', 'outside', 'anchor_from_keypoints', 'max_dwell', 'max_visits',
                                    'counted', 'visits'}
        for key, value in w.items():
            if isinstance(value, int):
                assert type(g[key]) is int and g[key] == value, key
            else:
                assert g[key].dtype == value.dtype and g[key].shape == value.shape, key
                np.testing.assert_array_equal(g[key], value, err_msg=key)
    assert got[0]['cell'].tolist() == [[2, 2]] and got[5]['cell'].tolist() == [[-1, -1]] and got[5]['outside'].tolist() == [True]
    final = np.frombuffer(state, ref.state_dtype(6, 10))
    for s in range(2):
        for plane in ('dwell', 'visits'):
            grid = density.grid(s, plane)
            assert grid.dtype == np.uint32 and grid.shape == (6, 10)
            np.testing.assert_array_equal(grid, final[s][plane])
    assert int(density.grid(0)[2, 2]) == 3 and int(density.grid(1, 'visits')[2, 2]) == 2
    assert int(density.state(0)['frames']) == 4 and int(density.state(1)['frames']) == 4
    density.reset(stream=1)
    assert int(density.state(1)['frames']) == 0 and not density.grid(1).any() and int(density.grid(0)[2, 2]) == 3
    density.reset()
    assert not density.prev.cpu().numpy().any() and not density.next.cpu().numpy().any()
    with pytest.raises(ValueError, match="plane must be one of"):
        density.grid(0, 'both')
    # dicts without 'track_ids': the dwell plane alone - the launch without track rows
    untracked = cases.BY_NAME['untracked_launch']
    alone = _density(untracked, 1)
    alone.update(cases.outputs_of(untracked['frames'], track_ids=False))
    assert alone.last_out.tobytes() == ref.packed(*reference['untracked_launch'][:2]).tobytes()
    assert alone.prev.cpu().numpy().tobytes() == reference['untracked_launch'][3]
    shown = _density(dict(untracked, params=cases.params(show='visits')), 1)
    with pytest.raises(ValueError, match="show='visits'.*'track_ids'"):
        shown.update(cases.outputs_of(untracked['frames'], track_ids=False))
    with pytest.raises(ValueError, match="needs 'boxes' and 'scores'"):
        alone.update([{'scores': np.zeros(0, np.float32)}])


def test_records_without_keypoints_take_the_box(cuda):
    """Dicts without 'keypoints' (a Detector without the PRN): the zeros of the record do not pass for ankles."""
    c = cases.BY_NAME['box_bottom']
    feet = _density(dict(c, params=cases.params()), 1)
    outputs = cases.outputs_of(c['frames'], keypoints=False)
    got = feet.update(outputs)
    p = cases.reference_params(c['params'])
    state = ref.new_state(1, p)
    rows, images, _ = ref.run(p, outputs, state, c['max_boxes'])
    assert feet.last_out.tobytes() == ref.packed(rows, images).tobytes() and feet.prev.cpu().numpy().tobytes() == state.tobytes()
    assert not got[0]['anchor_from_keypoints'].any() and got[0]['tracked'].all() and got[0]['cell'].tolist() == [[2, 3], [-1, -1]]


def test_the_largest_grid_with_full_rows(cuda):
    """1024 x 1024 frames at cell = 8: G = 16384, the cap; the box footprint; 64 rows a frame, one of them over every cell."""
    rng = np.random.RandomState(5)
    frames = []
    for f in range(2):
        persons = []
        for i in range(64):
            x, y = int(rng.randint(0, 1024)), int(rng.randint(0, 1024))
            w, h = int(rng.randint(1, 200)), int(rng.randint(1, 200))
            box = (x - w // 2, y - h, x + w - w // 2, y + 3) if i else (-3, -3, 1030, 1030)
            q = cases.person(1 + (i + f) % 70, x, y, box=box)
            q['box'] = np.array([box[1] / 1024, box[0] / 1024, box[3] / 1024, box[2] / 1024], np.float32)
            persons.append(q)
        frames.append(persons)
    c = cases.case('cap', dict(frame_size=(1024, 1024), cell=8, footprint='box', half_life=2), frames, max_boxes=64)
    p = cases.reference_params(c['params'])
    assert p.gh * p.gw == 16384
    state = ref.new_state(1, p)
    outputs = cases.outputs_of(frames)
    rows, images, snaps = ref.run(p, outputs, state, 64)
    density = _density(c, 1)
    got = _launch(density, outputs, None, cuda)
    _same(got, rows, images, 'cap')
    np.testing.assert_array_equal(got[1], snaps)
    density.commit()
    _same_state(density.prev.cpu().numpy().tobytes(), state.tobytes(), 128, 128, 'cap')
    assert int(rows['cells'].max()) == 16384 and int(images['max_dwell'][1]) >= 2 and (rows['cells'][:128] > 0).sum() > 100
