"""GPU: mpn_track_eval through `track_metrics.TrackEvaluator.update` on the handmade cases of tests/track_eval_cases.py, against the
plain-loop definition tests/track_eval_ref.py: rows and state byte for byte, the similarities to rtol 1e-12 (exp is within an
ulp of numpy's; no decision of the reference is within 1e-9 of flipping, tests/test_track_eval_host.py)."""
import numpy as np
import pytest

import track_eval_cases as cases
import track_eval_ref as ref

pytestmark = pytest.mark.gpu

MAX_IDENTITIES, MAX_BOXES, MAX_GT = 256, 64, 64
NAMES = [c['name'] for c in cases.CASES]
BY_NAME = {c['name']: c for c in cases.CASES}


@pytest.fixture(scope="module")
def reference():
    """name -> (results per image, packed state) of the definition, computed once."""
    out = {}
    for c in cases.CASES:
        state = ref.new_state(c['streams'], MAX_IDENTITIES)
        out[c['name']] = (ref.run(c['outputs'], c['groundtruth'], c['identities'], state, c['threshold']), ref.pack_state(state))
    return out


def _evaluator(c):
    from multiposenet_amd.track_metrics import TrackEvaluator
    return TrackEvaluator(streams=c['streams'], threshold=c['threshold'], max_gt=MAX_GT, max_identities=MAX_IDENTITIES,
                          max_boxes=MAX_BOXES)


def _update(ev, c, which):
    given = [c['identities'][i] for i in which] if c['raw_identities'] else None
    return ev.update([c['outputs'][i] for i in which], [c['groundtruth'][i] for i in which], identities=given)


def _same_tables(out, want, what):
    """The raw rows of a call against `ref.tables` of the reference's results for the same images."""
    b = len(want)
    frame, gt, hyp = ref.tables(want, MAX_BOXES, MAX_GT)
    assert len(out) == frame.nbytes + gt.nbytes + hyp.nbytes
    got_frame = out[:frame.nbytes].view(ref.FRAME)
    got_gt = out[frame.nbytes:frame.nbytes + gt.nbytes].view(ref.GT).reshape(b, MAX_GT)
    got_hyp = out[frame.nbytes + gt.nbytes:].view(ref.HYP)
    assert got_hyp.tobytes() == hyp.tobytes(), what
    for name in ref.FRAME.names:
        if name != 'similarity_sum':
            np.testing.assert_array_equal(got_frame[name], frame[name], err_msg=f"{what} frame {name}")
    for name in ref.GT.names:
        if name != 'similarity':
            np.testing.assert_array_equal(got_gt[name], gt[name], err_msg=f"{what} ground truth {name}")
    np.testing.assert_allclose(got_frame['similarity_sum'], frame['similarity_sum'], rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(got_gt['similarity'], gt['similarity'], rtol=1e-12, atol=0, err_msg=what)
    assert ((got_gt['similarity'] == 1.0) == (gt['similarity'] == 1.0)).all(), what     # exact where the poses are equal


@pytest.mark.parametrize("name", NAMES)
def test_update_equals_the_reference(cuda, reference, name):
    c = BY_NAME[name]
    want, want_state = reference[name]
    ev = _evaluator(c)
    got = _update(ev, c, range(len(want)))
    _same_tables(ev.last_out, want, name)
    assert ev.prev.cpu().numpy().tobytes() == want_state and ev.next.cpu().numpy().tobytes() == want_state
    F = len(want) // c['streams']
    for i, (g, w) in enumerate(zip(got, want)):                     # what `unpack` makes of the rows
        assert g['stream'] == i // F and g['matches'] == int(w['frame']['matches'])
        np.testing.assert_array_equal(g['gt_track_ids'], w['gt']['track_id'])
        np.testing.assert_array_equal(g['gt_switch'], (w['gt']['flags'] & ref.GT_SWITCH) != 0)
        np.testing.assert_array_equal(g['gt_identities'], c['identities'][i] if not c['raw_identities'] else g['gt_identities'])
        np.testing.assert_array_equal(g['person_gt'], w['hyp']['gt'])
        np.testing.assert_array_equal(g['person_false_positive'], (w['hyp']['flags'] & ref.HYP_FALSE_POSITIVE) != 0)
    stats = ev.evaluate()
    for key, value in c['expect'].items():                          # the numbers written out by hand in the case table
        assert abs(stats[key] - value) < 1e-12, (key, stats[key], value)
    if name != 'full':
        brute = ref.metrics(want, c['outputs'], c['identities'], c['streams'])
        for key in ('mota', 'idf1', 'idtp', 'num_switches', 'num_fragmentations', 'mostly_tracked', 'mostly_lost'):
            assert stats[key] == brute[key] or (stats[key] != stats[key] and brute[key] != brute[key]), key


@pytest.mark.parametrize("name", [c['name'] for c in cases.CASES if len(c['outputs']) // c['streams'] > 1])
def test_the_state_carries_over_every_cut(cuda, reference, name):
    """The frames of every stream split over two calls, at every cut: the rows of the one call."""
    c = BY_NAME[name]
    want, want_state = reference[name]
    streams, F = c['streams'], len(want) // c['streams']
    for cut in range(1, F):
        ev = _evaluator(c)
        for part in (range(0, cut), range(cut, F)):
            which = [s * F + f for s in range(streams) for f in part]
            _update(ev, c, which)
            _same_tables(ev.last_out, [want[i] for i in which], f"{name} cut {cut} frames {part}")
        assert ev.prev.cpu().numpy().tobytes() == want_state
        assert ev.state(0)['frames'] == F


def test_the_launch_is_pure(cuda, reference):
    """Two launches before the commit write the same bytes and leave prev alone; the commit is what advances the state."""
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    from multiposenet_amd.track_metrics import _TRACK_ROW
    c = BY_NAME['video_1']
    want, want_state = reference['video_1']
    ev = _evaluator(c)
    first, second = list(range(0, 8)), list(range(8, 16))
    _update(ev, c, first)
    before = ev.prev.cpu().numpy().tobytes()
    b = len(second)
    record, _ = fill_record([c['outputs'][i] for i in second], b, MAX_BOXES)
    rows = np.zeros(b * MAX_BOXES, _TRACK_ROW)
    ids = np.concatenate([c['outputs'][i]['track_ids'] for i in second])
    rows['track_id'][:len(ids)] = ids
    record, rows = torch.from_numpy(record).to(cuda), torch.from_numpy(rows.view(np.uint8)).to(cuda)
    ev.place([c['groundtruth'][i] for i in second], b)
    outs = [torch.full((ev.out_bytes(b),), 0xAB, dtype=torch.uint8, device=cuda) for _ in range(2)]
    states = []
    for out in outs:
        ev.launch(record, rows, out, b)
        states.append(ev.next.cpu().numpy().tobytes())
        assert ev.prev.cpu().numpy().tobytes() == before
    assert states[0] == states[1] == want_state
    assert outs[0].cpu().numpy().tobytes() == outs[1].cpu().numpy().tobytes()
    _same_tables(outs[0].cpu().numpy(), [want[i] for i in second], "pure")
    ev.commit()
    assert ev.prev.cpu().numpy().tobytes() == want_state
    with pytest.raises(ValueError, match="pure function"):
        from multiposenet_amd import _lib
        _lib.call("mpn_track_eval", _lib.ptr(record), _lib.ptr(rows), b, MAX_BOXES, 1, _lib.ptr(ev.buffers(b).dev),
                  _lib.ptr(ev.buffers(b).dev), _lib.ptr(ev.buffers(b).dev), MAX_GT, MAX_IDENTITIES, 0.5, _lib.ptr(ev.prev),
                  _lib.ptr(ev.prev), ev.state_bytes, _lib.ptr(outs[0]), outs[0].numel(), None)


def test_identities_run_out_and_reset(cuda):
    from multiposenet_amd.track_metrics import TrackEvaluator
    ev = TrackEvaluator(streams=2, max_identities=2, max_boxes=8)
    one = cases.case('x', [([cases.person(1, *cases.A)], [cases.truth(5, *cases.A), cases.truth(6, *cases.B)])] * 2, streams=2)
    ev.update(one['outputs'], one['groundtruth'])
    assert ev.state(0)['identities'] == {5: 0, 6: 1} and ev.state(1)['track_ids'].tolist() == [1, 0]
    more = cases.case('y', [([cases.person(1, *cases.A)], [cases.truth(7, *cases.A)])] * 2, streams=2)
    before = ev.prev.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="max_identities = 2"):
        ev.update(more['outputs'], more['groundtruth'])
    assert ev.prev.cpu().numpy().tobytes() == before and ev.state(0)['identities'] == {5: 0, 6: 1}
    ev.reset(stream=0)
    assert ev.state(0)['frames'] == 0 and ev.state(0)['identities'] == {} and ev.state(1)['frames'] == 1
    with pytest.raises(ValueError, match="max_identities = 2"):     # stream 1 is still full
        ev.update(more['outputs'], more['groundtruth'])
    ev.reset()
    got = ev.update(more['outputs'], more['groundtruth'])
    assert [g['gt_identities'].tolist() for g in got] == [[0], [0]] and not ev.next.cpu().numpy().view(np.int32)[5:6].any()
    stats = ev.evaluate()                                           # a reset starts new identities: 5 and 7 are told apart
    assert stats['num_unique_objects'] == 6 and stats['num_frames'] == 4
