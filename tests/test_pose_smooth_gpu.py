"""GPU: mpn_pose_smooth against the plain-loop reference (tests/smooth_ref.py). `out`, `next` and the untouched `prev` are
compared as bytes - every operation of the definition is one correctly rounded float32 operation, so no tolerance applies.
Records come from pose_metrics.fill_record; track rows are handcrafted or mpn_pose_track's own on tests/track_cases.py."""
import copy

import numpy as np
import pytest

import smooth_ref as ref
import track_cases as cases

pytestmark = pytest.mark.gpu

K = 17


def _person(rng, cx=300.0, cy=200.0, spread=80.0, score=0.9):
    kp = np.zeros((K, 3), np.float32)
    kp[:, 0] = cx + rng.uniform(-spread, spread, K)
    kp[:, 1] = cy + rng.uniform(-spread, spread, K)
    kp[:, 2] = score
    return kp


def _image(persons):
    n = len(persons)
    return {'scores': np.full(n, 0.9, np.float32), 'keypoints': np.array(persons, np.float32).reshape(n, K, 3)}


def _track_rows(ids, slots, B, max_boxes):
    from multiposenet_amd import tracking
    rows = np.zeros(B * max_boxes, tracking._OUT)
    rows['track_id'][:len(ids)] = ids
    rows['slot'][:len(ids)] = slots
    rows['hits'][:len(ids)] = 1                                     # fields the kernel must not read
    rows['similarity'][:len(ids)] = 0.5
    return rows


def _device_launch(cuda, record, track, B, max_boxes, streams, max_tracks, p, prev):
    """One launch from the state bytes `prev` -> (out bytes, next bytes, prev bytes afterwards). out and next start as 0xff."""
    import torch
    from multiposenet_amd import _lib
    lib = _lib.lib()
    assert len(prev) == lib.mpn_pose_smooth_state_bytes(streams, max_tracks)
    record_dev = torch.from_numpy(record).to(cuda)
    track_dev = torch.from_numpy(track.view(np.uint8).copy()).to(cuda)
    prev_dev = torch.from_numpy(np.frombuffer(prev, np.uint8).copy()).to(cuda)
    next_dev = torch.full_like(prev_dev, 255)
    out_dev = torch.full((lib.mpn_pose_smooth_out_bytes(B, max_boxes),), 255, dtype=torch.uint8, device=cuda)
    _lib.call("mpn_pose_smooth", _lib.ptr(record_dev), _lib.ptr(track_dev), B, max_boxes, streams, max_tracks, float(p.rate),
              float(p.min_cutoff), float(p.beta), float(p.d_cutoff), float(p.min_keypoint_score), _lib.ptr(prev_dev),
              _lib.ptr(next_dev), _lib.ptr(out_dev), _lib.stream_ptr())
    return out_dev.cpu().numpy().tobytes(), next_dev.cpu().numpy().tobytes(), prev_dev.cpu().numpy().tobytes()


def _check(cuda, images, ids, slots, max_boxes, state, p, msg, trace=None):
    """One launch over `images` (result dicts, b = streams * F) with handcrafted track rows, against the reference from `state`
    (a list of smooth_ref.Stream). Returns (the reference's new state, out bytes, keypoints, velocities)."""
    from multiposenet_amd.pose_metrics import fill_record
    B, streams, max_tracks = len(images), len(state), len(state[0].id)
    record, counts = fill_record(images, B, max_boxes)
    track = _track_rows(ids, slots, B, max_boxes)
    total = int(sum(counts))
    assert total == len(ids)
    kp = np.concatenate([o['keypoints'].reshape(-1, K, 3) for o in images]) if total else np.zeros((0, K, 3), np.float32)
    (want, want_vel), new_state = ref.launch(kp, counts, track[:total], state, p, trace)
    prev = ref.pack_state(state)
    out, nxt, prev_after = _device_launch(cuda, record, track, B, max_boxes, streams, max_tracks, p, prev)
    assert prev_after == prev, f"{msg}: prev was written"
    assert out == ref.pack_rows(want, want_vel, B, max_boxes), f"{msg}: out"
    assert nxt == ref.pack_state(new_state), f"{msg}: next"
    return new_state, out, want, want_vel


def test_smallest(cuda):
    """B = 1, max_boxes = 1, max_tracks = 1, one tracked person that moves."""
    rng = np.random.RandomState(0)
    p = ref.Params()
    state = ref.new_state(1, 1)
    for f in range(4):
        state, _, kp, vel = _check(cuda, [_image([_person(rng, 300 + 5 * f)])], [1], [0], 1, state, p, f"frame {f}")
        assert vel.any() == (f > 0)
    assert state[0].frames == 4


def test_gap_reset_untracked_and_empty_frame(cuda):
    """streams = 1, F = 5, max_boxes = 3, max_tracks = 4. Person A (id 1, slot 0) is there in frames 1, 2 and 5: gap 3. B (id 2,
    slot 1) gives its slot to C (id 3) in the next frame: reset. One row of frame 1 is untracked; frame 3 is empty. Then the
    same five frames' successors in a second launch, every filter continuing."""
    rng = np.random.RandomState(1)
    p = ref.Params(beta=0.05)
    state = ref.new_state(1, 4)
    for call in range(2):
        A = [_person(rng, 100 + 4 * f, 150) for f in range(5)]
        C = [_person(rng, 400, 250 + 3 * f) for f in range(5)]
        images = [_image([A[0], _person(rng, 400, 240), _person(rng, 550, 100)]), _image([A[1], C[1]]), _image([]), _image([C[3]]),
                  _image([A[4], C[4]])]
        first_slot1 = 2 if call == 0 else 3
        ids, slots = [1, first_slot1, 0, 1, 3, 3, 1, 3], [0, 1, -1, 0, 1, 1, 0, 1]
        trace = []
        state, _, kp, vel = _check(cuda, images, ids, slots, 3, state, p, f"call {call}", trace)
        assert state[0].frames == 5 * (call + 1)
        assert np.float32(np.float32(3) / p.rate) in trace          # A's sample of frame 5 has te = 3 / rate
        assert not vel[2].any() and kp[2].tobytes() == images[0]['keypoints'][2].tobytes()      # the untracked row
        if call == 0:
            assert not vel[4].any() and vel[5].all()                # C: first sample in frame 2 (the reset), filtered in frame 4
            assert not vel[0].any() and vel[3].all() and vel[6].all()
        else:
            assert vel[0].all() and vel[1].all()                    # both continue over the launches; C took B's slot for good
    assert list(state[0].id) == [1, 3, 0, 0] and (state[0].last[:2] == 10).all()


def test_bad_slots_are_untracked(cuda):
    """A slot of -1, 64, -5 or 2^30 beside a positive id, and one inside the 64 of the kernel's LDS but not below max_tracks:
    treated as untracked, nothing else changes."""
    rng = np.random.RandomState(2)
    p = ref.Params()
    state = ref.new_state(1, 8)
    images = [_image([_person(rng, 100 * i) for i in range(6)]), _image([_person(rng, 100 * i + 3) for i in range(6)])]
    ids = [7, 7, 7, 7, 7, 1] * 2
    bad = [-1, 64, -5, 2 ** 30, 8, 3] * 2
    state_bad, out_bad, _, vel = _check(cuda, images, ids, bad, 8, state, p, "bad slots")
    state_zero, out_zero, _, _ = _check(cuda, images, [0, 0, 0, 0, 0, 1] * 2, [-1, -1, -1, -1, -1, 3] * 2, 8, state, p, "id 0")
    assert out_bad == out_zero and ref.pack_state(state_bad) == ref.pack_state(state_zero)
    assert vel[11].all() and not vel[:11].any()
    assert list(state_bad[0].id) == [0, 0, 0, 1, 0, 0, 0, 0]


def test_full_load(cuda):
    """max_boxes = max_tracks = 64, F = 3, every row tracked, the slots a fixed permutation of the rows: 1088 items a frame, more
    than four passes of the block. Two launches, so that all 64 x 17 filters run over a launch boundary as well."""
    rng = np.random.RandomState(3)
    p = ref.Params(beta=0.02)
    perm = [(37 * r + 11) % 64 for r in range(64)]
    assert sorted(perm) == list(range(64))
    state = ref.new_state(1, 64)
    for call in range(2):
        images = [_image([_person(rng, 10 * r + f, 5 * r - f) for r in range(64)]) for f in range(3)]
        state, _, _, vel = _check(cuda, images, list(range(1, 65)) * 3, perm * 3, 64, state, p, f"call {call}")
        assert vel[64:].all() and vel[:64].any() == (call == 1)
    assert [int(i) for i in state[0].id[perm]] == list(range(1, 65)) and (state[0].last == 6).all()


def _stream_images(rng, counts, shift=0.0):
    return [_image([_person(rng, 100 * (i + 1) + shift, 80 * (r + 1)) for r in range(n)]) for i, n in enumerate(counts)]


def test_streams_are_independent(cuda):
    """streams = 3, F = 2, different counts per image; changing stream 1's input leaves the rows and states of 0 and 2 equal."""
    from multiposenet_amd import _lib
    p = ref.Params()
    counts = [2, 3, 0, 1, 3, 2]
    ids = [1, 2, 1, 2, 3, 4, 1, 2, 3, 2, 1]
    slots = [0, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    results = []
    for shift in (0.0, 17.0):
        state = ref.new_state(3, 4)
        outs = []
        for call in range(2):
            rng = np.random.RandomState(10 + call)
            images = _stream_images(rng, counts)
            if shift:
                for o in images[2:4]:                               # stream 1 owns images 2 and 3
                    o['keypoints'][..., :2] += np.float32(shift)
            state, out, _, _ = _check(cuda, images, ids, slots, 3, state, p, f"shift {shift} call {call}")
            outs.append(out)
        results.append((outs, ref.pack_state(state)))
    stream_bytes = _lib.lib().mpn_pose_smooth_state_bytes(1, 4)
    (a_out, a_state), (b_out, b_state) = results
    for s in (0, 2):
        assert a_state[s * stream_bytes:(s + 1) * stream_bytes] == b_state[s * stream_bytes:(s + 1) * stream_bytes]
    assert a_state[stream_bytes:2 * stream_bytes] != b_state[stream_bytes:2 * stream_bytes]
    row = ref.ROW_BYTES
    for a, b in zip(a_out, b_out):                                  # rows 0..4 are stream 0's, row 5 stream 1's, 6..10 stream 2's
        assert a[:5 * row] == b[:5 * row] and a[6 * row:] == b[6 * row:] and a[5 * row:6 * row] != b[5 * row:6 * row]


def test_score_rule(cuda):
    """min_keypoint_score = 0.5: scores on both sides, exactly 0.5 (kept), the float32 below it and a NaN (rejected)."""
    rng = np.random.RandomState(4)
    p = ref.Params(min_keypoint_score=0.5)
    state = ref.new_state(1, 2)
    below = np.nextafter(np.float32(0.5), np.float32(0))
    for f in range(4):
        person = _person(rng, 200 + 7 * f)
        person[:, 2] = rng.choice(np.array([0.1, below, 0.5, 0.9, 1.0], np.float32), K)
        if f == 2:
            person[:5, 2] = (0.5, below, np.nan, 0.9, 0.4999)
        state, _, kp, vel = _check(cuda, [_image([person])], [1], [1], 2, state, p, f"frame {f}")
        if f == 2:
            assert not vel[0, 1].any() and not vel[0, 2].any() and not vel[0, 4].any()
            assert list(state[0].last[1, :5]) == [3, 0, 0, 3, 0]
    assert state[0].last[1].min() == 0 and state[0].last[1].max() == 4


def test_launch_is_pure_and_cuts_do_not_matter(cuda):
    """Two launches from the same prev give equal bytes and leave prev alone (an entry's first call in the Detector runs the
    device side twice); one F = 4 launch equals F = 2, copy, F = 2."""
    from multiposenet_amd.pose_metrics import fill_record
    rng = np.random.RandomState(5)
    p = ref.Params(beta=0.1)
    frames = [_image([_person(rng, 100 + 9 * f, 100), _person(rng, 400, 300 - 6 * f)]) for f in range(8)]
    ids, slots = [1, 2] * 4, [2, 0] * 4
    state = ref.new_state(1, 3)
    state, out0, _, _ = _check(cuda, frames[:4], ids, slots, 2, state, p, "warm-up")
    whole_state, whole_out, _, _ = _check(cuda, frames[4:], ids, slots, 2, state, p, "F = 4")
    record, _ = fill_record(frames[4:], 4, 2)
    again = _device_launch(cuda, record, _track_rows(ids, slots, 4, 2), 4, 2, 1, 3, p, ref.pack_state(state))
    assert again == (whole_out, ref.pack_state(whole_state), ref.pack_state(state))
    half, out_a, _, _ = _check(cuda, frames[4:6], ids[:4], slots[:4], 2, state, p, "first half")
    half, out_b, _, _ = _check(cuda, frames[6:], ids[:4], slots[:4], 2, half, p, "second half")
    row = ref.ROW_BYTES
    assert out_a[:4 * row] + out_b[:4 * row] == whole_out and ref.pack_state(half) == ref.pack_state(whole_state)


@pytest.mark.parametrize("rate", [30.0, 24000 / 1001, 1000.0])
def test_arithmetic(cuda, rate):
    """Coordinates of both signs with magnitudes 1e-3 .. 1e4 and jumps of thousands of pixels, for every beta and min_cutoff of
    the list; then a sample after 500 frames away, where min_cutoff = 1e6 makes r + 1 == r at rate 30. No intermediate of
    the reference's run is subnormal, so the comparison does not rest on denormal handling."""
    magnitudes = np.array([1e-3, 0.03, 0.7, 12.0, 345.0, 6789.0, 1e4, 2.5, 99.0], np.float32)
    for beta in (0.0, 0.007, 1.0):
        for min_cutoff in (0.05, 1.0, 1e6):
            rng = np.random.RandomState(6)
            p = ref.Params(rate=rate, min_cutoff=min_cutoff, beta=beta)
            state, trace = ref.new_state(1, 2), []
            for call in range(3):
                images = []
                for f in range(3):
                    persons = []
                    for r in range(2):
                        kp = np.zeros((K, 3), np.float32)
                        kp[:, :2] = rng.choice(magnitudes, (K, 2)) * rng.choice([-1, 1], (K, 2)) * rng.uniform(0.5, 1.0, (K, 2))
                        kp[:, 2] = 0.8
                        persons.append(kp)
                    images.append(_image(persons))
                msg = f"rate {rate} beta {beta} min_cutoff {min_cutoff} call {call}"
                state, _, _, vel = _check(cuda, images, [1, 2] * 3, [0, 1] * 3, 2, state, p, msg, trace)
                assert vel[2:].all()
                if call == 1:
                    state = copy.deepcopy(state)
                    state[0].frames += 500                          # the stream went on without these two persons
            assert len(trace) > 3000 and len(ref.subnormal(trace)) == 0 and np.isfinite(np.array(trace)).all()
            assert np.float32(np.float32(501) / p.rate) in trace
            if min_cutoff == 1e6 and rate == 30.0:
                assert np.float32(1) in trace                       # alpha = r / (r + 1) with r + 1 == r


@pytest.mark.parametrize("name", ["drift", "crossing", "absent_max_misses"])
def test_tracker_chain(cuda, name):
    """mpn_pose_track then mpn_pose_smooth through PoseTracker.launch_all, four frames a call, against track_ref and smooth_ref
    chained: the smooth launch reads the ids and slots the track launch wrote."""
    import torch
    from multiposenet_amd import tracking
    from multiposenet_amd.pose_metrics import fill_record
    _, max_tracks, frames = next(c for c in cases.cases() if c[0] == name)
    rows, _ = cases.reference([frames], max_tracks, 'iou')
    p = ref.Params(rate=25.0, min_cutoff=0.8, beta=0.01, min_keypoint_score=0.55)   # the scripts' scores are 0.5 + 0.02 k
    smooth = tracking.OneEuro(25.0, 0.8, 0.01, 1.0, 0.55)
    tracker = tracking.PoseTracker(1, max_tracks, 'iou', cases.MATCH_THRESHOLD, cases.MAX_MISSES, cases.NEW_TRACK_SCORE,
                                   cases.MAX_BOXES, smooth=smooth)
    F = 4
    out_dev = torch.zeros(tracker.out_bytes(F), dtype=torch.uint8, device=cuda)
    assert tracker.out_bytes(F) == F * cases.MAX_BOXES * (24 + ref.ROW_BYTES) and tracker.track_bytes(F) == F * cases.MAX_BOXES * 24
    state = ref.new_state(1, max_tracks)
    moved = False
    for at in range(0, cases.FRAMES, F):
        record, counts = fill_record(frames[at:at + F], F, cases.MAX_BOXES)
        out_dev.fill_(255)
        tracker.launch_all(torch.from_numpy(record).to(cuda), out_dev, F)
        want_rows = {'track_id': np.concatenate([rows[0][f]['track_ids'] for f in range(at, at + F)]),
                     'slot': np.concatenate([rows[0][f]['slots'] for f in range(at, at + F)])}
        kp = np.concatenate([frames[f]['keypoints'] for f in range(at, at + F)])
        (want, want_vel), state = ref.launch(kp, counts, want_rows, state, p)
        out = out_dev.cpu().numpy()
        got_rows = out[:tracker.track_bytes(F)].view(tracking._OUT)[:len(kp)]
        np.testing.assert_array_equal(got_rows['track_id'], want_rows['track_id'])
        np.testing.assert_array_equal(got_rows['slot'], want_rows['slot'])
        assert out[tracker.track_bytes(F):].tobytes() == ref.pack_rows(want, want_vel, F, cases.MAX_BOXES), (name, at)
        assert tracker.smooth_next.cpu().numpy().tobytes() == ref.pack_state(state), (name, at)
        unpacked = tracker.unpack(out, counts)
        assert unpacked[F - 1]['keypoints_smoothed'].tobytes() == want[len(kp) - counts[F - 1]:].tobytes()
        moved = moved or bool(want_vel.any())
        tracker.commit()
    assert moved and tracker.smooth_prev.cpu().numpy().tobytes() == ref.pack_state(state) and state[0].frames == cases.FRAMES


def test_update_reset_and_tracks(cuda):
    """PoseTracker.update() with smooth= on host dicts: the new keys, dtypes and shapes, the reference on the returned ids,
    reset(stream) clearing one stream's filters only, tracks()['frames']."""
    from multiposenet_amd.tracking import OneEuro, PoseTracker
    name, max_tracks, seqs = cases.pairs()[0]
    tracker = PoseTracker(2, max_tracks, 'iou', cases.MATCH_THRESHOLD, cases.MAX_MISSES, cases.NEW_TRACK_SCORE, cases.MAX_BOXES,
                          smooth=OneEuro())
    plain = PoseTracker(2, max_tracks, 'iou', cases.MATCH_THRESHOLD, cases.MAX_MISSES, cases.NEW_TRACK_SCORE, cases.MAX_BOXES)
    assert not hasattr(plain, 'smooth_prev') and plain.out_bytes(4) == 4 * cases.MAX_BOXES * 24
    p, ids = ref.Params(), ref.new_id_state(2)
    for at in (0, 2, 4):
        outputs = [o for seq in seqs for o in seq[at:at + 2]]
        got = tracker.update(outputs)
        base = plain.update(outputs)
        want = ref.run([dict(o, track_ids=g['track_ids']) for o, g in zip(outputs, got)], ids, p)
        for i, (o, g, b, w) in enumerate(zip(outputs, got, base, want)):
            n = len(o['scores'])
            assert set(g) == set(b) | {'keypoints_smoothed', 'keypoint_velocities'}
            for k in b:
                np.testing.assert_array_equal(g[k], b[k], err_msg=k)
            assert g['keypoints_smoothed'].shape == (n, K, 3) and g['keypoints_smoothed'].dtype == np.float32
            assert g['keypoint_velocities'].shape == (n, K, 2) and g['keypoint_velocities'].dtype == np.float32
            assert g['keypoints_smoothed'].tobytes() == w['keypoints_smoothed'].tobytes()
            assert g['keypoint_velocities'].tobytes() == w['keypoint_velocities'].tobytes()
            assert n >= 2 and bool(g['keypoint_velocities'].any()) == (at > 0 or i % 2 == 1)      # all but a stream's first frame
    t0, t1 = tracker.tracks(0), tracker.tracks(1)
    assert t0['frames'] == 6 and t1['frames'] == 6 and 'frames' not in plain.tracks(0)
    m = len(t0['ids'])
    assert m >= 2 and t0['keypoints_smoothed'].shape == (m, K, 2) and t0['keypoints_smoothed'].dtype == np.float32
    assert t0['keypoint_last'].shape == (m, K) and t0['keypoint_last'].dtype == np.int32 and (t0['keypoint_last'] == 6).all()
    tracker.reset(1)
    after0, after1 = tracker.tracks(0), tracker.tracks(1)
    assert after1['frames'] == 0 and len(after1['ids']) == 0
    for k in t0:
        np.testing.assert_array_equal(t0[k], after0[k])
    stream_bytes = tracker.smooth_stream_bytes
    assert not tracker.smooth_prev[stream_bytes:].cpu().numpy().any() and not tracker.smooth_next[stream_bytes:].cpu().numpy().any()
    got = tracker.update([seqs[0][6], seqs[1][6]])
    assert got[0]['keypoint_velocities'].any() and not got[1]['keypoint_velocities'].any()      # stream 1 starts again
    assert tracker.tracks(0)['frames'] == 7 and tracker.tracks(1)['frames'] == 1
    tracker.reset()
    assert not tracker.smooth_prev.cpu().numpy().any() and not tracker.smooth_next.cpu().numpy().any()
    with pytest.raises(ValueError, match="smooth="):
        plain.launch_smooth(None, None, None, 2)
