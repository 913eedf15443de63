"""The definition of mpn_pose_smooth (include/mpn.h) as plain loops in numpy float32: one operation per line in the documented
order, every result wrapped in np.float32. Test infrastructure only; the kernel, `tracking.PoseTracker(smooth=...)` and the
Detector's `track=` are compared with it, byte for byte.

    state = new_state(streams, max_tracks)
    (keypoints, velocities), state = launch(record_keypoints, counts, track_rows, state, params)   # keyed by slot, as the kernel
    pack_state(state)                                # the bytes mpn_pose_smooth leaves in `next`
    pack_rows(keypoints, velocities, B, max_boxes)   # the bytes it leaves in `out`

    ids = new_id_state(streams)
    rows = run(outputs, ids, params)                 # predict_*-style dicts with 'keypoints' and 'track_ids', keyed by (stream, id)

The two are equivalent because a track never changes its slot and an id is never given twice: a slot whose id changes is a
new key. `trace=[]` collects every float32 intermediate of the filtered samples (tests assert that none is subnormal)."""
import collections
import copy

import numpy as np

K = 17
F32 = np.float32
TWO_PI = F32(6.2831855)
ROW_BYTES = 4 * 5 * K                   # keypoints[17][3], velocities[17][2]

_Params = collections.namedtuple('Params', 'rate min_cutoff beta d_cutoff min_keypoint_score')


def Params(rate=30.0, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, min_keypoint_score=0.0):
    """The launch's five float arguments, as the float32 values the kernel receives."""
    return _Params(F32(rate), F32(min_cutoff), F32(beta), F32(d_cutoff), F32(min_keypoint_score))


class Stream:
    def __init__(self, max_tracks):
        self.frames = 0
        self.id = np.zeros(max_tracks, np.int32)
        self.last = np.zeros((max_tracks, K), np.int32)
        self.hat = np.zeros((max_tracks, K, 4), np.float32)         # x_hat, y_hat, dx_hat, dy_hat


def new_state(streams, max_tracks):
    return [Stream(max_tracks) for _ in range(streams)]


def pack_state(state):
    out = []
    for st in state:
        out.append(np.array([st.frames, 0, 0, 0], np.int32).tobytes())
        for t in range(len(st.id)):
            out.append(np.array([st.id[t]], np.int32).tobytes())
            for k in range(K):
                out.append(np.array([st.last[t, k]], np.int32).tobytes())
                out.append(st.hat[t, k].tobytes())
            out.append(bytes(8))
    return b''.join(out)


def pack_rows(keypoints, velocities, B, max_boxes):
    out = np.zeros((B * max_boxes, 5 * K), np.float32)
    n = len(keypoints)
    out[:n, :3 * K] = np.asarray(keypoints, np.float32).reshape(n, 3 * K)
    out[:n, 3 * K:] = np.asarray(velocities, np.float32).reshape(n, 2 * K)
    return out.tobytes()


def _alpha(fc, te, trace):
    w = F32(TWO_PI * fc)
    r = F32(w * te)
    r1 = F32(r + F32(1))
    a = F32(r / r1)
    if trace is not None:
        trace += [w, r, r1, a]
    return a


def _coordinate(x, x_hat, dx_hat, te, alpha_d, p, trace):
    e = F32(x - x_hat)
    dx = F32(e / te)
    u = F32(dx - dx_hat)
    v = F32(alpha_d * u)
    dx_hat = F32(dx_hat + v)
    speed = F32(np.abs(dx_hat))
    w = F32(p.beta * speed)
    fc = F32(p.min_cutoff + w)
    a = _alpha(fc, te, trace)
    e2 = F32(x - x_hat)
    g = F32(a * e2)
    x_hat = F32(x_hat + g)
    if trace is not None:
        trace += [e, dx, u, v, dx_hat, w, fc, g, x_hat]
    return x_hat, dx_hat


def joint(sample, last, hat, n, p, trace=None):
    """One sample (x, y, score) of one joint at frame number n -> (out (x, y, vx, vy), new last, new hat[4])."""
    x, y, score = F32(sample[0]), F32(sample[1]), F32(sample[2])
    zero = F32(0)
    if not score >= p.min_keypoint_score:                           # rejected: the filter restarts with the next good sample
        return (x, y, zero, zero), 0, hat
    if last == 0:                                                   # first
        return (x, y, zero, zero), n, np.array([x, y, zero, zero], np.float32)
    gap = int(n) - int(last)
    assert gap >= 1
    te = F32(F32(gap) / p.rate)
    alpha_d = _alpha(p.d_cutoff, te, trace)
    if trace is not None:
        trace.append(te)
    x_hat, dx_hat = _coordinate(x, F32(hat[0]), F32(hat[2]), te, alpha_d, p, trace)
    y_hat, dy_hat = _coordinate(y, F32(hat[1]), F32(hat[3]), te, alpha_d, p, trace)
    return (x_hat, y_hat, dx_hat, dy_hat), n, np.array([x_hat, y_hat, dx_hat, dy_hat], np.float32)


def launch(record_keypoints, counts, track_rows, state, p, trace=None):
    """record_keypoints f32 [total,17,3] (the record's rows in order), counts [B] rows per image, track_rows: 'track_id' and
    'slot' per row (mpn_pose_track's output rows), state: new_state(...) or what an earlier call returned (not modified).
    -> ((keypoints f32 [total,17,3], velocities f32 [total,17,2]), the new state)."""
    state = copy.deepcopy(state)
    kp_in = np.asarray(record_keypoints, np.float32).reshape(-1, K, 3)
    ids, slots = np.asarray(track_rows['track_id']), np.asarray(track_rows['slot'])
    streams, B = len(state), len(counts)
    assert B % streams == 0
    frames = B // streams
    kp, vel = kp_in.copy(), np.zeros((len(kp_in), K, 2), np.float32)
    r = 0
    for b in range(B):
        st = state[b // frames]
        T = len(st.id)
        n = st.frames + b % frames + 1
        for _ in range(int(counts[b])):
            tid, t = int(ids[r]), int(slots[r])
            if tid > 0 and 0 <= t < T:                              # else untracked: raw, velocity 0, no state touched
                if st.id[t] != tid:                                 # the slot was given to another track
                    st.id[t] = tid
                    st.last[t] = 0
                for k in range(K):
                    out, st.last[t, k], st.hat[t, k] = joint(kp_in[r, k], st.last[t, k], st.hat[t, k], n, p, trace)
                    kp[r, k, 0], kp[r, k, 1], vel[r, k, 0], vel[r, k, 1] = out
            r += 1
    for st in state:
        st.frames += frames
    assert r == len(kp_in)
    return (kp, vel), state


class IdState:
    def __init__(self, streams):
        self.frames = [0] * streams
        self.filters = {}                                           # (stream, id) -> [last int [17], hat f32 [17,4]]


def new_id_state(streams):
    return IdState(streams)


def run(outputs, state, p, trace=None):
    """b = streams * F result dicts with 'keypoints' f32 [n,17,3] and 'track_ids' [n]: stream s owns images s*F .. s*F+F-1 in
    time order. The IdState is advanced in place. -> b dicts {'keypoints_smoothed' [n,17,3], 'keypoint_velocities' [n,17,2]}."""
    streams = len(state.frames)
    assert len(outputs) % streams == 0
    frames = len(outputs) // streams
    res = []
    for i, o in enumerate(outputs):
        s = i // frames
        n = state.frames[s] + i % frames + 1
        kp_in = np.asarray(o['keypoints'], np.float32).reshape(-1, K, 3)
        kp, vel = kp_in.copy(), np.zeros((len(kp_in), K, 2), np.float32)
        for r, tid in enumerate(o['track_ids']):
            if int(tid) <= 0:
                continue
            last, hat = state.filters.setdefault((s, int(tid)), [np.zeros(K, np.int32), np.zeros((K, 4), np.float32)])
            for k in range(K):
                out, last[k], hat[k] = joint(kp_in[r, k], last[k], hat[k], n, p, trace)
                kp[r, k, 0], kp[r, k, 1], vel[r, k, 0], vel[r, k, 1] = out
        res.append({'keypoints_smoothed': kp, 'keypoint_velocities': vel})
    for s in range(streams):
        state.frames[s] += frames
    return res


def subnormal(trace):
    """The traced float32 intermediates that are subnormal (nonzero, below 2^-126 in magnitude)."""
    v = np.abs(np.array(trace, np.float32))
    return v[(v > 0) & (v < np.finfo(np.float32).tiny)]
