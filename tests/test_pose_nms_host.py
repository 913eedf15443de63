"""CPU: the plain-loop reference of mpn_pose_nms against an independent numpy formulation; the case table shows what it is
there for and decides nothing within 1e-9; `PoseNms`; the checks, messages and entry keys of `pose_nms=`; `RecordLayout`;
the launcher's checks without a GPU; the command lines' flags."""
import ctypes
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import pose_nms_cases as cases
import pose_nms_ref as ref
from test_detector_options_host import B, CAP, H, SERIAL, STYLE, THR, W, _detector, _key_of, _tracker

from multiposenet_amd import _lib
from multiposenet_amd.inference import OneEuro, PoseNms
from multiposenet_amd.inference.detector import RecordLayout

N = PoseNms(0.75, 0.25, 'box*keypoints')


# ------------------------------------------------------------------ the reference
def _numpy_nms(kp, scores, thr):
    """Greedy NMS the usual vectorised way: every joint counts."""
    order = np.argsort(-scores, kind='stable')
    x, y = kp[:, :, 0], kp[:, :, 1]
    area = (x.max(1).astype(np.float64) - x.min(1)) * (y.max(1).astype(np.float64) - y.min(1))
    variances = (np.array(ref.SIGMAS) / 10.0 * 2) ** 2
    keep = []
    while order.size:
        head, rest = order[0], order[1:]
        keep.append(int(head))
        d2 = ((kp[rest, :, :2].astype(np.float64) - kp[head, :, :2].astype(np.float64)) ** 2).sum(-1)
        denom = (area[head] + area[rest]) / 2 + np.spacing(1)
        sim = np.exp(-d2 / variances / denom[:, None] / 2).mean(1)
        order = rest[sim <= thr]
    return sorted(keep)


@pytest.mark.parametrize("seed", range(6))
def test_reference_equals_the_vectorised_formulation(seed):
    """Random crowds: poses of random size around a few centres, so that some suppress each other and some do not."""
    rs = np.random.RandomState(seed)
    n, thr = 40, (0.3, 0.5, 0.7)[seed % 3]
    centres = rs.uniform(0, 400, (5, 2))
    kp = np.zeros((n, 17, 3), np.float32)
    for p in range(n):
        kp[p, :, :2] = cases._POSE * rs.uniform(0.5, 1.5) + centres[rs.randint(5)] + rs.uniform(-12, 12, (1, 2)) + rs.uniform(-3, 3, (17, 2))
    kp[:, :, 2] = rs.uniform(0.1, 1.0, (n, 17))
    scores = rs.permutation(n).astype(np.float32) / n
    log = []
    kept, absorbed, sim = ref.survivors(kp, scores, kp[:, :, 2], thr, -1.0, 0, log)
    assert ref.undecided(log) == []
    assert kept == _numpy_nms(kp, scores, np.float64(np.float32(thr)))
    assert 3 < len(kept) < n and sum(absorbed) == n - len(kept) and all(absorbed[p] == 0 for p in range(n) if p not in kept)
    assert all(sim[p][q] == sim[q][p] and 0 <= sim[p][q] <= 1 for p in range(n) for q in range(n))


def _unpack(out, info, b=cases.B, mb=cases.MAX_BOXES):
    """(counts [b], per image the kept sources and what each absorbed, suppressed [b])."""
    header = out[:ref.header_words(b) * 4].view(np.int32)
    counts = header[1:1 + b]
    head = ref.info_head_bytes(b)
    rows = info[head:head + 8 * b * mb].view(np.int32).reshape(-1, 2)
    at = np.cumsum(counts) - counts
    assert header[0] == counts.sum() and not rows[header[0]:].any()
    return counts, [rows[a:a + c].tolist() for a, c in zip(at, counts)], info[:4 * b].view(np.int32)


@pytest.mark.parametrize("score_mode", [0, 1])
@pytest.mark.parametrize("mks", cases.MIN_KEYPOINT_SCORES)
def test_case_table_shows_what_it_is_there_for(score_mode, mks):
    imgs = cases.images()
    record = cases.table(overflow=5)
    log = []
    out, info, sim = ref.run(record, cases.B, cases.MAX_BOXES, cases.THRESHOLD, mks, score_mode, log)
    assert ref.undecided(log) == [] and len(log) > 2016
    header = out[:ref.header_words(cases.B) * 4].view(np.int32)
    counts, kept, suppressed = _unpack(out, info)
    n_in = np.array([len(im) for im in imgs])
    assert header[1 + cases.B:1 + 2 * cases.B].tolist() == (n_in + 1 + np.arange(cases.B)).tolist() and header[1 + 2 * cases.B] == 5
    assert (suppressed == n_in - counts).all()
    assert kept[0] == [] and kept[1] == [[0, 0]]
    assert kept[2] == [[40, 63]]
    a, b, c = 0, 1, 2
    assert kept[3] == [[a, 1], [c, 0]] and sim[3, b, c] > cases.THRESHOLD > sim[3, a, c] and sim[3, a, b] > cases.THRESHOLD
    assert kept[4] == [[p, 0] for p in range(64)] and np.count_nonzero(sim[4]) == 64 * 63      # every pair computed, none exactly 0
    kp5 = [kp for kp, _ in imgs[5]]
    m = [int(np.count_nonzero((kp5[p][:, 2] >= np.float32(mks)) & (kp5[p + 1][:, 2] >= np.float32(mks)))) for p in (0, 2, 4)]
    if mks == 0.5:
        assert m == [0, 1, 17] and kept[5] == [[0, 0], [1, 0], [2, 1], [4, 1]] and sim[5, 0, 1] == 0.0
    else:
        assert m == [17, 17, 17] and kept[5] == [[0, 1], [2, 1], [4, 1]]
    assert kept[6] == ([[0, 1], [2, 0]] if score_mode == 0 else [[1, 1], [2, 0]])
    assert kept[7] == [[0, 2], [1, 0]]
    rows = record[ref.header_words(cases.B) * 4:].reshape(-1, ref.ROW_WORDS * 4)
    first7 = int(n_in[:7].sum())
    assert rows[first7].tobytes() == rows[first7 + 2].tobytes() == rows[first7 + 3].tobytes() != rows[first7 + 1].tobytes()
    # the kept rows are byte copies, dense; the rest is zero
    out_rows = out[ref.header_words(cases.B) * 4:].reshape(-1, ref.ROW_WORDS * 4)
    src = [int(n_in[:i].sum()) + p for i in range(cases.B) for p, _ in kept[i]]
    assert np.array_equal(out_rows[:len(src)], rows[src]) and not out_rows[len(src):].any()
    # the order scores of mode 1 are distinct, the identical rows of image 7 apart
    for i, im in enumerate(imgs):
        s = [float(ref.order_score(score, kp[:, 2], 1)) for kp, score in im]
        assert len(set(s)) == len(s) - (2 if i == 7 else 0), i


def test_large_and_nan_cases_decide_nothing_closely():
    log = []
    out, info, _ = ref.run(cases.large(), 64, 64, cases.THRESHOLD, 0.5, 1, log)
    counts, kept, _ = _unpack(out, info, 64, 64)
    assert ref.undecided(log) == [] and counts.tolist() == [0, 1, 1, 2, 64, 4, 2, 2] * 8 and counts.sum() > 512
    log = []
    out, info, _ = ref.run(cases.pack(cases.nan_scores(), 2, 4), 2, 4, cases.THRESHOLD, 0.0, 0, log)
    assert ref.undecided(log) == [] and _unpack(out, info, 2, 4)[1] == [[[0, 0], [1, 0], [2, 0], [3, 0]], [[1, 1]]]
    assert ref.visited_before(0.1, 5, float('nan'), 0) and not ref.visited_before(float('nan'), 0, 0.1, 5)
    assert ref.visited_before(float('nan'), 1, float('nan'), 2) and not ref.visited_before(float('nan'), 2, float('nan'), 1)
    # a threshold of 1: nothing is logged as undecided although identical rows sit exactly on it
    log = []
    out, _, _ = ref.run(cases.table(), cases.B, cases.MAX_BOXES, 1.0, 0.0, 0, log)
    assert any(s == 1.0 for s, _ in log) and ref.undecided(log) == [] and out.tobytes() == cases.table().tobytes()


# ------------------------------------------------------------------ PoseNms
def test_pose_nms_parameters():
    defaults = dict(threshold=float(np.float32(0.9)), min_keypoint_score=0.0, score='box')
    p = PoseNms()
    assert repr(p) == "PoseNms(threshold=0.8999999761581421, min_keypoint_score=0.0, score='box')"
    assert p.astuple() == tuple(defaults.values()) and list(PoseNms.__slots__) == list(defaults)
    assert not hasattr(p, '__dict__')
    assert p == PoseNms(**defaults) and hash(p) == hash(PoseNms(**defaults)) and p != PoseNms(threshold=0.25) and p != p.astuple()
    assert p != PoseNms(score='box*keypoints') and p != OneEuro()
    assert len({p, PoseNms(), PoseNms(threshold=0.25), PoseNms(score='box*keypoints')}) == 3
    assert PoseNms(threshold=0.1).astuple()[0] == float(np.float32(0.1))           # rounded to what the launch receives
    for change in (lambda: setattr(p, 'threshold', 1.0), lambda: setattr(p, 'score', 'box'), lambda: setattr(p, 'other', 1.0),
                   lambda: delattr(p, 'threshold')):
        with pytest.raises(AttributeError, match="^PoseNms is immutable$"):
            change()
    for name in ('threshold', 'min_keypoint_score'):
        with pytest.raises(ValueError, match=f"^PoseNms: {name} must be a number \\(got 'fast'\\)$"):
            PoseNms(**{name: 'fast'})
        for bad in (float('nan'), float('inf'), 1e39):
            with pytest.raises(ValueError, match="^" + re.escape(f"PoseNms: {name} must be finite (got {bad!r})") + "$"):
                PoseNms(**{name: bad})
    for bad in (-0.25, 1.5):
        with pytest.raises(ValueError, match=f"^PoseNms: threshold must be in 0..1 \\(got {bad!r}\\)$"):
            PoseNms(threshold=bad)
    assert PoseNms(threshold=0).threshold == 0.0 and PoseNms(threshold=1).threshold == 1.0
    assert PoseNms(min_keypoint_score=-3).min_keypoint_score == -3.0
    for bad in ('keypoints', None, 1, ['box']):
        with pytest.raises(ValueError, match="^PoseNms: score must be one of \\['box', 'box\\*keypoints'\\]"):
            PoseNms(score=bad)
    assert "NOT tuned" in PoseNms.__doc__


# ------------------------------------------------------------------ pose_nms= of the Detector
def test_entry_keys_end_in_the_pose_nms():
    gt, trk = [{}] * B, _tracker(smooth=OneEuro())
    table = [
        (dict(pose_nms=N), ('pose_nms', N)),
        (dict(pose_nms=None), ()),
        (dict(annotate='jpeg', jpeg_subsampling='4:2:2', plot_maps=True, groundtruth=gt, flip=True, scales=[(256, 256)], track=trk,
              track_style=STYLE, return_heatmaps=False, pose_nms=N),
         ('annotate', 'jpeg', '4:2:2', 'maps', 'oks', 'box', 20, 'tta', True, ((256, 256),), 'track', SERIAL, B, 'style', STYLE,
          'pose_nms', N)),
    ]
    batch = np.zeros((B, H, W, 3), np.uint8)
    frames = [np.zeros((50, 70, 3), np.uint8), np.zeros((64, 33, 3), np.uint8)]
    for use_graph in (True, False):
        det = _detector(use_graph)
        for options, tail in table:
            key = _key_of(det.predict_batch, batch, score_threshold=THR, **options)
            assert key == ((B, H, W, THR) if use_graph else ('eager', B, H, W)) + tail, options
            key = _key_of(det.predict_images, frames, size=(H, W), score_threshold=THR, **options)
            assert key == ('images', B, H, W, THR, CAP) + tail, options
    # an equal PoseNms finds the same entry; another one does not
    det = _detector(True)
    key = _key_of(det.predict_batch, batch, score_threshold=THR, pose_nms=PoseNms(0.75, 0.25, 'box*keypoints'))
    assert key == (B, H, W, THR, 'pose_nms', N) and hash(key) == hash((B, H, W, THR, 'pose_nms', N))
    assert _key_of(det.predict_batch, batch, score_threshold=THR, pose_nms=PoseNms(0.5)) != key
    given = dict(score_threshold=THR, return_heatmaps=True, annotate=False, jpeg_quality=75, jpeg_subsampling='4:2:0',
                 plot_maps=False, groundtruth=None, flip=False, scales=None, track=None, track_style=None)
    assert det._options(lambda: (B, H, W), **given)[0].pose_nms is None                       # the key may be absent
    opts = det._options(lambda: (B, H, W), pose_nms=N, **given)[0]
    assert opts.pose_nms is N and opts.tail(B) == ('pose_nms', N) and opts._fields[-1] == 'pose_nms'


def test_pose_nms_is_checked_last_and_says_what_is_missing():
    det = _detector(True)
    batch, frames = np.zeros((B, H, W, 3), np.uint8), [np.zeros((50, 70, 3), np.uint8)] * B
    for method, first in ((det.predict_batch, batch), (det.predict_images, frames)):
        with pytest.raises(ValueError, match="flip must be"):
            method(first, flip=1, pose_nms='x')
        with pytest.raises(ValueError, match="scale must be"):
            method(first, scales=[(100, 100)], pose_nms='x')
        for bad in ('x', 0.9, True, OneEuro()):
            with pytest.raises(ValueError, match="^pose_nms must be None or an inference.PoseNms$"):
                method(first, pose_nms=bad)
    with pytest.raises(ValueError, match="^pose_nms must be None or an inference.PoseNms$"):
        det._options(lambda: (B, H, W), score_threshold=THR, return_heatmaps=True, annotate=False, jpeg_quality=75,
                     jpeg_subsampling='4:2:0', plot_maps=False, groundtruth=None, flip=False, scales=None, track=None,
                     track_style=None, pose_nms='x')
    det.retinanet = None
    with pytest.raises(ValueError, match="pose_nms= needs the person detector \\(detector_path\\)"):
        det.predict_batch(batch, pose_nms=N)
    det.retinanet, det.assigner = object(), None
    with pytest.raises(ValueError, match="pose_nms= compares keypoints, which need the PRN \\(prn_path\\)"):
        det.predict_batch(batch, pose_nms=N)
    det.assigner = object()
    det.params = {'max_boxes': 65}
    with pytest.raises(ValueError, match="max_boxes must be in 1..64 \\(got 65\\)"):
        det.predict_batch(batch, pose_nms=N)
    det.params = {'max_boxes': 64}
    assert _key_of(det.predict_batch, batch, score_threshold=THR, pose_nms=N)[-2:] == ('pose_nms', N)


def test_record_layout_has_four_slices():
    lib = _lib.lib()
    for b, mb in ((1, 25), (4, 25), (6, 64)):
        record = lib.mpn_pose_gather_record_bytes(b, mb)
        oks = types.SimpleNamespace(out_bytes=lib.mpn_oks_match_out_bytes(b, mb))
        nms = types.SimpleNamespace(info_bytes=lib.mpn_pose_nms_info_bytes(b, mb))
        trk = _tracker(smooth=OneEuro(), max_boxes=mb)
        base = lambda layout: (layout.record, layout.oks, layout.track, layout.nms)     # noqa: E731
        assert base(RecordLayout(b, mb)) == (slice(0, record), slice(record, record), slice(record, record), slice(record, record))
        assert base(RecordLayout(b, mb, oks, trk))[:3] == base(RecordLayout(b, mb, oks, trk, None))[:3]
        end = record + oks.out_bytes + trk.out_bytes(b)
        at = (end + 15) // 16 * 16
        assert trk.out_bytes(b) % 8 == 4 * (b * mb % 2)             # 364 bytes a slot: the info block needs its own alignment
        assert base(RecordLayout(b, mb, oks, trk, nms)) == (slice(0, record), slice(record, record + oks.out_bytes),
                                                            slice(record + oks.out_bytes, end), slice(at, at + nms.info_bytes))
        assert RecordLayout(b, mb, oks, trk, nms).nbytes == at + nms.info_bytes
        assert RecordLayout(b, mb, nms=nms).nms == slice(record, record + nms.info_bytes) and record % 16 == 0
        assert nms.info_bytes == (4 * b + 15) // 16 * 16 + 16 * b * mb == ref.info_bytes(b, mb)
        assert record == ref.record_bytes(b, mb)


# ------------------------------------------------------------------ the launcher, without a GPU
def test_launcher_checks_need_no_gpu():
    lib = _lib.lib()
    for name in ("mpn_pose_nms_info_bytes", "mpn_pose_nms"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["mpn_pose_nms"][1]) == 12
    for b, mb in ((0, 64), (1, 0), (1, 65), (-1, 8), (65, 64), (4097, 1), (1 << 30, 1 << 30)):
        assert lib.mpn_pose_nms_info_bytes(b, mb) == 0, (b, mb)
    assert lib.mpn_pose_nms_info_bytes(4096, 1) == 4096 * 4 + 4096 * 16 and lib.mpn_pose_nms_info_bytes(64, 64) == 256 + 65536
    b, mb = 8, 64
    need, info_need = lib.mpn_pose_gather_record_bytes(b, mb), lib.mpn_pose_nms_info_bytes(b, mb)
    IN, OUT, INFO, SIM = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20))

    def call(record_in=IN, b=b, mb=mb, thr=0.5, mks=0.0, mode=0, record_out=OUT, record_bytes=need, info=INFO,
             info_bytes=info_need, sim=SIM):
        _lib.call("mpn_pose_nms", record_in, b, mb, thr, mks, mode, record_out, record_bytes, info, info_bytes, sim, None)
    for null in ('record_in', 'record_out', 'info'):
        with pytest.raises(ValueError, match="BAD_ARG.*null pointer"):
            call(**{null: None})
    for mode in (2, -1):
        with pytest.raises(ValueError, match="BAD_ARG.*score_mode must be 0 or 1"):
            call(mode=mode)
    for nan in ('thr', 'mks'):
        with pytest.raises(ValueError, match="BAD_ARG.*NaN"):
            call(**{nan: float('nan')})
    for shape in (dict(mb=65), dict(b=4097, mb=1), dict(b=0), dict(mb=0), dict(b=65, mb=64)):
        with pytest.raises(ValueError, match="BAD_SHAPE"):
            call(**shape)
    for out in (IN, ctypes.c_void_p(IN.value + need - 16), ctypes.c_void_p(IN.value - need + 16)):
        with pytest.raises(ValueError, match="BAD_ARG.*must not overlap"):
            call(record_out=out)
    for misaligned in (dict(record_in=ctypes.c_void_p(IN.value + 8)), dict(record_out=ctypes.c_void_p(OUT.value + 4)),
                       dict(info=ctypes.c_void_p(INFO.value + 4)), dict(sim=ctypes.c_void_p(SIM.value + 4))):
        with pytest.raises(ValueError, match="BAD_ALIGN"):
            call(**misaligned)
    with pytest.raises(_lib.MpnError, match="WORKSPACE.*record_out"):
        call(record_bytes=need - 1)
    with pytest.raises(_lib.MpnError, match="WORKSPACE.*info"):
        call(info_bytes=info_need - 1)
    # the order: an argument error before a shape error before an alignment error before a size error
    with pytest.raises(ValueError, match="BAD_ARG"):
        call(mode=2, mb=65, info=ctypes.c_void_p(INFO.value + 4), record_bytes=0)
    with pytest.raises(ValueError, match="BAD_SHAPE"):
        call(mb=65, info=ctypes.c_void_p(INFO.value + 4), record_bytes=0)
    with pytest.raises(ValueError, match="BAD_ALIGN"):
        call(info=ctypes.c_void_p(INFO.value + 4), record_bytes=0)


# ------------------------------------------------------------------ command lines
@pytest.mark.parametrize("module, required", [("evaluate_pose", []), ("track_frames", ["--images", "nowhere"])])
def test_command_lines_take_the_flags(module, required):
    run = lambda *a: subprocess.run([sys.executable, "-m", f"multiposenet_amd.{module}", *a], capture_output=True, text=True)
    r = run("--help")
    assert r.returncode == 0
    for flag in ("--pose-nms [THRESHOLD]", "--pose-nms-min-keypoint-score X", "--pose-nms-score {box,box*keypoints}"):
        assert flag in r.stdout, flag
    r = run(*required, "--pose-nms", "1.5")
    assert r.returncode == 2 and "PoseNms: threshold must be in 0..1 (got 1.5)" in r.stderr
    r = run(*required, "--pose-nms", "--pose-nms-score", "keypoints")
    assert r.returncode == 2 and "--pose-nms-score" in r.stderr


def test_flags_make_the_pose_nms():
    import argparse
    from multiposenet_amd import pose_nms
    ap = argparse.ArgumentParser()
    pose_nms.add_arguments(ap)
    assert pose_nms.from_arguments(ap, ap.parse_args([])) is None
    assert pose_nms.from_arguments(ap, ap.parse_args(["--pose-nms"])) == PoseNms()
    assert pose_nms.from_arguments(ap, ap.parse_args(["--pose-nms", "0.75", "--pose-nms-min-keypoint-score", "0.25",
                                                      "--pose-nms-score", "box*keypoints"])) == N
    assert pose_nms.from_arguments(ap, ap.parse_args(["--pose-nms", "0"])) == PoseNms(0.0)
