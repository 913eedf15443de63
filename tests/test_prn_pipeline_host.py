"""CPU: the host side of the PRN input pipeline - jpeg_shape, record order, curriculum filter, annotation cache, the
restatement's invariants, the argument checks of mpn_prn_examples and the stage arithmetic of train_prn."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prn_pipeline_cases as cases  # noqa: E402
import prn_pipeline_ref as ref  # noqa: E402

from multiposenet_amd import _lib  # noqa: E402
from multiposenet_amd.detector.input_pipeline import prn_pipeline as pp  # noqa: E402
from multiposenet_amd.detector.input_pipeline import tfrecord as tfr  # noqa: E402
from multiposenet_amd.detector.input_pipeline import AnnotationCache, PoseResidualNetworkPipeline  # noqa: E402


# ---------------------------------------------------------------- jpeg_shape
def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def _jpeg(sof, height, width, before=()):
    frame = struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    body = b"".join(before) + _segment(sof, frame) + _segment(0xDA, bytes(10)) + bytes(20) + b"\xff\xd9"
    return b"\xff\xd8" + body


def test_jpeg_shape_handmade_headers():
    app0 = _segment(0xE0, b"JFIF\0" + bytes(9))
    dqt = _segment(0xDB, bytes(65))
    dht = _segment(0xC4, bytes([0xC0, 0xC2] * 15))      # a Huffman table whose bytes look like frame markers
    assert tfr.jpeg_shape(_jpeg(0xC0, 97, 131, [app0, dqt, dht])) == (97, 131)          # baseline
    assert tfr.jpeg_shape(_jpeg(0xC2, 480, 640, [app0, dqt, dqt, dht])) == (480, 640)   # progressive
    assert tfr.jpeg_shape(_jpeg(0xC1, 1, 65535, [b"\xff", dht, _segment(0xCC, bytes(4)), _segment(0xC8, bytes(8))])) == (1, 65535)
    assert tfr.jpeg_shape(memoryview(_jpeg(0xCF, 300, 200))) == (300, 200)


def test_jpeg_shape_rejects_streams_without_a_frame():
    for bad in (b"", b"garbage that is no image", b"\xff\xd8" + bytes(40), b"\xff\xd8\xff\xd9",
                b"\xff\xd8" + _segment(0xC4, bytes(30)) + _segment(0xDA, bytes(8)),
                b"\xff\xd8" + _segment(0xE0, bytes(14)) + b"\xff\xc0\x00\x11\x08"):
        with pytest.raises(ValueError):
            tfr.jpeg_shape(bad)


def test_jpeg_shape_of_encoded_images():
    Image = pytest.importorskip("PIL.Image")
    import io
    for (h, w), kw in (((37, 53), {}), ((203, 157), {"progressive": True}), ((64, 48), {"optimize": True})):
        buf = io.BytesIO()
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(buf, format="JPEG", **kw)
        assert tfr.jpeg_shape(buf.getvalue()) == (h, w)


# ---------------------------------------------------------------- toy shards
def _record(rng, height, width, persons, boxes=None):
    if boxes is None:
        y0, x0 = rng.uniform(0, height / 2, persons), rng.uniform(0, width / 2, persons)
        boxes = np.stack([y0, x0, y0 + rng.uniform(20, height / 2, persons), x0 + rng.uniform(20, width / 2, persons)], 1)
    boxes = np.asarray(boxes, np.float32).reshape(persons, 4)
    kp = np.stack([rng.integers(0, height, (persons, 17)), rng.integers(0, width, (persons, 17)),
                   rng.integers(0, 3, (persons, 17))], 2).astype(np.int64)
    return {"image": _jpeg(0xC0, height, width), "num_persons": np.array([persons], np.int64), "boxes": boxes.reshape(-1),
            "keypoints": kp.reshape(-1), "masks": b"\0"}


def _shards(tmp_path, rng):
    """Two files; records with 0 persons, with a degenerate box and with ordinary people. Returns (paths, records)."""
    recs = [[_record(rng, 97, 131, 2), _record(rng, 200, 300, 0), _record(rng, 203, 157, 3)],
            [_record(rng, 120, 90, 2, boxes=[[10, 10, 10, 60], [5, 6, 80, 70]]), _record(rng, 480, 640, 4),
             _record(rng, 64, 64, 1, boxes=[[30, 40, 20, 50]])]]
    paths = []
    for i, rs in enumerate(recs):
        paths.append(str(tmp_path / f"shard-{i}.tfrecords"))
        with open(paths[-1], "wb") as f:
            for r in rs:
                f.write(tfr.frame_record(tfr.encode_example(r)))
    return paths, recs


def _expected(paths, recs, max_keypoints=None):
    """[(source, person index in the record)] of the kept persons in record order."""
    out = []
    for path, rs in zip(paths, recs):
        for k, r in enumerate(rs):
            p = int(r["num_persons"][0])
            bx, kp = r["boxes"].reshape(p, 4), r["keypoints"].reshape(p, 17, 3)
            for j in ref.filter_persons(kp, bx, max_keypoints) if p else []:
                if bx[j, 2] > bx[j, 0] and bx[j, 3] > bx[j, 1]:
                    out.append(((path, k), int(j)))
    return out


def _ids(tables):
    fp = tables["first_person"]
    return [(tables["sources"][e["image"]], int(tables["persons"][e["image"]][e["person"] - fp[e["image"]]]), int(e["flip"]))
            for e in tables["examples"]]


def test_evaluation_pass_order_partial_batch_and_skips(tmp_path):
    rng = np.random.default_rng(0)
    paths, recs = _shards(tmp_path, rng)
    want = _expected(paths, recs)
    assert len(want) == 2 + 3 + 1 + 4                   # empty record, degenerate boxes skipped
    batches = list(PoseResidualNetworkPipeline(paths, False, 4).samples())
    assert [len(t["examples"]) for t in batches] == [4, 4, len(want) % 4]
    got = [i for t in batches for i in _ids(t)]
    assert [(s, k) for s, k, _ in got] == want
    assert not any(f for _, _, f in got)                # no flip in evaluation
    for t in batches:                                   # the tables are consistent
        assert t["keypoints"].dtype == np.int32 and t["boxes"].dtype == np.float32
        assert t["first_person"][-1] == len(t["boxes"]) == len(t["keypoints"])
        for e in t["examples"]:
            assert t["first_person"][e["image"]] <= e["person"] < t["first_person"][e["image"] + 1]
    t = batches[0]                                      # sizes come from the JPEG header
    assert (int(t["height"][0]), int(t["width"][0])) == (97, 131)


def test_max_keypoints_keeps_the_right_persons_and_their_images_people(tmp_path):
    rng = np.random.default_rng(1)
    paths, recs = _shards(tmp_path, rng)
    counts = sorted({int((r["keypoints"].reshape(-1, 17, 3)[:, :, 2] > 0).sum(1)[j]) for rs in recs for r in rs
                     for j in range(int(r["num_persons"][0]))})
    mk = counts[len(counts) // 2]
    want = _expected(paths, recs, mk)
    assert 0 < len(want) < len(_expected(paths, recs))
    batches = list(PoseResidualNetworkPipeline(paths, False, 3, max_keypoints=mk).samples())
    assert [(s, k) for t in batches for s, k, _ in _ids(t)] == want
    by_path = dict(zip(paths, recs))
    for t in batches:
        assert ((t["keypoints"][:, :, 2] > 0).sum(1) <= mk).all()       # only kept people are passed on (heatmap inputs)
        for r, (path, k) in enumerate(t["sources"]):
            rec = by_path[path][k]
            a, b = t["first_person"][r], t["first_person"][r + 1]
            np.testing.assert_array_equal(t["keypoints"][a:b], rec["keypoints"].reshape(-1, 17, 3)[t["persons"][r]])
            np.testing.assert_array_equal(t["boxes"][a:b], rec["boxes"].reshape(-1, 4)[t["persons"][r]])
    with pytest.raises(ValueError, match="no person is left"):
        next(PoseResidualNetworkPipeline(paths, True, 2, max_keypoints=-1, shuffle_buffer_size=2).samples())


def test_seed_fixes_the_training_sequence(tmp_path):
    rng = np.random.default_rng(2)
    paths, recs = _shards(tmp_path, rng)

    def seq(seed):
        it = PoseResidualNetworkPipeline(paths, True, 4, seed=seed, shuffle_buffer_size=5).samples()
        return [i for _ in range(12) for i in _ids(next(it))]
    a, b, c = seq(3), seq(3), seq(4)
    assert a == b and a != c
    assert {(s, k) for s, k, _ in a} == set(_expected(paths, recs))      # every person turns up
    flips = [f for _, _, f in a]
    assert 0 < sum(flips) < len(flips)


def test_second_epoch_and_second_pipeline_open_no_file(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    paths, recs = _shards(tmp_path, rng)
    opened = []
    real = pp.read_records
    monkeypatch.setattr(pp, "read_records", lambda path, *a, **k: (opened.append(path), real(path, *a, **k))[1])
    cache = AnnotationCache()
    it = PoseResidualNetworkPipeline(paths, True, 5, annotations=cache, shuffle_buffer_size=3).samples()
    for _ in range(10):                                  # 50 persons: five epochs of the 10 kept ones
        next(it)
    assert sorted(opened) == sorted(paths)
    other = PoseResidualNetworkPipeline(paths, True, 5, max_keypoints=17, annotations=cache, shuffle_buffer_size=3).samples()
    next(other)
    assert list(PoseResidualNetworkPipeline(paths, False, 4, annotations=cache).samples())
    assert sorted(opened) == sorted(paths)
    assert cache.num_persons == 12 and 0 < cache.nbytes < 12 * 260
    list(PoseResidualNetworkPipeline(paths, False, 4).samples())          # without the shared cache the files are read again
    assert len(opened) == 2 * len(paths)


def test_in_memory_examples_with_image_or_size():
    rng = np.random.default_rng(4)
    kp = np.stack([rng.integers(0, 90, (2, 17)), rng.integers(0, 120, (2, 17)), rng.integers(0, 3, (2, 17))], 2)
    bx = np.array([[5, 6, 80, 70], [10, 20, 60, 110]], np.float32)
    exs = [{"image": np.zeros((97, 131, 3), np.uint8), "boxes": bx, "keypoints": kp},
           {"height": 203, "width": 157, "boxes": bx[:1], "keypoints": kp[:1]}]
    (t,) = list(PoseResidualNetworkPipeline(exs, False, 8).samples())
    assert t["height"].tolist() == [97, 203] and t["width"].tolist() == [131, 157]
    assert len(t["examples"]) == 3 and t["sources"] == [(0, 0), (1, 0)]


# ---------------------------------------------------------------- the restatement
def test_restatement_invariants():
    t = cases.handmade_tables()
    crops, labels = ref.batch(t)
    cases.check_handmade(t, crops, labels)
    for n, e in enumerate(t["examples"]):
        assert labels[n].sum() == (t["keypoints"][e["person"], :, 2] > 0).sum()
    un = dict(t, examples=t["examples"].copy())
    un["examples"]["flip"] = 0
    c0, l0 = ref.batch(un)
    for n, e in enumerate(t["examples"]):
        if e["flip"]:
            np.testing.assert_array_equal(crops[n], c0[n][:, ::-1][:, :, ref.FLIP_ORDER])
            np.testing.assert_array_equal(labels[n], l0[n][:, ::-1][:, :, ref.FLIP_ORDER])
        else:
            np.testing.assert_array_equal(crops[n], c0[n])
    assert crops.max() <= 1.0 and crops.min() >= 0.0
    r = cases.random_tables(5)
    cases.check_batch(r, *ref.batch(r))


def test_label_rounds_half_to_even_and_clips():
    kp = np.zeros((17, 3), np.int64)
    kp[0] = (5, 5, 1)        # (5 - 0) * 56/112 = 2.5 -> 2 ; (5 - 0) * 36/72 = 2.5 -> 2
    kp[1] = (7, 7, 2)        # 3.5 -> 4
    kp[2] = (500, -40, 1)    # clipped to (55, 0)
    lab = ref.label_map(kp, np.array([0, 0, 112, 72], np.float32))
    assert lab.sum() == 3 and lab[2, 2, 0] == 1 and lab[4, 4, 1] == 1 and lab[55, 0, 2] == 1


# ---------------------------------------------------------------- mpn_prn_examples: argument checks need no device
def test_prn_examples_argument_checks_need_no_gpu():
    P, Q = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    ws = _lib.lib().mpn_prn_examples_workspace_bytes(3)
    assert ws >= 3 * (14 * 8 + 17 * 8 + 4) and _lib.lib().mpn_prn_examples_workspace_bytes(0) > 0
    assert _lib.lib().mpn_prn_example_desc_bytes() == pp.DESC_DTYPE.itemsize == 16

    def call(kp=P, bx=P, q=3, fp=P, w=P, h=P, r=1, ex=P, n=2, ch=56, cw=36, ds=4, crops=P, labels=P, wsp=P, wsb=ws):
        _lib.call("mpn_prn_examples", kp, bx, q, fp, w, h, r, ex, n, ch, cw, ds, crops, labels, wsp, wsb, None)
    with pytest.raises(ValueError, match="N must be >= 0"):
        call(n=-1)
    for kw in ({"ch": 0}, {"cw": 0}, {"ch": -56}):
        with pytest.raises(ValueError, match="crop size must be positive"):
            call(**kw)
    for name in ("kp", "bx", "fp", "w", "h", "ex", "crops", "labels", "wsp"):
        with pytest.raises(ValueError, match="null pointer"):
            call(**{name: None})
    for name in ("crops", "labels"):
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(**{name: Q})
    with pytest.raises(_lib.MpnError, match="workspace too small"):
        call(wsb=ws - 1)
    call(n=0)                                            # MPN_OK, nothing launched
    call(n=0, kp=None, bx=None, fp=None, w=None, h=None, ex=None, crops=None, labels=None, wsp=None, wsb=0)


# ---------------------------------------------------------------- train_prn
def test_stage_for_step_boundaries():
    from multiposenet_amd.train_prn import NUM_STEPS_PER_KEYPOINT, stage_for_step
    assert NUM_STEPS_PER_KEYPOINT == 10000
    for i in range(14):
        assert stage_for_step(i * 10000) == 4 + i
        assert stage_for_step(i * 10000 + 9999) == 4 + i
    assert stage_for_step(0) == 4 and stage_for_step(139999) == 17
    assert stage_for_step(140000) is None and stage_for_step(199999) is None and stage_for_step(10 ** 9) is None
    assert [stage_for_step(s, 2) for s in range(0, 30)] == [4 + s // 2 for s in range(28)] + [None, None]
    with pytest.raises(ValueError):
        stage_for_step(-1)


def test_train_prn_main_points_at_the_toy_records(tmp_path):
    from multiposenet_amd import train_prn
    with pytest.raises(SystemExit, match="make_toy_tfrecords"):
        train_prn.main(["--train-dataset", str(tmp_path), "--val-dataset", str(tmp_path), "--model-dir", str(tmp_path / "m")])
