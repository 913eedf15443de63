"""CPU: the TFRecord / Example reader and the host-side sampling of the keypoint input pipeline."""
import math
import struct

import numpy as np
import pytest

from multiposenet_amd.detector.input_pipeline import keypoint_augment as ka
from multiposenet_amd.detector.input_pipeline import tfrecord as tfr


def _write(path, payloads):
    with open(path, "wb") as f:
        for p in payloads:
            f.write(tfr.frame_record(p))


def _example(rng, h=97, w=131, p=2, image=None):
    boxes = np.array([[10, 12, 60, 50], [30, 40, 90, 120]][:p], np.float32)
    kp = np.stack([rng.integers(0, h, (p, 17)), rng.integers(0, w, (p, 17)), rng.integers(0, 3, (p, 17))], 2)
    mh, mw = math.ceil(h / 4), math.ceil(w / 4)
    masks = np.packbits(rng.integers(0, 2, (mh, mw, 2)).astype(np.uint8))
    return {"image": image if image is not None else rng.bytes(300), "num_persons": np.array([p], np.int64),
            "boxes": boxes.reshape(-1), "keypoints": kp.astype(np.int64).reshape(-1), "masks": masks.tobytes()}


def test_crc32c_known_values():
    assert tfr.crc32c(b"") == 0
    assert tfr.crc32c(b"123456789") == 0xE3069283
    assert tfr.crc32c(bytes(32)) == 0x8A9136AA


def test_record_round_trip_without_decode(tmp_path):
    rng = np.random.default_rng(0)
    exs = [_example(rng) for _ in range(3)]
    path = str(tmp_path / "a.tfrecords")
    _write(path, [tfr.encode_example(e) for e in exs])
    recs = list(tfr.read_records(path, verify_data_crc=True))
    assert len(recs) == 3
    for rec, ex in zip(recs, exs):
        d = tfr.decode_keypoint_example(rec, decode_image=False)
        assert d["image"] == ex["image"]
        np.testing.assert_array_equal(d["boxes"].reshape(-1), ex["boxes"])
        np.testing.assert_array_equal(d["keypoints"].reshape(-1), ex["keypoints"])
        assert d["masks"].tobytes() == ex["masks"]


def test_record_round_trip_with_jpeg(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (97, 131, 3)).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")      # lossless: the decoded pixels are checked exactly
    path = str(tmp_path / "b.tfrecords")
    _write(path, [tfr.encode_example(_example(rng, image=buf.getvalue()))])
    d = tfr.decode_keypoint_example(next(tfr.read_records(path)))
    np.testing.assert_array_equal(d["image"], img)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG")
    assert tfr.decode_jpeg(buf.getvalue()).shape == (97, 131, 3)


def test_corruption_and_truncation_raise(tmp_path):
    rng = np.random.default_rng(2)
    good = tfr.encode_example(_example(rng))
    blob = bytearray(tfr.frame_record(good) * 2)
    bad_len = bytearray(blob)
    bad_len[8] ^= 1
    p = tmp_path / "len.tfrecords"
    p.write_bytes(bytes(bad_len))
    with pytest.raises(IOError, match="length"):
        list(tfr.read_records(str(p)))
    bad_data = bytearray(blob)
    bad_data[20] ^= 0xFF
    p = tmp_path / "data.tfrecords"
    p.write_bytes(bytes(bad_data))
    assert len(list(tfr.read_records(str(p)))) == 2            # unchecked by default
    with pytest.raises(IOError, match="data"):
        list(tfr.read_records(str(p), verify_data_crc=True))
    p = tmp_path / "trunc.tfrecords"
    p.write_bytes(bytes(blob[:-7]))
    with pytest.raises(IOError, match=r"trunc\.tfrecords.*offset %d" % (len(blob) // 2)):
        list(tfr.read_records(str(p)))


def _ld(num, payload):
    return tfr._enc_varint((num << 3) | 2) + tfr._enc_varint(len(payload)) + payload


def test_example_decoder_packed_unpacked_negative():
    vals = [5, -1, -(1 << 63), (1 << 63) - 1, 0]
    packed = _ld(3, _ld(1, b"".join(tfr._enc_varint(v & 0xFFFFFFFFFFFFFFFF) for v in vals)))
    unpacked = _ld(3, b"".join(tfr._enc_varint(1 << 3) + tfr._enc_varint(v & 0xFFFFFFFFFFFFFFFF) for v in vals))
    fl = np.array([1.5, -2.25, 3e7], np.float32)
    fpacked = _ld(2, _ld(1, fl.tobytes()))
    funpacked = _ld(2, b"".join(tfr._enc_varint((1 << 3) | 5) + struct.pack("<f", v) for v in fl))
    feats = {"a": packed, "b": unpacked, "c": fpacked, "d": funpacked}
    entries = b"".join(_ld(1, _ld(1, k.encode()) + _ld(2, v)) for k, v in feats.items())
    out = tfr.parse_example(_ld(1, entries))
    assert out["a"].tolist() == vals and out["b"].tolist() == vals
    np.testing.assert_array_equal(out["c"], fl)
    np.testing.assert_array_equal(out["d"], fl)
    assert tfr._varint(tfr._enc_varint((-1) & 0xFFFFFFFFFFFFFFFF), 0)[1] == 10


@pytest.mark.parametrize("hw", [(97, 131), (9, 5), (33, 45)])
def test_mask_unpack_matches_numpy(hw):
    mh, mw = math.ceil(hw[0] / 4), math.ceil(hw[1] / 4)
    m = np.random.default_rng(3).integers(0, 2, (mh, mw, 2)).astype(np.uint8)
    packed = np.packbits(m)
    np.testing.assert_array_equal(tfr.unpack_masks(packed.tobytes(), mh, mw), m)
    np.testing.assert_array_equal(tfr.unpack_masks(packed, mh, mw).reshape(-1),
                                  np.unpackbits(packed)[:mh * mw * 2])


def _people(rng, h, w, p):
    y0 = rng.uniform(0, h * 0.6, p)
    x0 = rng.uniform(0, w * 0.6, p)
    boxes = np.stack([y0, x0, y0 + rng.uniform(20, h * 0.4, p), x0 + rng.uniform(20, w * 0.4, p)], 1).astype(np.float32)
    kp = np.stack([rng.integers(0, h, (p, 17)), rng.integers(0, w, (p, 17)), rng.integers(0, 3, (p, 17))], 2)
    return boxes, kp.astype(np.int32)


def test_crop_sampler_invariants():
    rng = np.random.default_rng(4)
    for _ in range(300):
        h, w = int(rng.integers(60, 700)), int(rng.integers(60, 700))
        boxes, _ = _people(rng, h, w, int(rng.integers(1, 5)))
        nb = boxes / np.array([h, w, h, w], np.float32)
        (y, x, ch, cw), win = ka.sample_distorted_bounding_box(rng, h, w, nb)
        assert 0 <= y and 0 <= x and y + ch <= h and x + cw <= w and ch >= 1 and cw >= 1
        np.testing.assert_allclose(win, [y / h, x / w, (y + ch) / h, (x + cw) / w], rtol=1e-6)
        if (y, x, ch, cw) == (0, 0, h, w):
            continue
        assert 0.5 * h * w - (ch + cw + 1) <= ch * cw <= h * w
        assert 0.95 - 1.0 / ch - 1e-6 <= cw / ch <= 1.05 + 1.0 / ch + 1e-6
        r = np.stack([(nb[:, 0] * h).astype(np.int32), (nb[:, 1] * w).astype(np.int32),
                      (nb[:, 2] * h).astype(np.int32), (nb[:, 3] * w).astype(np.int32)], 1)
        ih = np.maximum(0, np.minimum(y + ch, r[:, 2]) - np.maximum(y, r[:, 0]))
        iw = np.maximum(0, np.minimum(x + cw, r[:, 3]) - np.maximum(x, r[:, 1]))
        area = (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
        assert np.any((area >= 1) & (ih * iw >= 0.9 * area - 1e-3))


def test_training_sampler_keeps_keypoints_inside_and_counts_persons():
    rng = np.random.default_rng(5)
    seen = 0
    for _ in range(300):
        h, w = int(rng.integers(97, 481)), int(rng.integers(131, 641))
        boxes, kp = _people(rng, h, w, int(rng.integers(1, 6)))
        d, b, k = ka.sample_training(rng, h, w, boxes, kp, (512, 384))
        seen |= int(d["flags"])
        assert b.shape == (k.shape[0], 4) and k.shape[1:] == (17, 3)
        vis = k[:, :, 2] > 0
        assert np.all(k[:, :, 0][vis] >= 0) and np.all(k[:, :, 0][vis] < 512)
        assert np.all(k[:, :, 1][vis] >= 0) and np.all(k[:, :, 1][vis] < 384)
        assert d["crop_y"] + d["crop_h"] <= h and d["crop_x"] + d["crop_w"] <= w
        assert (d["valid_h"], d["valid_w"], d["valid_mh"], d["valid_mw"]) == (512, 384, 128, 96)
        ka.check_descriptors(d.reshape(1), h * w * 3, 10 ** 6, 512, 384)
    assert seen == ka.ROTATE | ka.COLOR | ka.GRAYSCALE | ka.PIXEL_SCALE | ka.FLIP


def test_flip_is_an_involution():
    assert np.array_equal(ka.FLIP_ORDER[ka.FLIP_ORDER], np.arange(17))
    rng = np.random.default_rng(6)
    boxes, kp = _people(rng, 256, 384, 4)
    b1, k1 = ka.flip_left_right(boxes, kp, 384)
    b2, k2 = ka.flip_left_right(b1, k1, 384)
    np.testing.assert_array_equal(k2, kp)
    np.testing.assert_allclose(b2, boxes, atol=1e-4)
    assert np.all(b1[:, 1] <= b1[:, 3])


def test_evaluation_sizes():
    assert ka.evaluation_size(480, 640) == (512, 683, 512, 768)
    assert ka.evaluation_size(640, 427) == (767, 512, 768, 512)
    d, b, k, size = ka.sample_evaluation(480, 640, *_people(np.random.default_rng(7), 480, 640, 2))
    assert size == (512, 768) and d["flags"] == ka.EVAL and d["valid_mw"] == math.ceil(683 / 4)


def test_same_seed_same_batches_at_any_thread_count():
    torch = pytest.importorskip("torch")
    from multiposenet_amd.detector.input_pipeline.keypoints_detector_pipeline import KeypointPipeline
    rng = np.random.default_rng(8)
    exs = []
    for _ in range(12):
        h, w = int(rng.integers(97, 300)), int(rng.integers(131, 300))
        boxes, kp = _people(rng, h, w, 3)
        mh, mw = math.ceil(h / 4), math.ceil(w / 4)
        exs.append({"image": rng.integers(0, 256, (h, w, 3)).astype(np.uint8), "boxes": boxes, "keypoints": kp,
                    "masks": np.packbits(rng.integers(0, 2, (mh, mw, 2)).astype(np.uint8))})
    params = {"batch_size": 4, "image_size": (256, 256), "seed": 3, "shuffle_buffer_size": 5}

    def host_batches(threads):
        pipe = KeypointPipeline(exs, True, params, device="cpu", num_threads=threads)
        shuffle_rng, rng = pipe.generators()
        recs = pipe._records(shuffle_rng)
        out = []
        for _ in range(4):
            batch = [next(recs) for _ in range(4)]
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(threads) as pool:
                decoded = list(pool.map(pipe._decode, batch))
            out.append(pipe.sample(rng, decoded))
        return out
    a, b = host_batches(1), host_batches(12)
    for (da, pa, *_), (db, pb, *_) in zip(a, b):
        assert da.tobytes() == db.tobytes()
        for (ba, ka_), (bb, kb) in zip(pa, pb):
            np.testing.assert_array_equal(ba, bb)
            np.testing.assert_array_equal(ka_, kb)
    assert torch is not None


def test_descriptor_dtype_matches_the_library():
    from multiposenet_amd import _lib
    assert ka.DESC_DTYPE.itemsize == _lib.lib().mpn_keypoint_augment_desc_bytes() == 192
