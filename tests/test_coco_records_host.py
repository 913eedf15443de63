"""CPU: the COCO mask yardstick (tests/coco_mask_ref.py) against facts that need no library, the record rules of
multiposenet_amd/coco_records.py on a toy data set (the rasteriser replaced by the yardstick, so no device is needed), and
the argument checks of mpn_coco_masks, which run before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

import coco_mask_cases as cases
import coco_mask_ref as ref
from multiposenet_amd import _lib
from multiposenet_amd import coco_records as cr
from multiposenet_amd.detector.input_pipeline import tfrecord


# ---------------------------------------------------------------- the transcription
@pytest.mark.parametrize("h,w,x0,y0,x1,y1", [(8, 9, 2, 3, 6, 7), (37, 53, 0, 0, 53, 37), (33, 40, 5, 31, 6, 33), (5, 7, 6, 0, 7, 5),
                                             (64, 48, 10, 20, 11, 21)])
def test_integer_rectangle_sets_exactly_its_pixels(h, w, x0, y0, x1, y1):
    m = ref.annotation_mask([[x0, y0, x1, y0, x1, y1, x0, y1]], h, w)
    want = np.zeros((h, w), np.uint8)
    want[y0:y1, x0:x1] = 1
    np.testing.assert_array_equal(m, want)


def test_rle_round_trips():
    rng = np.random.default_rng(1)
    for h, w in [(1, 1), (5, 7), (37, 53)]:
        for p in (0.0, 0.3, 1.0):
            m = (rng.random((h, w)) < p).astype(np.uint8)
            runs = ref.rle_encode(m)
            assert sum(runs) == h * w
            np.testing.assert_array_equal(ref.rle_decode(runs, h, w), m)
            s = ref.rle_to_string(runs)
            assert ref.rle_from_string(s) == runs == cr.rle_from_string(s)
    # run lengths that need several characters and a negative difference
    runs = [0, 70000, 3, 5, 1000000, 2]
    assert ref.rle_from_string(ref.rle_to_string(runs)) == runs == cr.rle_from_string(ref.rle_to_string(runs))
    # the union of two codes is the OR of their masks
    a, b = (rng.random((9, 11)) < 0.4).astype(np.uint8), (rng.random((9, 11)) < 0.4).astype(np.uint8)
    np.testing.assert_array_equal(ref.rle_decode(ref.rle_merge([ref.rle_encode(a), ref.rle_encode(b)]), 9, 11), a | b)


@pytest.mark.parametrize("h,w", [(4, 4), (5, 7), (37, 53)])
def test_constant_masks_survive_the_lanczos_stage(h, w):
    mh, mw = -(-h // 4), -(-w // 4)
    for v in (0, 1):
        small = ref.lanczos_quarter(np.full((h, w, 2), v, np.uint8))
        assert small.shape == (mh, mw, 2) and small.dtype == np.uint8
        np.testing.assert_array_equal(small, np.full((mh, mw, 2), v, np.uint8))
    for src, dst in [(w, mw), (h, mh)]:
        first, weights = ref.lanczos_taps(src, dst)
        assert np.all(np.abs(weights.astype(np.int64).sum(1) - 2048) <= 4)      # eight weights rounded to 11 bits
        taps = cr.lanczos_taps(src, dst)                                        # the product's tables are the yardstick's
        np.testing.assert_array_equal(taps['first'], first)
        np.testing.assert_array_equal(taps['weights'], weights)


def test_packed_bytes_pass_unpack_masks():
    h, w = 33, 257
    anns = [{'segmentation': [[10.0, 5.0, 200.0, 8.0, 120.0, 30.0]], 'dropped': False},
            {'segmentation': [[0.0, 0.0, 40.0, 0.0, 40.0, 33.0, 0.0, 33.0]], 'dropped': True}]
    packed, full = ref.rasterize_image(h, w, anns)
    mh, mw = 9, 65
    assert packed.dtype == np.uint8 and packed.size == (mh * mw * 2 + 7) // 8 == _lib.lib().mpn_coco_masks_packed_bytes(h, w)
    masks = tfrecord.unpack_masks(packed, mh, mw)
    np.testing.assert_array_equal(masks, (ref.lanczos_quarter(full) > 0).astype(np.uint8))
    assert packed[-1] & 0x3f == 0                                                # 1170 bits: the last byte is zero-padded
    assert full[:, :40, 0].max() == 0 and full[:, 41:, 0].min() == 1             # the dropped person is out of the loss
    assert masks[:, :9, 0].max() == 0 and masks[:, 12:, 0].min() == 1 and masks[..., 1].any()


def test_cases_cover_what_they_claim():
    items, packed, full = cases.group('combinations')
    a, b = full[0][..., 1], full[1]
    assert a[int(0.5 * 64), int(0.5 * 48)] == 1                                  # the overlap of the two polygons: OR, not XOR
    assert b[..., 1].any() and (b[..., 0] == 0).any() and ((b[..., 1] == 1) & (b[..., 0] == 0)).any()
    np.testing.assert_array_equal(packed[3], packed[4])                          # the run lengths and their string
    np.testing.assert_array_equal(full[3], full[4])
    assert (full[3][..., 0] == 0).any()
    assert full[6][..., 0].all() and not full[6][..., 1].any() and full[7][..., 0].all() and not full[7][..., 1].any()
    assert len({(h, w) for h, w, _ in cases.group('ragged')[0]}) == 9
    for h, w, anns in cases.group('shapes')[0] + cases.group('random')[0]:
        cr._Batch([(h, w, anns)], False)                                         # the product's checks accept every case


# ---------------------------------------------------------------- the record rules
def test_record_rules_on_the_toy_data_set(tmp_path):
    path, images_dir = cases.toy_dataset(tmp_path)
    entries = dict(cr.person_images(path))
    assert sorted(entries) == ['a.jpg', 'b.jpg', 'c.png', 'd.jpg', 'e.jpg', 'f.jpg']
    assert cr.read_image(os.path.join(images_dir, 'c.png')) is None
    data, h, w = cr.read_image(os.path.join(images_dir, 'a.jpg'))
    assert (h, w) == (48, 64) and data == open(os.path.join(images_dir, 'a.jpg'), 'rb').read()
    persons = cr.apply_record_rules(entries['a.jpg'], h, w)
    assert [p['dropped'] for p in persons] == [False, True, True, False]
    assert persons[0]['box'] == (6.25, 5.5, 41.25, 35.5)
    assert persons[3]['box'] == (38.0, 50.0, 48.0, 64.0)                         # clipped to the image
    kp = persons[3]['keypoints']
    assert kp.dtype == np.int64 and kp.shape == (17, 3)
    assert kp[:, 0].max() == 47 and kp[:, 1].max() == 63 and kp[0].tolist() == [44, 60, 2]     # (y, x, v), clipped
    packed = ref.rasterize([(h, w, persons)])[0]
    example = cr.to_example(data, persons, packed)
    got = tfrecord.decode_keypoint_example(example)
    assert got['image'].shape == (48, 64, 3)
    np.testing.assert_array_equal(got['boxes'], np.array([[6.25, 5.5, 41.25, 35.5], [38, 50, 48, 64]], np.float32))
    np.testing.assert_array_equal(got['keypoints'][1], kp.astype(np.int32))
    masks = tfrecord.unpack_masks(got['masks'], 12, 16)
    assert masks[..., 1].any() and (masks[..., 0] == 0).any() and masks[..., 0].any()
    feats = tfrecord.parse_example(example)
    assert set(feats) == {'image', 'num_persons', 'boxes', 'keypoints', 'masks'} and feats['num_persons'].tolist() == [2]
    # only dropped persons: no record
    bd, bh, bw = cr.read_image(os.path.join(images_dir, 'b.jpg'))
    dropped = cr.apply_record_rules(entries['b.jpg'], bh, bw)
    assert all(p['dropped'] for p in dropped) and cr.to_example(bd, dropped, packed) is None
    # a grayscale JPEG is stored as RGB
    from PIL import Image
    import io
    gd, gh, gw = cr.read_image(os.path.join(images_dir, 'd.jpg'))
    assert (gh, gw) == (37, 53) and gd != open(os.path.join(images_dir, 'd.jpg'), 'rb').read()
    assert Image.open(io.BytesIO(gd)).mode == 'RGB' and Image.open(os.path.join(images_dir, 'd.jpg')).mode == 'L'


def test_write_shards_is_deterministic_and_readable(tmp_path):
    path, images_dir = cases.toy_dataset(tmp_path)
    reports, blobs = [], []
    for out in ('one', 'two'):
        reports.append(cr.write_shards(path, images_dir, str(tmp_path / out), 2, seed=5, batch=4, rasterizer=ref.rasterize))
        names = sorted(os.listdir(tmp_path / out))
        assert names == ['shard-0000.tfrecords', 'shard-0001.tfrecords']
        blobs.append([open(tmp_path / out / n, 'rb').read() for n in names])
    assert reports[0] == reports[1] == {'images': 6, 'written': 4, 'skipped': 2, 'shards': 2}
    assert blobs[0] == blobs[1]
    other = cr.write_shards(path, images_dir, str(tmp_path / 'three'), 2, seed=6, batch=4, rasterizer=ref.rasterize)
    assert other == reports[0]
    assert [open(tmp_path / 'three' / n, 'rb').read() for n in sorted(os.listdir(tmp_path / 'three'))] != blobs[0]
    counts, sizes = [], set()
    for n in sorted(os.listdir(tmp_path / 'one')):
        records = list(tfrecord.read_records(str(tmp_path / 'one' / n), verify_data_crc=True))
        counts.append(len(records))
        for r in records:
            ex = tfrecord.decode_keypoint_example(r)
            h, w = ex['image'].shape[:2]
            sizes.add((h, w))
            assert len(ex['boxes']) >= 1 and ex['masks'].size == (-(-h // 4) * -(-w // 4) * 2 + 7) // 8
            if (h, w) == (33, 70):                                               # f.jpg: the crowd region (columns 0..11) masks the loss
                masks = tfrecord.unpack_masks(ex['masks'], 9, 18)
                assert masks[:, :2, 0].max() == 0 and masks[:, 5:, 0].min() == 1
    assert counts == [3, 1] and sizes == {(48, 64), (37, 53), (64, 48), (33, 70)}


def test_rasterizer_refuses_bad_input_before_any_launch():
    good = [{'segmentation': [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]], 'dropped': False}]
    cr._Batch([(8, 8, good)], False)
    with pytest.raises(ValueError, match="1024"):
        cr._Batch([(1025, 8, good)], False)
    with pytest.raises(ValueError, match="1024"):
        cr._Batch([(8, 0, good)], False)
    with pytest.raises(ValueError, match="not finite"):
        cr._Batch([(8, 8, [{'segmentation': [[1.0, float('nan'), 5.0, 1.0, 5.0, 5.0]], 'dropped': False}])], False)
    with pytest.raises(ValueError, match="not finite"):
        cr._Batch([(8, 8, [{'segmentation': [[1.0, float('inf'), 5.0, 1.0, 5.0, 5.0]], 'dropped': True}])], False)
    with pytest.raises(ValueError, match="outside the image"):
        cr._Batch([(8, 8, [{'segmentation': [[1.0, 1.0, 16.5, 1.0, 5.0, 5.0]], 'dropped': False}])], False)
    with pytest.raises(ValueError, match="outside the image"):
        cr._Batch([(8, 8, [{'segmentation': [[1.0, -8.5, 5.0, 1.0, 5.0, 5.0]], 'dropped': False}])], False)
    with pytest.raises(ValueError, match="uint32"):
        cr._Batch([(8, 8, [{'segmentation': {'counts': [3, -1, 62]}, 'dropped': True}])], False)


# ---------------------------------------------------------------- the launcher
def test_launcher_checks_run_before_any_hip_call():
    P = ctypes.c_void_p(4096)
    ok = [P, 1, 640, P, 1, P, 6, P, 3, P, 280, P, 4096, P, 4096, None, 0, None]

    def call(**change):
        names = ["images", "num_images", "max_side", "parts", "num_parts", "xy", "num_xy", "runs", "num_runs", "taps", "num_taps",
                 "workspace", "workspace_bytes", "packed", "packed_bytes", "full", "full_bytes", "stream"]
        args = list(ok)
        for k, v in change.items():
            args[names.index(k)] = v
        _lib.call("mpn_coco_masks", *args)

    with pytest.raises(ValueError, match="1024"):
        call(max_side=1025)
    with pytest.raises(ValueError, match="max_side"):
        call(max_side=0)
    with pytest.raises(ValueError, match="num_images"):
        call(num_images=0)
    for name in ("images", "parts", "xy", "runs", "taps", "workspace", "packed"):
        with pytest.raises(ValueError, match="null pointer"):
            call(**{name: None})
    with pytest.raises(ValueError, match="aligned"):
        call(workspace=ctypes.c_void_p(4100))
    with pytest.raises(ValueError, match="aligned"):
        call(xy=ctypes.c_void_p(4100))
    with pytest.raises(_lib.MpnError, match="workspace_bytes"):
        call(workspace_bytes=100)
    with pytest.raises(_lib.MpnError, match="full_bytes"):
        call(full=P, full_bytes=0)
    lib = _lib.lib()
    assert lib.mpn_coco_masks_image_desc_bytes() == cr._IMAGE_DESC.itemsize == 40
    assert lib.mpn_coco_masks_part_desc_bytes() == cr._PART_DESC.itemsize == 24
    assert lib.mpn_coco_masks_plane_words(427, 640) == 2 * 640 * 14 and lib.mpn_coco_masks_plane_words(1, 1) == 2
    assert lib.mpn_coco_masks_packed_bytes(427, 640) == (107 * 160 * 2 + 7) // 8 and lib.mpn_coco_masks_packed_bytes(1, 1) == 1
    assert lib.mpn_coco_masks_plane_words(1025, 8) == 0 == lib.mpn_coco_masks_packed_bytes(8, 1025)
    assert lib.mpn_coco_masks_plane_words(0, 8) == 0 and lib.mpn_coco_masks_plane_words(1024, 1024) == 2 * 1024 * 32
    assert cr.MAX_SIDE == 1024
