"""GPU: mpn_coco_masks through coco_records.CocoMaskRasterizer against the plain-loop transcription
(tests/coco_mask_ref.py) on the case groups of tests/coco_mask_cases.py: the full-resolution masks and the packed bits are
EQUAL byte for byte, one device call per group. Then `write_shards` on a toy data set, read back by `KeypointPipeline`."""
import os

import numpy as np
import pytest

import coco_mask_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rasterizer(cuda):
    from multiposenet_amd.coco_records import CocoMaskRasterizer
    return CocoMaskRasterizer(64)


def _check(got_packed, got_full, items, packed, full):
    assert len(got_packed) == len(got_full) == len(items)
    for i, (h, w, _) in enumerate(items):
        assert got_full[i].shape == (h, w, 2) and got_full[i].dtype == np.uint8 and got_packed[i].dtype == np.uint8
        bad = np.argwhere(got_full[i] != full[i])
        assert bad.size == 0, f"image {i} ({h} x {w}): {len(bad)} full-resolution values differ, the first at (y, x, c) = {bad[0]}"
        assert np.array_equal(got_packed[i], packed[i]), f"image {i} ({h} x {w}): packed masks differ"


@pytest.mark.parametrize("name", ["shapes", "combinations", "coco", "random", "paths"])
def test_masks_equal_the_transcription(rasterizer, name):
    """shapes: triangle, concave, self-intersecting, sliver, two points, axis-aligned edges, .5 / .1 fractions, vertices
    outside all four sides, a polygon touching y == h - each at 1x1, 4x4, 5x7, 37x53, 64x48, 130x70 and 33x257.
    combinations: two overlapping polygons in one annotation, a dropped person over a kept one, a crowd region as run lengths
    and as the compressed string, no dropped person, no polygon at all. coco: one 640 x 427 image with 20 persons.
    random: seeded polygons of 3..40 vertices. paths: polygons over two LDS column chunks (h = 1000), 300 vertices (two groups
    of edges), a run-length code of thousands of runs, a 1024 x 1024 image."""
    items, packed, full = cases.group(name)
    got_packed, got_full = rasterizer.rasterize(items, return_full=True)
    _check(got_packed, got_full, items, packed, full)
    again = rasterizer.rasterize(items)                                # without the full-resolution output
    assert all(np.array_equal(a, b) for a, b in zip(again, packed))


def test_ragged_batch_equals_one_image_at_a_time_and_calls_leak_no_state(rasterizer):
    items, packed, full = cases.group('ragged')
    assert len(items) == 9
    _check(*rasterizer.rasterize(items, return_full=True), items, packed, full)
    for i, item in enumerate(items):
        one_packed, one_full = rasterizer.rasterize([item], return_full=True)
        assert np.array_equal(one_packed[0], packed[i]) and np.array_equal(one_full[0], full[i]), i
    # the same object again, after calls of other sizes and in another order: nothing is left in the workspace
    _check(*rasterizer.rasterize(items, return_full=True), items, packed, full)
    back = items[::-1]
    _check(*rasterizer.rasterize(back, return_full=True), back, packed[::-1], full[::-1])
    empty = [(h, w, []) for h, w, _ in items]
    got_packed, got_full = rasterizer.rasterize(empty, return_full=True)
    for (h, w, _), f in zip(empty, got_full):
        assert f[..., 0].all() and not f[..., 1].any()
    with pytest.raises(ValueError, match="1..64 images"):
        rasterizer.rasterize([])
    with pytest.raises(ValueError, match="1024"):
        rasterizer.rasterize([(8, 2000, [])])


def test_write_shards_end_to_end_and_the_pipeline_reads_them(cuda, tmp_path):
    from multiposenet_amd import coco_records as cr
    from multiposenet_amd.detector.input_pipeline import tfrecord
    from multiposenet_amd.detector.input_pipeline.keypoints_detector_pipeline import KeypointPipeline
    import coco_mask_ref as ref
    path, images_dir = cases.toy_dataset(tmp_path)
    out = str(tmp_path / "records")
    report = cr.write_shards(path, images_dir, out, 2, seed=5, batch=4)
    assert report == {'images': 6, 'written': 4, 'skipped': 2, 'shards': 2}
    want = str(tmp_path / "want")
    cr.write_shards(path, images_dir, want, 2, seed=5, batch=4, rasterizer=ref.rasterize)
    names = sorted(os.listdir(out))
    assert names == sorted(os.listdir(want)) == ['shard-0000.tfrecords', 'shard-0001.tfrecords']
    for n in names:                                                    # the device's masks in the records are the yardstick's
        assert open(os.path.join(out, n), 'rb').read() == open(os.path.join(want, n), 'rb').read()
    assert sum(1 for n in names for _ in tfrecord.read_records(os.path.join(out, n), verify_data_crc=True)) == 4
    pipeline = KeypointPipeline([os.path.join(out, n) for n in names], True,
                                {"batch_size": 2, "image_size": (128, 128), "seed": 1, "shuffle_buffer_size": 4})
    features, labels = next(iter(pipeline.batches()))
    import torch
    torch.cuda.synchronize()
    assert tuple(features["images"].shape) == (2, 128, 128, 3)
    assert labels["loss_masks"].shape[0] == 2 and labels["segmentation_masks"].shape[0] == 2
