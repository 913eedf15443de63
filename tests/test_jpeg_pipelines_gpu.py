"""GPU: device JPEG decode behind its three consumers. `KeypointPipeline` and `DetectorPipeline` with decode='device' yield the
batches of decode='host' bit for bit from the same seed (TFRecords in the contract of tools/make_toy_tfrecords.py plus one
progressive record, and in-memory examples), and `Detector.predict_jpegs` returns exactly what `predict_images` returns for the
frames Pillow decodes."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from multiposenet_amd.detector.input_pipeline.keypoints_detector_pipeline import KeypointPipeline
from multiposenet_amd.detector.input_pipeline.person_detector_pipeline import DetectorPipeline
from multiposenet_amd.detector.input_pipeline.tfrecord import (decode_keypoint_example, encode_example, frame_record,
                                                               parse_example)
from multiposenet_amd.inference import jpeg as J
from test_detector_batch_gpu import _detector, models  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy():
    spec = importlib.util.spec_from_file_location("make_toy_tfrecords", os.path.join(ROOT, "tools", "make_toy_tfrecords.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _progressive(record):
    """The record with its image re-encoded as a progressive JPEG (which the device path leaves to Pillow)."""
    from PIL import Image
    f = parse_example(record)
    buf = io.BytesIO()
    Image.open(io.BytesIO(f["image"][0])).save(buf, format="JPEG", quality=85, progressive=True)
    assert J.jpeg_info(buf.getvalue())['reason'] == 'progressive'
    feats = {k: (v[0] if k in ("image", "masks") else v) for k, v in f.items()}
    feats["image"] = buf.getvalue()
    return encode_example(feats)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    toy = _toy()
    d = tmp_path_factory.mktemp("jpeg_records")
    rng = np.random.default_rng(11)
    paths = []
    for s in range(2):
        records = [toy.toy_example(rng) for _ in range(6)]
        if s == 0:
            records[2] = _progressive(records[2])
        paths.append(str(d / f"shard-{s:04d}.tfrecords"))
        with open(paths[-1], "wb") as f:
            for r in records:
                f.write(frame_record(r))
    return paths


def _same_batches(a, b, count):
    n = 0
    for (fa, la), (fb, lb) in zip(a, b):
        torch.cuda.synchronize()
        for da, db in ((fa, fb), (la, lb)):
            assert set(da) == set(db)
            for k in da:
                assert da[k].shape == db[k].shape and da[k].dtype == db[k].dtype, k
                assert torch.equal(da[k], db[k]), f"batch {n}: '{k}' differs between decode='host' and decode='device'"
        n += 1
        if n == count:
            break
    return n


@pytest.mark.parametrize("pipeline", [KeypointPipeline, DetectorPipeline])
def test_training_batches_are_bit_identical_in_both_modes(cuda, shards, pipeline):
    params = {"batch_size": 4, "image_size": (256, 128), "seed": 9, "shuffle_buffer_size": 5}
    host = pipeline(shards, True, params, decode='host').batches()
    dev = pipeline(shards, True, params, decode='device').batches()
    assert _same_batches(host, dev, 7) == 7             # 28 records of 12: every record, the progressive one included


@pytest.mark.parametrize("pipeline", [KeypointPipeline, DetectorPipeline])
def test_evaluation_batches_are_bit_identical_in_both_modes(cuda, shards, pipeline):
    params = {"min_dimension": 256}
    host = pipeline(shards, False, params, decode='host').batches()
    dev = pipeline(shards, False, params, decode='device').batches()
    assert _same_batches(host, dev, 12) == 12


def test_in_memory_examples_work_in_both_modes(cuda, shards):
    """Decoded arrays pass through decode='device' as pixels; an in-memory example may also carry JPEG bytes."""
    from multiposenet_amd.detector.input_pipeline.tfrecord import read_records
    records = list(read_records(shards[1]))
    decoded = [decode_keypoint_example(r) for r in records]
    as_bytes = [decode_keypoint_example(r, decode_image=False) for r in records]
    mixed = [a if i % 2 else b for i, (a, b) in enumerate(zip(decoded, as_bytes))]
    params = {"batch_size": 3, "image_size": (128, 128), "seed": 2, "shuffle_buffer_size": 1}
    want = KeypointPipeline(decoded, True, params).batches()
    for examples in (decoded, mixed):
        assert _same_batches(want, KeypointPipeline(examples, True, params, decode='device').batches(), 3) == 3
        want = KeypointPipeline(decoded, True, params).batches()


def test_predict_jpegs_equals_predict_images_of_pillows_pixels(cuda, models, shards):
    from multiposenet_amd.detector.input_pipeline.tfrecord import read_records
    jpegs = [bytes(parse_example(r)["image"][0]) for r in read_records(shards[0])][:4]     # [2] is progressive
    from test_jpeg_host import goldens
    g = goldens()
    jpegs += [g["120x160_422_checker"][0], g["37x53_gray"][0], g["17x17_cmyk"][0]]
    frames = [J.pillow_decode(j) for j in jpegs]
    det = _detector(models)
    for kwargs in ({"size": (128, 128), "score_threshold": 0.0, "annotate": True},
                   {"size": (128, 256), "keep_aspect_ratio": True, "score_threshold": 0.35, "return_heatmaps": True},
                   {"size": (128, 128), "score_threshold": 0.0, "annotate": True}):          # the graph of the first call, replayed
        want = det.predict_images(frames, **kwargs)
        got = det.predict_jpegs(jpegs, **kwargs)
        assert len(got) == len(want) == len(jpegs)
        for i, (a, b) in enumerate(zip(got, want)):
            assert set(a) == set(b)
            for k in a:
                assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (i, k)
        if kwargs.get("annotate"):
            assert all(p['annotated'].shape == f.shape[:2] + (4,) for p, f in zip(got, frames))
    # fewer frames, another order: the same capacity, other sizes
    got = det.predict_jpegs(jpegs[::-1][:3], size=(128, 128), score_threshold=0.0)
    want = det.predict_images(frames[::-1][:3], size=(128, 128), score_threshold=0.0)
    for a, b in zip(got, want):
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    eager = _detector(models, graph=False)
    got = eager.predict_jpegs(jpegs[:2], size=(128, 128), score_threshold=0.0)
    want = eager.predict_images(frames[:2], size=(128, 128), score_threshold=0.0)
    for a, b in zip(got, want):
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
