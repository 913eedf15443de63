"""GPU: the device's JPEG entropy stage behind its three consumers. `KeypointPipeline` and `DetectorPipeline` with
decode='device', entropy='device' yield the batches of decode='host' bit for bit from the same seed (one progressive record
among the records), and `Detector.predict_jpegs(entropy='device')` returns the dicts of entropy='host' while it uploads less."""
import numpy as np
import pytest
import torch

from multiposenet_amd.detector.input_pipeline.keypoints_detector_pipeline import KeypointPipeline
from multiposenet_amd.detector.input_pipeline.person_detector_pipeline import DetectorPipeline
from multiposenet_amd.detector.input_pipeline.tfrecord import parse_example, read_records
from test_detector_batch_gpu import _detector, models  # noqa: F401
from test_jpeg_pipelines_gpu import _same_batches, shards  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pipeline", [KeypointPipeline, DetectorPipeline])
def test_training_batches_are_bit_identical_with_the_entropy_stage_on_the_device(cuda, shards, pipeline):
    params = {"batch_size": 4, "image_size": (256, 128), "seed": 9, "shuffle_buffer_size": 5}
    host = pipeline(shards, True, params, decode='host').batches()
    dev = pipeline(shards, True, params, decode='device', entropy='device').batches()
    assert _same_batches(host, dev, 4) == 4             # 16 records of 12: every record, the progressive one included


def test_entropy_mode_is_checked(cuda, shards):
    with pytest.raises(ValueError, match="entropy"):
        KeypointPipeline(shards, True, {"batch_size": 1, "image_size": (128, 128)}, decode='device', entropy='gpu')
    with pytest.raises(ValueError, match="needs decode='device'"):
        DetectorPipeline(shards, True, {"batch_size": 1, "image_size": (128, 128)}, decode='host', entropy='device')


def test_predict_jpegs_returns_the_same_dicts_in_both_entropy_modes(cuda, models, shards):
    jpegs = [bytes(parse_example(r)["image"][0]) for r in read_records(shards[1])][:4]
    det = _detector(models)
    want = det.predict_jpegs(jpegs, size=(128, 128), score_threshold=0.0)
    staged_host = det.jpeg_staged_bytes
    got = det.predict_jpegs(jpegs, size=(128, 128), score_threshold=0.0, entropy='device')
    assert det.jpeg_fallbacks == 0 and 0 < det.jpeg_staged_bytes < staged_host, (det.jpeg_staged_bytes, staged_host)
    assert len(got) == len(want) == 4
    for i, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b)
        for k in a:
            assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (i, k)
