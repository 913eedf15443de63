"""GPU: mpn_prn_examples against tests/prn_pipeline_ref.py bit for bit, PoseResidualNetworkPipeline end to end from toy
shards, and the curriculum loop of train_prn on them."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prn_pipeline_cases as cases  # noqa: E402
import prn_pipeline_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(tables):
    """One mpn_prn_examples call on NaN-filled outputs (every element must be written)."""
    import torch
    from multiposenet_amd import _lib
    dev = "cuda"

    def up(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)
    kp, bx, fp = up(tables["keypoints"]), up(tables["boxes"]), up(tables["first_person"])
    w, h, ex = up(tables["width"]), up(tables["height"]), up(tables["examples"])
    N, Q, R = len(tables["examples"]), len(tables["boxes"]), len(tables["width"])
    crops = torch.full((N, 56, 36, 17), float("nan"), device=dev)
    labels = torch.full((N, 56, 36, 17), float("nan"), device=dev)
    nbytes = _lib.lib().mpn_prn_examples_workspace_bytes(Q)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("mpn_prn_examples", _lib.ptr(kp), _lib.ptr(bx), Q, _lib.ptr(fp), _lib.ptr(w), _lib.ptr(h), R, _lib.ptr(ex),
              N, 56, 36, ref.DOWNSAMPLE, _lib.ptr(crops), _lib.ptr(labels), _lib.ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return crops.cpu().numpy(), labels.cpu().numpy()


def _compare(tables, want_crops, want_labels):
    crops, labels = _run(tables)
    dc = np.flatnonzero((crops != want_crops).reshape(len(crops), -1).any(1))
    dl = np.flatnonzero((labels != want_labels).reshape(len(labels), -1).any(1))
    print(f"examples {len(crops)}: crops differ in {dc.tolist()}, labels differ in {dl.tolist()}, "
          f"max |crop diff| {np.nanmax(np.abs(crops - want_crops)) if len(crops) else 0}")
    np.testing.assert_array_equal(crops, want_crops)
    np.testing.assert_array_equal(labels, want_labels)


def test_kernel_handmade_cases_bit_exact(cuda):
    t = cases.handmade_tables()
    want_crops, want_labels = ref.batch(t)
    cases.check_handmade(t, want_crops, want_labels)
    _compare(t, want_crops, want_labels)


@pytest.mark.parametrize("seed,images,n", [(11, 9, 32), (12, 40, 128), (13, 3, 5)])
def test_kernel_random_batches_bit_exact(cuda, seed, images, n):
    t = cases.random_tables(seed, images, n)
    want_crops, want_labels = ref.batch(t)
    cases.check_batch(t, want_crops, want_labels)
    _compare(t, want_crops, want_labels)


# ---------------------------------------------------------------- pipeline
def _jpeg_header(height, width):
    frame = struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    seg = lambda m, p: bytes([0xFF, m]) + struct.pack(">H", len(p) + 2) + p   # noqa: E731
    return b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes(9)) + seg(0xC0, frame) + seg(0xDA, bytes(10)) + b"\xff\xd9"


def _toy_shards(tmp_path, seed=0, shards=2, records=7):
    """Records in the contract of tools/make_toy_tfrecords.py; the image is a JPEG header only (it is never decoded)."""
    # (the visible count of a person is at most the drawn one: random_tables hides a third of the keypoints already)
    from multiposenet_amd.detector.input_pipeline.tfrecord import encode_example, frame_record
    rng = np.random.default_rng(seed)
    paths = []
    for s in range(shards):
        paths.append(str(tmp_path / f"shard-{s:04d}.tfrecords"))
        with open(paths[-1], "wb") as f:
            for _ in range(records):
                t = cases.random_tables(int(rng.integers(1 << 30)), images=1, n=1)
                for kp in t["keypoints"]:               # 0..17 visible keypoints, so every curriculum stage has people
                    kp[rng.permutation(17)[int(rng.integers(0, 18)):], 2] = 0
                f.write(frame_record(encode_example({
                    "image": _jpeg_header(int(t["height"][0]), int(t["width"][0])),
                    "num_persons": np.array([len(t["boxes"])], np.int64), "boxes": t["boxes"].reshape(-1),
                    "keypoints": t["keypoints"].astype(np.int64).reshape(-1), "masks": b"\0"})))
    return paths


def test_pipeline_batches_equal_the_restatement(cuda, tmp_path):
    import torch
    from multiposenet_amd.detector.input_pipeline import PoseResidualNetworkPipeline
    paths = _toy_shards(tmp_path)
    kw = dict(batch_size=8, max_keypoints=12, seed=5, shuffle_buffer_size=6)
    host = PoseResidualNetworkPipeline(paths, True, **kw).samples()
    a = PoseResidualNetworkPipeline(paths, True, **kw).batches()
    b = PoseResidualNetworkPipeline(paths, True, **kw).batches()
    flips = 0
    for _ in range(5):
        t = next(host)
        want_crops, want_labels = ref.batch(t)
        cases.check_batch(t, want_crops, want_labels)
        flips += int(t["examples"]["flip"].sum())
        (ca, la), (cb, lb) = next(a), next(b)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ca.cpu().numpy(), want_crops)
        np.testing.assert_array_equal(la.cpu().numpy(), want_labels)
        assert torch.equal(ca, cb) and torch.equal(la, lb)          # the same seed: identical tensors
    assert 0 < flips < 40
    other = next(PoseResidualNetworkPipeline(paths, True, **dict(kw, seed=6)).batches())
    assert not torch.equal(other[1], la)


def test_pipeline_evaluation_ends_on_the_partial_batch_and_feeds_model_fn(cuda, tmp_path):
    import torch
    from multiposenet_amd import prn_model
    from multiposenet_amd.detector.input_pipeline import PoseResidualNetworkPipeline
    from multiposenet_amd.keypoints_model import ModeKeys
    paths = _toy_shards(tmp_path, seed=1)
    tables = list(PoseResidualNetworkPipeline(paths, False, 8).samples())
    total = sum(len(t["examples"]) for t in tables)
    assert total % 8 != 0 and [len(t["examples"]) for t in tables] == [8] * (total // 8) + [total % 8]
    params = {"initial_learning_rate": 1e-3, "num_steps": 100, "dtype": "f32", "model_dir": str(tmp_path / "eval")}
    bufs = tuple(torch.empty((8, 56, 36, 17), device="cuda") for _ in range(2))
    n = 0
    for (crops, labels), t in zip(PoseResidualNetworkPipeline(paths, False, 8, buffers=bufs).batches(), tables):
        assert tuple(crops.shape) == (len(t["examples"]), 56, 36, 17) and crops.data_ptr() == bufs[0].data_ptr()
        want_crops, want_labels = ref.batch(t)
        np.testing.assert_array_equal(crops.cpu().numpy(), want_crops)
        np.testing.assert_array_equal(labels.cpu().numpy(), want_labels)
        got = float(prn_model.model_fn(crops, labels, ModeKeys.EVAL, params).loss)
        want = float(prn_model.model_fn(want_crops, want_labels, ModeKeys.EVAL, params).loss)
        assert np.isfinite(got) and got == want                      # the pipeline adds no arithmetic
        n += 1
    assert n == len(tables)
    prn_model.reset_registry()


def test_train_prn_curriculum_checkpoint_and_resume(cuda, tmp_path):
    from multiposenet_amd import prn_model, train_prn
    from multiposenet_amd.detector.input_pipeline import AnnotationCache, PoseResidualNetworkPipeline
    paths = _toy_shards(tmp_path, seed=2)
    model_dir = str(tmp_path / "run")
    params = dict(train_prn.PARAMS, model_dir=model_dir, batch_size=8, num_steps=40, dtype="f32")
    cache, stages, log = AnnotationCache(), [], []

    def train_batches(max_keypoints):
        stages.append(max_keypoints)
        return PoseResidualNetworkPipeline(paths, True, 8, max_keypoints, shuffle_buffer_size=8, annotations=cache).batches()

    def val_batches():
        return PoseResidualNetworkPipeline(paths, False, 8, annotations=cache).batches()
    cfg = {"save_summary_steps": 1, "log_step_count_steps": 2}
    step = train_prn.train(params, train_batches, val_batches, run_config=cfg, max_steps=3, steps_per_keypoint=2,
                           log=log.append)
    assert step == 3 and stages == [4, 5]
    assert os.path.exists(os.path.join(model_dir, "model.ckpt-2.npz")) and os.path.exists(os.path.join(model_dir, "model.ckpt-3.npz"))
    assert sum("[eval]" in ln for ln in log) == 2
    prn_model.reset_registry()                            # a fresh process: the variables come from the checkpoint
    step = train_prn.train(params, train_batches, val_batches, run_config=cfg, max_steps=4, steps_per_keypoint=2,
                           log=log.append)
    assert step == 4
    assert stages == [4, 5, 5]                            # resumed inside stage 5 (steps 2..3), not at stage 4
    assert any("restored" in ln and "global_step 3" in ln for ln in log)
    assert train_prn.latest_checkpoint(model_dir)[0] == 4
    import json
    recs = [json.loads(ln) for ln in open(os.path.join(model_dir, "summaries.jsonl"))]
    assert [r["step"] for r in recs] == [1, 2, 3, 4]
    assert all(np.isfinite(r["logloss"]) for r in recs)
    prn_model.reset_registry()
