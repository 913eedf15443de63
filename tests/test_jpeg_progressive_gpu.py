"""GPU: progressive and Adobe CMYK JPEGs through `JpegBatchDecoder` (the multi-scan host stage, then mpn_jpeg_decode with its
four-component case), held byte for byte to the pixels Pillow decoded (tests/golden/jpeg_progressive_goldens.npz); the same
batch beside the baseline goldens; and `Detector.predict_jpegs` on such files. No tolerance anywhere."""
import numpy as np
import pytest
import torch

import jpeg_progressive_ref as P
from jpeg_progressive_cases import CASES
from multiposenet_amd.inference import jpeg as J
from test_detector_batch_gpu import _detector, models  # noqa: F401
from test_jpeg_decode_gpu import SENTINEL, _run
from test_jpeg_host import goldens as baseline_goldens, supported_cases

pytestmark = pytest.mark.gpu


def test_every_golden_in_one_ragged_batch_equals_pillow(cuda):
    g = P.goldens()
    names = [c[0] for c in CASES]
    entries = [J.prepare(g[n][0], extended=True) for n in names]
    assert all(isinstance(e, J.Coefficients) for e in entries)
    assert {int(e.desc[0]['components']) for e in entries} == {1, 3, 4}
    dec = _run(cuda, entries, [g[n][1] for n in names])
    assert dec.fallbacks == 0


@pytest.mark.parametrize("entropy", J.ENTROPY_MODES)
def test_the_batch_mixed_with_baseline_goldens_equals_pillow(cuda, entropy):
    """Three-component and grayscale entries decode to the same bytes beside four-component ones; with entropy='device' the
    baseline files are Scan entries and the progressive / CMYK ones still arrive as Coefficients: nothing falls back."""
    g, b = P.goldens(), baseline_goldens()
    new, old = [c[0] for c in CASES if c[2] != (120, 160)], [c[0] for c in supported_cases()]
    files, wants = [], []
    for i in range(max(len(new), len(old))):                # interleaved: 4-component descriptors between the others
        for names, src in ((new, g), (old, b)):
            if i < len(names):
                files.append(src[names[i]][0])
                wants.append(src[names[i]][1])
    entries = [J.prepare(f, entropy, extended=True) for f in files]
    kinds = {type(e) for e in entries}
    assert kinds == ({J.Coefficients, J.Scan} if entropy == 'device' else {J.Coefficients})
    dec = _run(cuda, entries, wants, gap=16)
    assert dec.fallbacks == 0


def test_a_four_component_descriptor_out_of_range_is_skipped(cuda):
    """quant3 names one of the three tables, and CMYK is 1x1 only: any other descriptor writes nothing."""
    g = P.goldens()
    want = g["17x17_cmyk"][1]
    for field, value in (('quant3', 3), ('quant3', -1), ('h_samp', 2)):
        entry = J.prepare(g["17x17_cmyk"][0], extended=True)
        entry.desc[0][field] = value
        sources = torch.full((64 + want.size + 64,), SENTINEL, dtype=torch.uint8, device=cuda)
        J.JpegBatchDecoder(cuda).decode([entry], sources, [64])
        torch.cuda.synchronize()
        assert (sources.cpu().numpy() == SENTINEL).all(), (field, value)


@pytest.mark.parametrize("entropy", J.ENTROPY_MODES)
def test_predict_jpegs_on_progressive_and_cmyk_equals_predict_images_of_pillows_pixels(cuda, models, entropy):
    g = P.goldens()
    jpegs = [g["120x160_p420"][0], g["37x53_cmyk"][0]]
    frames = [J.pillow_decode(j) for j in jpegs]
    for f, n in zip(frames, ("120x160_p420", "37x53_cmyk")):
        np.testing.assert_array_equal(f, g[n][1])
    det = _detector(models)
    want = det.predict_images(frames, size=(128, 128), score_threshold=0.0)
    got = det.predict_jpegs(jpegs, size=(128, 128), score_threshold=0.0, entropy=entropy)
    assert det.jpeg_fallbacks == 0 and len(got) == len(want) == 2
    for i, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b)
        for k in a:
            assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (i, k)
