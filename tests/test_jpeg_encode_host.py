"""CPU: the host side of the JPEG encode (quality tables, headers, batch plan, argument checks) and the numpy restatement of
its device side (tests/jpeg_encode_ref.py), held byte for byte to the files Pillow wrote (tests/golden/jpeg_encode_goldens.npz)
and, coefficient for coefficient, to what the project's own host Huffman decoder reads from those files."""
import ctypes
import os

import numpy as np
import pytest

import jpeg_encode_ref as R
from jpeg_encode_cases import CASES, SIZES, SUBSAMPLING
from multiposenet_amd import _lib
from multiposenet_amd.inference import jpeg as J

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_goldens.npz")
_CACHE = {}


def goldens():
    """name -> (pixels uint8 [h, w, channels], Pillow's file). Loaded once."""
    if not _CACHE:
        with np.load(GOLDEN) as z:
            assert [str(n) for n in z["names"]] == [c[0] for c in CASES]
            assert any(str(v).startswith("Pillow ") for v in z["versions"])
            _CACHE.update({c[0]: (z[f"{c[0]}/pixels"], z[f"{c[0]}/jpeg"].tobytes()) for c in CASES})
    return _CACHE


def reference():
    """name -> (coefficients, scan, file) of the restatement. Computed once, shared by the tests."""
    if 'ref' not in _CACHE:
        g = goldens()
        _CACHE['ref'] = {name: R.encode(g[name][0], quality, sub) for name, _, _, _, sub, quality, _ in CASES}
    return _CACHE['ref']


def scan_of(data):
    at = data.index(b"\xff\xda")
    return data[at + 2 + ((data[at + 2] << 8) | data[at + 3]):]


def test_case_table_covers_what_the_issue_lists():
    assert {(c[2], c[4]) for c in CASES} >= {(s, sub) for s in SIZES for sub in SUBSAMPLING}
    assert {(1, 1), (8, 8), (9, 9), (16, 16), (17, 23), (24, 8), (8, 24), (33, 65), (40, 56), (50, 31)} <= set(SIZES)
    assert {c[5] for c in CASES} >= {10, 75, 95, 100} and {c[3] for c in CASES} == {'noise', 'ramp', 'binary'}
    big = [c for c in CASES if c[2] == (120, 160)]
    assert {(c[3], c[4], c[5]) for c in big} == {('binary', '4:4:4', 100), ('binary', '4:2:0', 100)}
    assert any(c[6] == 4 for c in CASES)
    assert all(c[2][0] <= 120 and c[2][1] <= 160 for c in CASES) and os.path.getsize(GOLDEN) <= 400 * 1024
    g = goldens()
    for name, *_ in big:
        assert len(g[name][1]) > 40000                             # many chunks of words, hundreds of blocks per plane
    for c in CASES:
        if c[6] == 4:
            assert (g[c[0]][0][..., 3] != 255).all()


def test_goldens_exercise_stuffing_zrl_and_dummy_blocks():
    import make_jpeg_encode_goldens as M
    M.check_set({n: f for n, (_, f) in goldens().items()})
    assert max(scan_of(f).count(b"\xff\x00") for _, f in goldens().values()) >= 8
    sizes = [np.abs(J.entropy_decode(goldens()[c[0]][1]).coefs[:, 1:]).max() for c in CASES if c[5] == 100 and c[3] == 'binary']
    assert max(sizes) >= 512                                        # an AC symbol of size 10


def test_restatement_writes_pillows_file_for_every_golden():
    g, ref = goldens(), reference()
    for name, *_ in CASES:
        assert ref[name][2] == g[name][1], name


def test_restatement_coefficients_equal_the_host_decoders():
    g, ref = goldens(), reference()
    for name, *_ in CASES:
        c = J.entropy_decode(g[name][1])
        assert ref[name][0].dtype == np.int16
        np.testing.assert_array_equal(ref[name][0], c.coefs, err_msg=name)
        assert scan_of(g[name][1]) == ref[name][1], name


def test_headers_and_scan_make_the_golden_file():
    g, ref = goldens(), reference()
    for name, _, (h, w), _, sub, quality, _ in CASES:
        head = J.jpeg_headers(w, h, sub, J.quality_tables(quality))
        assert head + ref[name][1] == g[name][1], name
        assert head + scan_of(g[name][1]) == g[name][1], name


def test_quality_tables_equal_the_dqt_segments():
    g = goldens()
    seen = set()
    for name, _, _, _, _, quality, _ in CASES:
        d = J.entropy_decode(g[name][1]).desc[0]
        luma, chroma = J.quality_tables(quality)
        assert luma.dtype == np.uint16 and luma.shape == (64,)
        np.testing.assert_array_equal(d['quant'][0], luma, err_msg=name)
        np.testing.assert_array_equal(d['quant'][1], chroma, err_msg=name)
        np.testing.assert_array_equal(d['quant'][2], chroma, err_msg=name)
        seen.add(quality)
    assert seen >= {10, 75, 95, 100}
    assert (J.quality_tables(100)[0] == 1).all() and J.quality_tables(1)[1].max() == 255
    for q in (1, 25, 49, 50, 51, 99):
        for a, b in zip(J.quality_tables(q), R.quality_tables(q)):
            np.testing.assert_array_equal(a, b)
    for bad in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            J.quality_tables(bad)


def test_goldens_equal_live_pillow():
    pytest.importorskip("PIL.Image")
    import make_jpeg_encode_goldens as M
    for name, _, _, _, sub, quality, _ in CASES:
        pixels, data = goldens()[name]
        assert M.pillow_encode(pixels, quality, sub) == data, name
        assert J.pillow_encode(pixels, quality, sub) == data, name     # the fallback writes the same file


def test_restatement_equals_live_pillow_on_a_seeded_sweep():
    pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(31)
    for k in range(40):
        h, w = (int(v) for v in rng.randint(1, 45, 2))
        px = rng.randint(0, 256, (h, w, 3)).astype(np.uint8) if k % 2 else (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
        q, sub = int(rng.randint(1, 101)), ('4:4:4', '4:2:2', '4:2:0')[k % 3]
        assert R.encode(px, q, sub)[2] == J.pillow_encode(px, q, sub), (k, h, w, q, sub)


def test_plan_is_host_arithmetic():
    lib = _lib.lib()
    assert lib.mpn_jpeg_enc_desc_bytes() == J.ENC_DESC_BYTES == J.ENC_DESC.itemsize == 512 and J.RECORD.itemsize == 32
    plan = J.EncodePlan([(17, 23), (8, 8)], [0, 4096], 4, quality=95, subsampling='4:2:0', capacities=[1024, 48])
    d = plan.descs
    assert J.total_blocks(17, 23, '4:2:0') == 24 and J.total_blocks(8, 8, '4:2:0') == 6 and J.total_blocks(9, 9, '4:4:4') == 12
    assert d['coef_offset'].tolist() == [0, 24 * 128] and d['out_offset'].tolist() == [0, 1024] and d['capacity'].tolist() == [1024, 48]
    share = lib.mpn_jpeg_entropy_encode_workspace_bytes(24, 1024)
    assert share > 0 and share % 16 == 0 and d['work_offset'].tolist() == [0, share]
    assert plan.need == (30 * 128, 1024 + 48, share + lib.mpn_jpeg_entropy_encode_workspace_bytes(6, 48))
    assert (d['width'].tolist(), d['height'].tolist(), d['channels'].tolist()) == ([23, 8], [17, 8], [4, 4])
    np.testing.assert_array_equal(d['quant'][0, 2], J.quality_tables(95)[1])
    assert plan.headers[1] == J.jpeg_headers(8, 8, '4:2:0', J.quality_tables(95))
    default = J.EncodePlan([(17, 23)], [0], 3)
    assert default.descs['capacity'][0] == 24 * 64 * J.BYTES_PER_SAMPLE + 256
    for kwargs, match in (({'subsampling': '4:1:1'}, "subsampling"), ({'quality': 0}, "quality")):
        with pytest.raises(ValueError, match=match):
            J.EncodePlan([(8, 8)], [0], 3, **kwargs)
    with pytest.raises(ValueError, match="multiple of 16"):
        J.EncodePlan([(8, 8)], [8], 3)
    with pytest.raises(ValueError, match="channels"):
        J.EncodePlan([(8, 8)], [0], 1)
    with pytest.raises(ValueError, match="capacity"):
        J.EncodePlan([(8, 8)], [0], 3, capacities=[8])


def test_entry_points_validate_before_any_hip_call():
    lib, call = _lib.lib(), _lib.call
    P16, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    ws = lib.mpn_jpeg_entropy_encode_workspace_bytes
    assert ws(0, 1024) == 0 and ws(1, 8) == 0 and ws((1 << 21) + 1, 1024) == 0 and ws(6, (1 << 30) + 1) == 0
    assert ws(6, 1024) >= 6 * 4 + 1024 and ws(1 << 21, 1 << 30) > 1 << 30
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_forward", None, 1024, P16, 1, P16, 1024, None)
    with pytest.raises(ValueError, match="B must"):
        call("mpn_jpeg_forward", P16, 1024, P16, 0, P16, 1024, None)
    with pytest.raises(ValueError, match="aligned"):
        call("mpn_jpeg_forward", P16, 1024, odd, 1, P16, 1024, None)
    with pytest.raises(_lib.MpnError, match="coefficients"):
        call("mpn_jpeg_forward", P16, 1024, P16, 1, P16, 64, None)
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_entropy_encode", P16, 1024, P16, 1, P16, 1024, None, P16, 1024, None)
    with pytest.raises(ValueError, match="B must"):
        call("mpn_jpeg_entropy_encode", P16, 1024, P16, 70000, P16, 1024, P16, P16, 1024, None)
    with pytest.raises(ValueError, match="aligned"):
        call("mpn_jpeg_entropy_encode", P16, 1024, P16, 1, odd, 1024, P16, P16, 1024, None)
    with pytest.raises(_lib.MpnError, match="workspace"):
        call("mpn_jpeg_entropy_encode", P16, 1024, P16, 1, P16, 1024, P16, P16, 0, None)


def test_argument_errors_need_no_device():
    from multiposenet_amd.inference import JpegBatchEncoder, encode_jpegs
    from multiposenet_amd.inference.detector import Detector, check_annotate
    assert JpegBatchEncoder is J.JpegBatchEncoder and encode_jpegs is J.encode_jpegs
    for bad, match in (([], "empty"), ([np.zeros((4, 4, 4), np.uint8)], "uint8"), ([np.zeros((4, 4, 3), np.float32)], "uint8")):
        with pytest.raises(ValueError, match=match):
            encode_jpegs(bad)
    with pytest.raises(ValueError, match="subsampling"):
        encode_jpegs([np.zeros((4, 4, 3), np.uint8)], subsampling='4:4:0')
    with pytest.raises(ValueError, match="width|side"):
        J.jpeg_headers(0, 8, '4:2:0', J.quality_tables(75))
    assert check_annotate(False, 75, '4:2:0') is None and check_annotate(True, 75, '4:2:0') is None
    assert check_annotate('jpeg', 90, '4:2:2') == (90, '4:2:2')
    for args, match in ((('png', 75, '4:2:0'), "annotate"), (('jpeg', 0, '4:2:0'), "quality"), (('jpeg', 75, 2), "subsampling")):
        with pytest.raises(ValueError, match=match):
            check_annotate(*args)
    det = object.__new__(Detector)
    with pytest.raises(ValueError, match="annotate"):
        det.predict_batch(np.zeros((1, 128, 128, 3), np.uint8), annotate='jpg')
