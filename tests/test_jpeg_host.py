"""CPU: the host stage of the JPEG decode (marker scan, Huffman decode) and the numpy restatement of its device stage, held
byte for byte to the pixels Pillow decoded (tests/golden/jpeg_goldens.npz); classification, damaged streams, threads and
every argument check, none of which needs a device."""
import ctypes
import io
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_decode_ref as R
from jpeg_cases import CASES, UNSUPPORTED
from multiposenet_amd import _lib
from multiposenet_amd.inference import jpeg as J

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_goldens.npz")


def goldens():
    with np.load(GOLDEN) as z:
        assert [str(n) for n in z["names"]] == [c[0] for c in CASES]
        return {c[0]: (z[f"{c[0]}/jpeg"].tobytes(), z[f"{c[0]}/pixels"]) for c in CASES}


def supported_cases():
    return [c for c in CASES if c[4] not in UNSUPPORTED]


def test_case_table_covers_what_the_decoder_claims():
    cases = supported_cases()
    assert {(1, 1), (8, 8), (5, 7), (17, 17), (16, 33), (37, 53), (48, 64), (120, 160)} <= {c[2] for c in cases}
    assert {'444', '422', '420', 'L'} == {c[4] for c in cases}
    assert {30, 75, 95, 100} <= {c[5] for c in cases}
    assert {'smooth', 'noise', 'flat', 'checker'} == {c[3] for c in cases}
    for key in ('optimize', 'restart_marker_blocks', 'restart_marker_rows'):
        assert any(key in c[6] for c in cases), key
    assert {c[4] for c in CASES if c[4] in UNSUPPORTED} == {'progressive', 'cmyk'}
    assert os.path.getsize(GOLDEN) <= 444 * 1024


def test_host_stage_and_restatement_equal_every_golden_exactly():
    g = goldens()
    for name, *_ in supported_cases():
        data, want = g[name]
        c = J.entropy_decode(data)
        assert c.shape == want.shape and c.coefs.dtype == np.int16
        got = R.decode_coefficients(c)
        assert got.dtype == np.uint8 and got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_checkerboard_goldens_overshoot_the_range():
    """A saturated checkerboard, coarsely quantised, drives the inverse DCT outside [0, 255]: the range limit is exercised by
    the goldens, not just present."""
    g = goldens()
    lo, hi = 0, 255
    for name, _, _, content, *_ in supported_cases():
        if content != 'checker':
            continue
        coefs, quant = J.entropy_decode(g[name][0]).planes()[0]
        x = coefs.astype(np.int64) * quant.astype(np.int64)
        ws = np.swapaxes(R._idct_1d(np.swapaxes(x, 2, 3), 11), 2, 3)
        px = R._idct_1d(ws, 18) + 128
        lo, hi = min(lo, int(px.min())), max(hi, int(px.max()))
    assert lo < 0 and hi > 255, (lo, hi)


def test_goldens_equal_live_pillow():
    pytest.importorskip("PIL.Image")
    import make_jpeg_goldens as M
    g = goldens()
    for name, seed, shape, content, mode, quality, extra in CASES:
        data, want = g[name]
        np.testing.assert_array_equal(M.decode(data), want, err_msg=name)          # the decoder has not drifted
        live = M.encode(seed, shape, content, mode, quality, extra)
        np.testing.assert_array_equal(R.decode_coefficients(J.entropy_decode(live)) if mode not in UNSUPPORTED else M.decode(live),
                                      M.decode(live), err_msg=name + " (re-encoded)")


def test_restatement_equals_live_pillow_on_a_seeded_sweep():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(77)
    for k in range(60):
        h, w = (int(v) for v in rng.randint(1, 70, 2))
        src = rng.randint(0, 256, (h, w, 3)).astype(np.uint8) if k % 2 else np.full((h, w, 3), 255 * (k % 4 == 0), np.uint8)
        if k % 6 == 2:
            src[::2, 1::2] = 255 - src[::2, 1::2]
        buf = io.BytesIO()
        Image.fromarray(src).save(buf, "JPEG", quality=int(rng.randint(5, 101)), subsampling=int(rng.randint(0, 3)),
                                  optimize=bool(k % 3 == 0), restart_marker_blocks=int(rng.randint(0, 4)))
        data = buf.getvalue()
        np.testing.assert_array_equal(R.decode_coefficients(J.entropy_decode(data)), J.pillow_decode(data), err_msg=f"{k}: {h}x{w}")


def test_classification():
    g = goldens()
    for name, seed, shape, content, mode, quality, extra in CASES:
        info = J.jpeg_info(g[name][0])
        assert (info['height'], info['width']) == shape, name
        if mode in UNSUPPORTED:
            assert not info['supported'] and info['reason'] == UNSUPPORTED[mode], (name, info)
            with pytest.raises(ValueError, match="not supported"):
                J.entropy_decode(g[name][0])
            assert isinstance(J.prepare(g[name][0]), np.ndarray)                    # the fallback: Pillow's pixels
            continue
        assert info['supported'] and info['reason'] == 'supported', (name, info)
        want = {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'L': (1, 1)}[mode]
        assert info['sampling'] == want and info['components'] == (1 if mode == 'L' else 3), (name, info)
        hs, vs = want
        mcu_x, mcu_y = -(-shape[1] // (8 * hs)), -(-shape[0] // (8 * vs))
        blocks = [(mcu_y * vs, mcu_x * hs)] + ([(mcu_y, mcu_x)] * 2 if mode != 'L' else [])
        assert info['blocks'] == blocks and info['total_blocks'] == sum(a * b for a, b in blocks)
        assert info['coef_bytes'] == info['total_blocks'] * 128
        assert (info['restart_interval'] > 0) == any(k.startswith('restart') for k in extra), name
    with pytest.raises(ValueError, match="BAD_DATA"):
        J.jpeg_info(b"not a jpeg at all")
    with pytest.raises(ValueError, match="bytes"):
        J.jpeg_info(np.zeros(4, np.uint8))


def _patched(data, marker, edit):
    """The stream with the payload of its first `marker` segment edited in place."""
    b = bytearray(data)
    at = data.index(bytes([0xFF, marker]))
    edit(b, at + 4)
    return bytes(b)


def test_classification_of_hand_patched_headers():
    """Streams Pillow does not write, made from a golden by editing header bytes: each is classified, none misdecoded."""
    data = goldens()["37x53_444"][0]

    def reason(d):
        return J.jpeg_info(d)['reason']

    assert reason(_patched(data, 0xC0, lambda b, p: b.__setitem__(p, 12))) == 'precision'
    assert reason(_patched(data, 0xC0, lambda b, p: b.__setitem__(p + 7, 0x12))) == 'sampling'        # 4:4:0
    assert reason(_patched(data, 0xC0, lambda b, p: b.__setitem__(p + 7, 0x41))) == 'sampling'        # 4:1:1
    assert reason(data.replace(b"\xff\xc0", b"\xff\xc9", 1)) == 'arithmetic'
    assert reason(data.replace(b"\xff\xc0", b"\xff\xc3", 1)) == 'frame_type'
    rgb_ids = _patched(data, 0xC0, lambda b, p: (b.__setitem__(p + 6, ord('R')), b.__setitem__(p + 9, ord('G')), b.__setitem__(p + 12, ord('B'))))
    rgb_ids = _patched(rgb_ids, 0xDA, lambda b, p: (b.__setitem__(p + 1, ord('R')), b.__setitem__(p + 3, ord('G')), b.__setitem__(p + 5, ord('B'))))
    assert reason(rgb_ids) == 'supported'                                                             # JFIF says YCbCr
    assert reason(rgb_ids.replace(b"JFIF\0", b"JFXX\0", 1)) == 'colorspace'
    adobe0 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    assert reason(data[:2] + adobe0 + data[2:]) == 'colorspace'
    assert reason(data[:2] + adobe0[:-1] + b"\x01" + data[2:]) == 'supported'


def _variants(data, rng, count):
    out = [data[:n] for n in sorted(set(int(v) for v in rng.randint(0, len(data), count)))]
    for _ in range(count):
        b = bytearray(data)
        b[int(rng.randint(0, len(b)))] = int(rng.randint(0, 256))
        out.append(bytes(b))
    return out


def test_damaged_streams_return_an_error_or_a_complete_output():
    g = goldens()
    rng = np.random.RandomState(4242)
    lib = _lib.lib()
    seen = {'error': 0, 'complete': 0}
    for name in ("17x17_420", "16x33_422_opt", "37x53_422_rst_blocks", "48x64_gray_rst", "120x160_420"):
        data = g[name][0]
        for bad in _variants(data, rng, 40):
            h = J._Header()
            rc = lib.mpn_jpeg_info(bad, len(bad), ctypes.byref(h))
            if rc != 0 or not h.supported:
                seen['error'] += 1
                continue
            # guard words behind the buffer: nothing is written past coef_bytes
            coefs = np.full(h.total_blocks * 64 + 64, 0x5A5A, np.int16)
            desc = np.zeros(1, J.DESC)
            rc = lib.mpn_jpeg_entropy_decode(bad, len(bad), coefs.ctypes.data_as(ctypes.c_void_p), h.total_blocks * 128,
                                             desc.ctypes.data_as(ctypes.c_void_p))
            assert (coefs[-64:] == 0x5A5A).all()
            if rc != 0:
                assert rc == -7 and _lib.last_error()
                seen['error'] += 1
                continue
            seen['complete'] += 1
            assert (desc[0]['height'], desc[0]['width']) == (h.height, h.width)
            c = J.Coefficients((h.height, h.width, 3), coefs[:-64].reshape(-1, 64), desc)
            assert R.decode_coefficients(c).shape == (h.height, h.width, 3)
    assert seen['error'] > 50 and seen['complete'] > 50, seen


def test_host_entry_points_reproduce_the_frozen_verdicts():
    """Every host entry point answers the corpus of make_jpeg_host_verdicts.py (87 files, 501 inputs each: the file, 400
    replacements in its headers, 60 anywhere, 40 prefixes) as tests/golden/jpeg_host_verdicts.npz recorded it before the
    one-scan and the multi-scan parser became one: return codes, verdicts, and a CRC32 of every output a call defines.
    The corpus must keep its point: the inputs on which the two policies part ("JPEG host front end") are 16.7 %
    of it as recorded, and at least 10 % are asked for. (The slowest host test: 43 587 inputs through five calls each,
    about 10 s on 8 cores; the counts are what keeps 200+ header mutations per file.)"""
    import make_jpeg_host_verdicts as M
    with np.load(os.path.join(os.path.dirname(GOLDEN), "jpeg_host_verdicts.npz")) as z:
        want = {k: z[k] for k in ('names', 'rc', 'verdict', 'crc')}
    got = M.run()
    names = [str(n) for n in want['names']]
    assert [str(n) for n in got['names']] == names and want['crc'].shape == (len(names), M.PER_FILE)

    def where(key, labels):
        """The first inputs whose `key` is not the recorded one: file, mutation index, entry point, recorded -> now."""
        out = []
        for at in np.argwhere(got[key] != want[key])[:8]:
            f, m = int(at[0]), int(at[1])
            which = labels[at[2]] if len(at) == 3 else "outputs of " + ", ".join(e for e, r in zip(M.ENTRY_POINTS, got['rc'][f, m]) if r == 0)
            out.append(f"{names[f]}, mutation {m}, {which}: {want[key][tuple(at)]} -> {got[key][tuple(at)]}")
        return "\n".join(out)

    assert (got['rc'] == want['rc']).all(), where('rc', M.ENTRY_POINTS)
    assert (got['verdict'] == want['verdict']).all(), where('verdict', M.VERDICTS)
    assert (got['crc'] == want['crc']).all(), where('crc', None)
    share = M.differ(want['rc'], want['verdict']).mean()
    assert share >= 0.10, share


def test_eight_threads_equal_the_serial_result():
    g = goldens()
    names = [c[0] for c in supported_cases()] * 8
    serial = [J.entropy_decode(g[n][0]) for n in names]
    with ThreadPoolExecutor(max_workers=8) as ex:
        threaded = list(ex.map(lambda n: J.entropy_decode(g[n][0]), names))
    for a, b in zip(serial, threaded):
        np.testing.assert_array_equal(a.coefs, b.coefs)
        assert a.desc.tobytes() == b.desc.tobytes() and a.shape == b.shape


def test_entry_points_validate_before_any_hip_call():
    lib = _lib.lib()
    call = _lib.call
    data = goldens()["8x8_444"][0]
    P16 = ctypes.c_void_p(4096)
    h = J._Header()
    coefs = np.zeros((3, 64), np.int16)
    desc = np.zeros(1, J.DESC)
    cp, dp = coefs.ctypes.data_as(ctypes.c_void_p), desc.ctypes.data_as(ctypes.c_void_p)
    assert lib.mpn_jpeg_desc_bytes() == J.DESC_BYTES == J.DESC.itemsize == 512
    assert ctypes.sizeof(J._Header) == 72
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_info", None, 10, ctypes.byref(h))
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_info", data, len(data), None)
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_entropy_decode", data, len(data), None, 384, dp)
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_entropy_decode", data, len(data), cp, 384, None)
    with pytest.raises(_lib.MpnError, match="coef_bytes"):
        call("mpn_jpeg_entropy_decode", data, len(data), cp, 383, dp)
    call("mpn_jpeg_entropy_decode", data, len(data), cp, 384, dp)
    assert lib.mpn_jpeg_decode_workspace_bytes(2, 100) == 6400 and lib.mpn_jpeg_decode_workspace_bytes(0, 100) == 0
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_decode", None, 1024, P16, 1, P16, 1024, P16, 1024, None)
    with pytest.raises(ValueError, match="B must"):
        call("mpn_jpeg_decode", P16, 1024, P16, 0, P16, 1024, P16, 1024, None)
    with pytest.raises(ValueError, match="aligned"):
        call("mpn_jpeg_decode", P16, 1024, ctypes.c_void_p(4100), 1, P16, 1024, P16, 1024, None)
    with pytest.raises(_lib.MpnError, match="workspace"):
        call("mpn_jpeg_decode", P16, 1024, P16, 1, P16, 1024, P16, 0, None)


def test_batch_plan_is_host_arithmetic():
    g = goldens()
    a, b = J.entropy_decode(g["17x17_420"][0]), J.entropy_decode(g["8x8_444"][0])
    px = np.zeros((5, 7, 3), np.uint8)
    jp, pix, lay = J.JpegBatchDecoder.plan([a, px, b], [0, 1024, 2048])
    assert jp == [0, 2] and pix == [1]
    assert lay['coef_base'] == 2 * 512 and lay['coef_at'] == [0, a.coefs.nbytes] and lay['coef_bytes'] == a.coefs.nbytes + b.coefs.nbytes
    assert lay['work_at'] == [0, a.coefs.shape[0] * 64] and lay['work_bytes'] == (a.coefs.shape[0] + 3) * 64
    assert lay['pix_at'] == [lay['coef_base'] + lay['coef_bytes']] and lay['stage_bytes'] == lay['pix_at'][0] + 112
    with pytest.raises(ValueError, match="multiple of 16"):
        J.JpegBatchDecoder.plan([a], [8])
    with pytest.raises(ValueError, match="uint8"):
        J.JpegBatchDecoder.plan([np.zeros((5, 7, 3), np.float32)], [0])


def test_predict_jpegs_argument_errors_need_no_device():
    from multiposenet_amd.inference.detector import Detector
    det = object.__new__(Detector)
    good = goldens()["48x64_420_flat"][0]
    for bad, match in (([], "empty"), ([np.zeros((4, 4, 3), np.uint8)], "bytes"), (good, "list"), ([b"junk"], "BAD_DATA")):
        with pytest.raises(ValueError, match=match):
            det.predict_jpegs(bad)
    with pytest.raises(ValueError, match="size"):
        det.predict_jpegs([good], size=(100, 100))


def test_pipelines_reject_an_unknown_decode_mode():
    from multiposenet_amd.detector.input_pipeline import keypoints_detector_pipeline as kp
    from multiposenet_amd.detector.input_pipeline import person_detector_pipeline as pd
    assert kp.DECODE_MODES == pd.DECODE_MODES == ('host', 'device')
    with pytest.raises(ValueError, match="decode"):
        kp.check_decode_mode('gpu')
    assert pd.check_decode_mode('device') == 'device'
