"""CPU: the multi-scan host stage of the JPEG decode (mpn_jpeg_scans_info / mpn_jpeg_scans_decode: progressive files, Adobe
CMYK) and the numpy restatement of the device stage over its coefficients, held byte for byte to the pixels Pillow decoded
(tests/golden/jpeg_progressive_goldens.npz): zero tolerance. Classification and routes, damaged files, scan scripts the
standard forbids, threads and argument checks, none of which needs a device."""
import ctypes
import io
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_progressive_ref as P
from jpeg_cases import CASES as BASELINE_CASES, UNSUPPORTED
from jpeg_progressive_cases import CASES, DAMAGED, DAMAGED_FROM, scans
from multiposenet_amd import _lib
from multiposenet_amd.inference import jpeg as J
from test_jpeg_host import goldens as baseline_goldens


def test_case_table_covers_what_the_stage_claims():
    assert {(1, 1), (8, 8), (17, 17), (37, 53), (120, 160)} == {c[2] for c in CASES}
    assert {'noise', 'smooth', 'checker', 'flat'} == {c[3] for c in CASES}
    assert {'p444', 'p422', 'p420', 'pL', 'cmyk', 'pcmyk'} == {c[4] for c in CASES}
    for mode in ('p444', 'p422', 'p420', 'pL'):
        assert {30, 75, 95} <= {c[5] for c in CASES if c[4] == mode}, mode
    progressive = [c for c in CASES if c[4] != 'cmyk']
    for c in progressive:                                   # every progressive case both ways
        twin = c[0][:-4] if c[0].endswith("_opt") else c[0] + "_opt"
        assert any(o[0] == twin and o[1:6] == c[1:6] and o[6]['optimize'] != c[6]['optimize'] for o in progressive), c[0]
    for key in ('restart_marker_blocks', 'restart_marker_rows'):
        assert any(key in c[6] for c in progressive), key
    for size in ((17, 17), (37, 53)):
        assert {'cmyk', 'pcmyk'} <= {c[4] for c in CASES if c[2] == size}
    g = P.goldens()
    # the restart intervals divide neither the MCU row nor a single-component scan's block row
    for name, _, (h, w), _, mode, _, extra in CASES:
        r = extra.get('restart_marker_blocks')
        if r and mode == 'p420':
            assert (-(-w // 16)) % r and (-(-w // 8)) % r, name
    assert len(scans(g[DAMAGED_FROM][0])) == sum(d[2] == 'cut' for d in DAMAGED) == 10
    assert any(s[0] > 0 and s[2] > 0 for s in scans(g[DAMAGED_FROM][0]))     # it has AC refinement scans
    assert os.path.getsize(P.GOLDEN) <= 1024 * 1024 and len(P.versions()) == 2


def test_classification_and_routes():
    g = P.goldens()
    for name, _, shape, _, mode, _, extra in CASES:
        data = g[name][0]
        info = J.jpeg_info(data)                            # the one-scan stage's verdict has not changed
        assert not info['supported'] and info['reason'] == ('components' if mode == 'cmyk' else 'progressive'), (name, info)
        with pytest.raises(ValueError, match="not supported"):
            J.entropy_decode(data)
        with pytest.raises(ValueError, match="not supported"):
            J.scan_prepare(data)
        assert J.jpeg_support(data) == 'host-entropy', name
        s = J.scans_info(data)
        assert (s['height'], s['width']) == shape and s['reason'] == 'supported' and s['progressive'] == (mode != 'cmyk'), (name, s)
        ncomp = {'pL': 1, 'cmyk': 4, 'pcmyk': 4}.get(mode, 3)
        hs, vs = {'p422': (2, 1), 'p420': (2, 2)}.get(mode, (1, 1))
        mcu_x, mcu_y = -(-shape[1] // (8 * hs)), -(-shape[0] // (8 * vs))
        blocks = [(mcu_y * vs, mcu_x * hs)] + [(mcu_y, mcu_x)] * (ncomp - 1)
        assert s['components'] == ncomp and s['sampling'] == (hs, vs) and s['blocks'] == blocks, (name, s)
        assert s['total_blocks'] == sum(a * b for a, b in blocks) and s['coef_bytes'] == s['total_blocks'] * 128
    b = baseline_goldens()
    for name, *_, mode, _, _ in BASELINE_CASES:
        assert J.jpeg_support(b[name][0]) == ('host-entropy' if mode in UNSUPPORTED else 'device'), name
    with pytest.raises(ValueError, match="BAD_DATA"):
        J.jpeg_support(b"not a jpeg at all")


def _with_adobe_transform(data, transform):
    at = data.index(b"\xff\xeeAdobe"[:2] + b"\x00\x0eAdobe")
    return data[:at + 15] + bytes([transform]) + data[at + 16:]


def test_streams_that_stay_with_pillow():
    g, b = P.goldens(), baseline_goldens()
    cmyk, prog = g["17x17_cmyk"][0], g["17x17_p444_checker"][0]
    assert J.jpeg_support(_with_adobe_transform(cmyk, 2)) == 'pillow'                      # YCCK
    assert J.scans_info(_with_adobe_transform(cmyk, 2))['reason'] == 'colorspace'
    at = cmyk.index(b"\xff\xee")
    assert J.jpeg_support(cmyk[:at] + cmyk[at + 16:]) == 'pillow'                            # four components, no Adobe marker
    sof = cmyk.index(b"\xff\xc0")
    assert J.jpeg_support(cmyk[:sof + 11] + b"\x22" + cmyk[sof + 12:]) == 'pillow'           # sampled CMYK
    sof = prog.index(b"\xff\xc2")
    assert J.scans_info(prog[:sof + 11] + b"\x12" + prog[sof + 12:])['reason'] == 'sampling'  # 4:4:0
    assert J.scans_info(prog[:sof + 4] + b"\x0c" + prog[sof + 5:])['reason'] == 'precision'
    assert J.scans_info(prog.replace(b"\xff\xc2", b"\xff\xca", 1))['reason'] == 'arithmetic'
    with pytest.raises(ValueError, match="not supported"):
        J.scans_decode(_with_adobe_transform(cmyk, 2))
    assert isinstance(J.prepare(_with_adobe_transform(cmyk, 2), extended=True), np.ndarray)
    assert J.jpeg_support(b["17x17_420"][0]) == 'device'


def test_host_stage_and_restatement_equal_every_golden_exactly():
    g = P.goldens()
    for name, *_ in CASES:
        data, want = g[name]
        c = J.scans_decode(data)
        assert c.shape == want.shape and c.coefs.dtype == np.int16 and len(c.planes()) == int(c.desc[0]['components'])
        got = P.decode_coefficients(c)
        assert got.dtype == np.uint8 and got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_refinement_scans_carry_correction_bits_and_flat_images_long_runs():
    """The goldens reach what they are there for: at quality 95 most coefficients of a block are non-zero before the
    refinement scans (correction bits), and the flat image has no AC coefficient at all (end-of-band runs over many blocks)."""
    g = P.goldens()
    busy = J.scans_decode(g["120x160_p444"][0]).coefs
    assert (np.abs(busy[:, 1:]) >= 2).mean() > 0.5
    flat = J.scans_decode(g["120x160_p420_flat"][0]).coefs
    assert flat.shape[0] == 480 and not flat[:, 1:].any() and flat[:, 0].any()


def test_the_sequential_files_decode_to_the_one_scan_stages_coefficients():
    b = baseline_goldens()
    for name, *_, mode, _, _ in BASELINE_CASES:
        if mode in UNSUPPORTED:
            continue
        one, many = J.entropy_decode(b[name][0]), J.scans_decode(b[name][0])
        np.testing.assert_array_equal(one.coefs, many.coefs, err_msg=name)
        assert one.desc.tobytes() == many.desc.tobytes() and one.shape == many.shape, name


def test_prepare_returns_coefficients_behind_its_option():
    g = P.goldens()
    for name, *_ in CASES:
        data = g[name][0]
        for entropy in J.ENTROPY_MODES:
            entry = J.prepare(data, entropy, extended=True)
            assert isinstance(entry, J.Coefficients) and entry.shape == g[name][1].shape, (name, entropy)
    assert isinstance(J.prepare(g["17x17_pcmyk"][0]), np.ndarray)          # the default: Pillow's pixels, as before
    b = baseline_goldens()
    assert isinstance(J.prepare(b["17x17_420"][0], 'device', extended=True), J.Scan)
    assert isinstance(J.prepare(b["17x17_420"][0], 'host', extended=True), J.Coefficients)


def _decode_guarded(data):
    """mpn_jpeg_scans_decode with guard words behind the buffer -> (rc, coefficients, desc); asserts the guard."""
    lib = _lib.lib()
    h = J._ScansHeader()
    if lib.mpn_jpeg_scans_info(data, len(data), ctypes.byref(h)) != 0 or h.route == 2:
        return None
    coefs = np.full(h.total_blocks * 64 + 64, 0x5A5A, np.int16)
    desc = np.zeros(1, J.DESC)
    rc = lib.mpn_jpeg_scans_decode(data, len(data), coefs.ctypes.data_as(ctypes.c_void_p), h.total_blocks * 128,
                                   desc.ctypes.data_as(ctypes.c_void_p))
    assert (coefs[-64:] == 0x5A5A).all(), "written past coef_bytes"
    return rc, J.Coefficients((h.height, h.width, 3), coefs[:-64].reshape(-1, 64), desc)


def test_damaged_goldens_raise_value_error():
    for name, data in P.damaged().items():
        with pytest.raises(ValueError, match="BAD_DATA"):
            J.scans_decode(data)
        rc, _ = _decode_guarded(data)
        assert rc == -7 and _lib.last_error(), name


def test_corrupted_streams_return_an_error_or_a_complete_output():
    g = P.goldens()
    rng = np.random.RandomState(777)
    seen = {'error': 0, 'complete': 0}
    for name in ("17x17_p420", "37x53_p420_rst3_opt", "37x53_p422_rst_rows", "17x17_pcmyk_rst2", "37x53_cmyk_opt_rst", "37x53_pL_rst3"):
        data = g[name][0]
        variants = [data[:n] for n in sorted(set(int(v) for v in rng.randint(0, len(data), 25)))]
        for _ in range(40):
            bad = bytearray(data)
            bad[int(rng.randint(0, len(bad)))] = int(rng.randint(0, 256))
            variants.append(bytes(bad))
        for bad in variants:
            res = _decode_guarded(bad)
            if res is None or res[0] != 0:
                assert res is None or res[0] in (-6, -7)
                seen['error'] += 1
                continue
            seen['complete'] += 1
            assert P.decode_coefficients(res[1]).shape == res[1].shape
    assert seen['error'] > 100 and seen['complete'] > 30, seen


def _patched_scan(data, index, ss=None, se=None, ahal=None):
    start = scans(data)[index][5]
    b = bytearray(data)
    for off, v in ((3, ss), (2, se), (1, ahal)):
        if v is not None:
            b[start - off] = v
    return bytes(b)


def test_scan_scripts_the_standard_forbids_are_refused():
    data = P.goldens()["37x53_p420_checker"][0]
    sc = scans(data)
    assert sc[0][:4] == (0, 0, 0, 1) and sc[1][0] > 0 and sc[1][2] == 0         # DC first, then an AC first scan
    refused = {
        "bit position 14": _patched_scan(data, 0, ahal=0x0E),
        "band past 63": _patched_scan(data, 1, se=64),
        "band upside down": _patched_scan(data, 1, ss=9, se=3),
        "refines a band never started": _patched_scan(data, 1, ahal=0x32),
        "refinement that skips a bit": _patched_scan(data, len(sc) - 1, ahal=0x20),
        "AC band with the DC": _patched_scan(data, 1, ss=0),
        "a band coded twice": data[:sc[1][5] - 10] + data[sc[1][5] - 10:sc[1][6]] * 2 + data[sc[1][6]:],
    }
    assert sc[1][4] == 1 and data[sc[1][5] - 10:sc[1][5] - 8] == b"\xff\xda"                    # (the doubled part starts at that scan's SOS)
    for what, bad in refused.items():
        with pytest.raises(ValueError, match="BAD_DATA"):
            J.scans_decode(bad)
    missing = data[:sc[-1][5] - 10] + b"\xff\xd9"                                # the last scan (one component) is cut away
    assert sc[-1][4] == 1 and J.jpeg_support(missing) == 'host-entropy'
    with pytest.raises(ValueError, match="scans are missing"):
        J.scans_decode(missing)


def test_eight_threads_equal_the_serial_result():
    g = P.goldens()
    names = [c[0] for c in CASES] * 4
    serial = [J.scans_decode(g[n][0]) for n in names]
    with ThreadPoolExecutor(max_workers=8) as ex:
        threaded = list(ex.map(lambda n: J.scans_decode(g[n][0]), names))
    for a, b in zip(serial, threaded):
        np.testing.assert_array_equal(a.coefs, b.coefs)
        assert a.desc.tobytes() == b.desc.tobytes() and a.shape == b.shape


def test_entry_points_validate_their_arguments():
    call = _lib.call
    data = P.goldens()["8x8_p444"][0]
    h = J._ScansHeader()
    coefs = np.zeros((3, 64), np.int16)
    desc = np.zeros(1, J.DESC)
    cp, dp = coefs.ctypes.data_as(ctypes.c_void_p), desc.ctypes.data_as(ctypes.c_void_p)
    assert ctypes.sizeof(J._ScansHeader) == 80
    # the descriptor kept its size and every field it had; the fourth component sits in what was reserved
    assert J.DESC.itemsize == 512 and J.DESC.fields['blocks_h'][1] == 60 and J.DESC.fields['blocks_w3'][1] == 72
    assert J.DESC.fields['quant3'][1] == 80 and J.DESC.fields['quant'][1] == 128
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_scans_info", None, 10, ctypes.byref(h))
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_scans_info", data, len(data), None)
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_scans_decode", data, len(data), None, 384, dp)
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_scans_decode", data, len(data), cp, 384, None)
    with pytest.raises(_lib.MpnError, match="coef_bytes"):
        call("mpn_jpeg_scans_decode", data, len(data), cp, 383, dp)
    call("mpn_jpeg_scans_decode", data, len(data), cp, 384, dp)
    four = J.scans_decode(P.goldens()["17x17_cmyk"][0]).desc[0]
    assert int(four['components']) == 4 and (int(four['blocks_h3']), int(four['blocks_w3'])) == (3, 3) and int(four['quant3']) == 0


def test_goldens_equal_live_pillow_and_a_seeded_sweep():
    Image = pytest.importorskip("PIL.Image")
    import make_jpeg_progressive_goldens as M
    g = P.goldens()
    for name, seed, shape, content, mode, quality, extra in CASES:
        np.testing.assert_array_equal(M.decode(g[name][0]), g[name][1], err_msg=name)     # the decoder has not drifted
        live = M.encode(seed, shape, content, mode, quality, extra)
        np.testing.assert_array_equal(P.decode_coefficients(J.scans_decode(live)), M.decode(live), err_msg=name + " (re-encoded)")
    rng = np.random.RandomState(78)
    for k in range(40):
        h, w = (int(v) for v in rng.randint(1, 70, 2))
        src = rng.randint(0, 256, (h, w, 3)).astype(np.uint8) if k % 2 else np.full((h, w, 3), 255 * (k % 4 == 0), np.uint8)
        if k % 6 == 2:
            src[::2, 1::2] = 255 - src[::2, 1::2]
        buf = io.BytesIO()
        kw = {'quality': int(rng.randint(5, 101)), 'restart_marker_blocks': int(rng.randint(0, 4)), 'progressive': bool(k % 5)}
        if k % 4 == 3:
            Image.fromarray(src).convert("CMYK").save(buf, "JPEG", **kw)
        else:
            Image.fromarray(src).save(buf, "JPEG", subsampling=int(rng.randint(0, 3)), **dict(kw, progressive=True))
        data = buf.getvalue()
        np.testing.assert_array_equal(P.decode_coefficients(J.scans_decode(data)), J.pillow_decode(data), err_msg=f"{k}: {h}x{w}")
