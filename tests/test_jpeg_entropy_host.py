"""CPU: the header stage of the device's JPEG entropy decode (mpn_jpeg_scan_prepare), the argument checks of
mpn_jpeg_entropy_decode_device, and the numpy / Python restatement of its scheme (tests/jpeg_entropy_ref.py) held to the host
`entropy_decode`, coefficient for coefficient, on every supported golden and on the 128-shift phase sweep."""
import ctypes

import numpy as np
import pytest

import jpeg_entropy_ref as E
from jpeg_cases import CASES, UNSUPPORTED
from multiposenet_amd import _lib
from multiposenet_amd.inference import jpeg as J
from test_jpeg_host import goldens, supported_cases

PHASE_FILES = ("48x64_444_q100", "48x64_420_rst_rows")


def phase_sweep(name):
    """The file with a COM segment of 2..129 bytes in front of its SOS: the scan's phase against the grid takes all 128 values."""
    data = goldens()[name][0]
    return [E.with_comment(data, length) for length in range(2, 130)]


def test_restatement_equals_the_host_stage_on_every_supported_golden():
    g = goldens()
    for name, *_ in supported_cases():
        want = J.entropy_decode(g[name][0]).coefs
        scan = E.Scan(g[name][0])
        np.testing.assert_array_equal(scan.decode(sweep=True), want, err_msg=name)
        assert scan.sweeps <= scan.nsub - scan.first + 1, name
        np.testing.assert_array_equal(scan.decode(sweep=False), want, err_msg=name + " (chain)")


def test_phase_sweep_every_shift_decodes_to_the_same_coefficients():
    g = goldens()
    for name in PHASE_FILES:
        data = g[name][0]
        want = J.entropy_decode(data).coefs
        files = phase_sweep(name)
        offsets = {E.parse(f)['scan_offset'] % 128 for f in files}
        assert offsets == set(range(128)), name
        if name == PHASE_FILES[0]:
            assert data.count(b"\xff\x00") > 20
        else:
            assert sum(data.count(bytes((0xFF, 0xD0 + k))) for k in range(8)) >= 2
        for f in files:                                         # the host decoder first: the same coefficients at every shift
            np.testing.assert_array_equal(J.entropy_decode(f).coefs, want)
        for f in files:
            np.testing.assert_array_equal(E.decode(f, sweep=False), want)
        # the plain sweep (guessed entries, re-decoding until nothing changes) re-decodes every subsequence several times
        # in Python: about 3 s per file, so it runs at four shifts here and on every golden above; the chain walk above
        # carries f_i across every boundary at every shift
        for f in files[::37]:
            np.testing.assert_array_equal(E.decode(f, sweep=True), want)


def test_scan_prepare_agrees_with_jpeg_info_on_all_cases():
    g = goldens()
    assert len(CASES) == 27
    lib = _lib.lib()
    for name, seed, shape, content, mode, quality, extra in CASES:
        data = g[name][0]
        info = J.jpeg_info(data)
        desc = np.zeros(1, J.SCAN_DESC)
        assert lib.mpn_jpeg_scan_prepare(data, len(data), desc.ctypes.data_as(ctypes.c_void_p)) == 0
        d = desc[0]
        assert bool(d['supported']) == info['supported'] and J.REASONS[int(d['reason'])] == info['reason'], name
        assert (int(d['height']), int(d['width']), int(d['components'])) == (info['height'], info['width'], info['components'])
        if mode in UNSUPPORTED:
            with pytest.raises(ValueError, match="not supported"):
                J.scan_prepare(data)
            assert isinstance(J.prepare(data, entropy='device'), np.ndarray)
            continue
        scan = J.prepare(data, entropy='device')
        assert isinstance(scan, J.Scan) and scan.shape == shape + (3,) and scan.data == data
        assert (int(d['h_samp']), int(d['v_samp'])) == info['sampling'] and int(d['restart_interval']) == info['restart_interval']
        assert [(int(d['blocks_h'][c]), int(d['blocks_w'][c])) for c in range(info['components'])] == info['blocks']
        assert int(d['total_blocks']) == info['total_blocks'] and int(d['nbytes']) == len(data)
        ref = E.parse(data)
        assert int(d['scan_offset']) == ref['scan_offset']
        host = J.entropy_decode(data).desc[0]
        np.testing.assert_array_equal(d['quant'], host['quant'])
        for c, (td, ta) in enumerate(ref['tables']):
            assert (int(d['dc_table'][c]), int(d['ac_table'][c])) == (td, ta)
            for cls, tid in ((0, td), (1, ta)):
                counts, symbols = ref['huff'][(cls, tid)]
                assert list(d['huff_bits'][cls][tid]) == counts and list(d['huff_vals'][cls][tid][:len(symbols)]) == symbols
    with pytest.raises(ValueError, match="BAD_DATA"):
        J.scan_prepare(b"not a jpeg at all")
    with pytest.raises(ValueError, match="entropy"):
        J.prepare(g["8x8_444"][0], entropy='gpu')


def test_scan_prepare_never_reads_the_scan():
    """Headers only: the descriptor of a file cut right behind its SOS header equals the whole file's but for nbytes."""
    data = goldens()["37x53_444"][0]
    whole = J.scan_prepare(data).desc.copy()
    cut = J.scan_prepare(data[:int(whole[0]['scan_offset'])]).desc
    whole[0]['nbytes'] = cut[0]['nbytes']
    assert whole.tobytes() == cut.tobytes()


def test_descriptor_and_record_sizes_are_the_library_s():
    lib = _lib.lib()
    assert lib.mpn_jpeg_scan_desc_bytes() == J.SCAN_DESC_BYTES == J.SCAN_DESC.itemsize == 2704
    assert J.ENTROPY_RECORD.itemsize == 16 and J.SCAN_DESC_BYTES % 16 == 0


def test_entry_points_validate_before_any_hip_call():
    lib = _lib.lib()
    call = _lib.call
    P = ctypes.c_void_p(4096)
    desc = np.zeros(1, J.SCAN_DESC)
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_scan_prepare", None, 10, desc.ctypes.data_as(ctypes.c_void_p))
    with pytest.raises(ValueError, match="null"):
        call("mpn_jpeg_scan_prepare", b"abcd", 4, None)
    ws = lib.mpn_jpeg_entropy_decode_device_workspace_bytes
    assert ws(0, 4096) == 0 and ws(1, 0) == 0 and ws(1, 1 << 31) == 0 and ws(70000, 4096) == 0
    assert ws(1, 4096) >= 32 * (4096 // 128) and ws(1, 4096) % 16 == 0 and ws(2, 1 << 20) > ws(1, 1 << 20) > ws(1, 4096)
    big = ws(1, 4096)
    args = lambda **k: [k.get('files', P), k.get('files_bytes', 4096), k.get('descs', P), k.get('B', 1), k.get('coefs', P),
                        k.get('coef_bytes', 1024), k.get('out', P), k.get('records', P), k.get('work', P), k.get('work_bytes', big),
                        k.get('max_passes', 4), None]
    for name in ('files', 'descs', 'coefs', 'out', 'records', 'work'):
        with pytest.raises(ValueError, match="null"):
            call("mpn_jpeg_entropy_decode_device", *args(**{name: None}))
    with pytest.raises(ValueError, match="B must"):
        call("mpn_jpeg_entropy_decode_device", *args(B=0))
    for passes in (0, 65):
        with pytest.raises(ValueError, match="max_passes"):
            call("mpn_jpeg_entropy_decode_device", *args(max_passes=passes))
    with pytest.raises(ValueError, match="aligned"):
        call("mpn_jpeg_entropy_decode_device", *args(records=ctypes.c_void_p(4104)))
    with pytest.raises(_lib.MpnError, match="files of"):
        call("mpn_jpeg_entropy_decode_device", *args(files_bytes=8))
    with pytest.raises(_lib.MpnError, match="workspace"):
        call("mpn_jpeg_entropy_decode_device", *args(work_bytes=big - 16))


def test_scan_batch_plan_is_host_arithmetic():
    g = goldens()
    a, b = J.scan_prepare(g["17x17_420"][0]), J.scan_prepare(g["8x8_444"][0])
    lay = J.JpegBatchDecoder.plan_scans([a, b], [0, 1024])
    r16 = lambda n: (n + 15) // 16 * 16
    assert lay['file_base'] == 2 * J.SCAN_DESC_BYTES and lay['file_at'] == [0, r16(len(a.data))]
    assert lay['files_bytes'] == r16(len(a.data)) + r16(len(b.data)) and lay['stage_bytes'] == lay['file_base'] + lay['files_bytes']
    assert lay['coef_at'] == [0, a.total_blocks * 128] and lay['work_at'] == [0, a.total_blocks * 64]
    with pytest.raises(ValueError, match="multiple of 16"):
        J.JpegBatchDecoder.plan_scans([a], [8])
