"""GPU: mpn_jpeg_forward and mpn_jpeg_entropy_encode, each against a yardstick of its own, then `JpegBatchEncoder`,
`encode_jpegs` and the `annotate='jpeg'` paths of the Detector against the files Pillow wrote
(tests/golden/jpeg_encode_goldens.npz). No tolerance anywhere: coefficients and bytes are equal or the test fails. Run it in a
process of its own under a time limit, e.g.

    timeout -k 10 600 python -m pytest -m gpu tests/test_jpeg_encode_gpu.py
"""
import numpy as np
import pytest
import torch

from jpeg_encode_cases import CASES
from multiposenet_amd import _lib
from multiposenet_amd.inference import jpeg as J
from test_jpeg_encode_host import goldens, scan_of

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7
_DECODED = {}


def decoded(name):
    """`entropy_decode` of a golden file: the yardstick of the forward kernel, the input of the entropy coder. Shared."""
    if name not in _DECODED:
        _DECODED[name] = J.entropy_decode(goldens()[name][1])
    return _DECODED[name]


def _case(name):
    return next(c for c in CASES if c[0] == name)


def _round16(n):
    return (n + 15) // 16 * 16


def _place(sizes, gap, first=16):
    """Byte offsets (multiples of 16) of ranges of `sizes` bytes with at least `gap` untouched bytes around each."""
    offsets, at = [], _round16(first + gap)
    for n in sizes:
        offsets.append(at)
        at = _round16(at + n + gap)
    return offsets, at + gap


def _descs(entries):
    """ENC_DESC records from dicts (the fields that matter to the call under test)."""
    d = np.zeros(len(entries), J.ENC_DESC)
    for i, e in enumerate(entries):
        for k, v in e.items():
            d[i][k] = v
    return d


def _device(array, cuda):
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)).to(cuda)


def _outside_untouched(host, ranges):
    outside = np.ones(host.size, bool)
    for at, n in ranges:
        outside[at:at + n] = False
    return bool((host[outside] == SENTINEL).all())


def _forward(cuda, names, gap=48):
    """mpn_jpeg_forward on the named goldens as ONE ragged batch: sentinel-filled coefficient buffer with gaps; asserts that
    every image's coefficients equal what the host decoder reads from Pillow's file and that nothing else was written."""
    g = goldens()
    pixels = [g[n][0] for n in names]
    wants = [decoded(n) for n in names]
    src_at, src_total = _place([p.size for p in pixels], gap)
    coef_at, coef_total = _place([w.coefs.nbytes for w in wants], gap)
    sources = np.full(src_total, SENTINEL, np.uint8)
    entries = []
    for n, p, w, sa, ca in zip(names, pixels, wants, src_at, coef_at):
        sources[sa:sa + p.size] = p.reshape(-1)
        d = w.desc[0]
        entries.append({'src_offset': sa, 'coef_offset': ca, 'width': p.shape[1], 'height': p.shape[0], 'channels': p.shape[2],
                        'h_samp': d['h_samp'], 'v_samp': d['v_samp'], 'quant': d['quant']})
    coefs = torch.full((coef_total,), SENTINEL, dtype=torch.uint8, device=cuda)
    dev_src, dev_desc = _device(sources, cuda), _device(_descs(entries), cuda)
    _lib.call("mpn_jpeg_forward", _lib.ptr(dev_src), dev_src.numel(), _lib.ptr(dev_desc), len(names), _lib.ptr(coefs), coefs.numel(),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    host = coefs.cpu().numpy()
    for n, w, ca in zip(names, wants, coef_at):
        got = host[ca:ca + w.coefs.nbytes].view(np.int16).reshape(w.coefs.shape)
        bad = np.argwhere(got != w.coefs)
        assert not len(bad), (n, len(bad), bad[:4].tolist(), got[tuple(bad[0])], w.coefs[tuple(bad[0])])
    assert _outside_untouched(host, [(ca, w.coefs.nbytes) for w, ca in zip(wants, coef_at)]), "bytes outside the planes were written"


def _entropy(cuda, items, capacities=None, gap=48):
    """mpn_jpeg_entropy_encode on [(coefs int16 [T, 64], width, height, h_samp, v_samp)] as one batch -> (records, scans or
    None per image). Asserts the sentinel everywhere outside the written streams."""
    lib = _lib.lib()
    caps = [int(c) for c in (capacities or [_round16(it[0].shape[0] * 64 * 4 + 256) for it in items])]
    coef_at, coef_total = _place([it[0].nbytes for it in items], gap)
    out_at, out_total = _place(caps, gap)
    shares = [lib.mpn_jpeg_entropy_encode_workspace_bytes(it[0].shape[0], c) for it, c in zip(items, caps)]
    assert all(s > 0 for s in shares)
    work_at, work_total = _place(shares, 0, first=0)
    coefs = np.full(coef_total, SENTINEL, np.uint8)
    entries = []
    for (c, w, h, hs, vs), ca, oa, wa, cap in zip(items, coef_at, out_at, work_at, caps):
        coefs[ca:ca + c.nbytes] = np.ascontiguousarray(c).view(np.uint8).reshape(-1)
        entries.append({'coef_offset': ca, 'out_offset': oa, 'capacity': cap, 'work_offset': wa, 'width': w, 'height': h, 'channels': 3,
                        'h_samp': hs, 'v_samp': vs})
    out = torch.full((out_total,), SENTINEL, dtype=torch.uint8, device=cuda)
    work = torch.full((work_total,), 0x5C, dtype=torch.uint8, device=cuda)          # nothing in it needs initialising
    records = torch.full((len(items) * J.RECORD_BYTES,), SENTINEL, dtype=torch.uint8, device=cuda)
    dev_coefs, dev_desc = _device(coefs, cuda), _device(_descs(entries), cuda)
    _lib.call("mpn_jpeg_entropy_encode", _lib.ptr(dev_coefs), dev_coefs.numel(), _lib.ptr(dev_desc), len(items), _lib.ptr(out),
              out.numel(), _lib.ptr(records), _lib.ptr(work), work.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    rec = records.cpu().numpy().view(J.RECORD)
    host = out.cpu().numpy()
    scans, written = [], []
    for r, oa in zip(rec, out_at):
        assert r['offset'] == oa
        if r['status'] == J.ENC_OK:
            scans.append(host[oa:oa + int(r['size'])].tobytes())
            written.append((oa, int(r['size'])))
        else:
            scans.append(None)
    assert _outside_untouched(host, written), "bytes outside the streams were written"
    return rec, scans


def _item(name):
    c = decoded(name)
    d = c.desc[0]
    return (c.coefs, int(d['width']), int(d['height']), int(d['h_samp']), int(d['v_samp']))


NAMES = [c[0] for c in CASES]


def test_forward_every_golden_alone(cuda):
    for name in NAMES:
        _forward(cuda, [name])


def test_forward_all_goldens_in_one_permuted_ragged_batch(cuda):
    order = np.random.RandomState(11).permutation(len(NAMES))
    _forward(cuda, [NAMES[i] for i in order], gap=16)


def test_forward_skips_descriptors_out_of_range(cuda):
    """An image whose descriptor reaches outside the buffers, is misaligned or names another sampling is left unwritten."""
    name = "17x23_420_noise_q95"
    px, want = goldens()[name][0], decoded(name)
    nbytes = want.coefs.nbytes
    base = {'src_offset': 0, 'coef_offset': 0, 'width': 23, 'height': 17, 'channels': 3, 'h_samp': 2, 'v_samp': 2, 'quant': want.desc[0]['quant']}
    second = dict(base, coef_offset=nbytes)                         # a valid place: only the named field is wrong
    entries = [base, dict(base, coef_offset=nbytes + 80), dict(base, coef_offset=nbytes + 8), dict(second, src_offset=1 << 40),
               dict(second, src_offset=8), dict(second, src_offset=-16), dict(second, h_samp=1, v_samp=2), dict(second, channels=5),
               dict(second, width=0), dict(second, width=70000), dict(second, height=65536)]
    dev_src = _device(np.concatenate([px.reshape(-1), np.zeros(64, np.uint8)]), cuda)
    coefs = torch.full((nbytes * 2 + 64,), SENTINEL, dtype=torch.uint8, device=cuda)
    dev_desc = _device(_descs(entries), cuda)
    _lib.call("mpn_jpeg_forward", _lib.ptr(dev_src), dev_src.numel(), _lib.ptr(dev_desc), len(entries), _lib.ptr(coefs), coefs.numel(),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    host = coefs.cpu().numpy()
    np.testing.assert_array_equal(host[:nbytes].view(np.int16).reshape(-1, 64), want.coefs)
    assert (host[nbytes:] == SENTINEL).all()


def test_entropy_encode_of_the_decoded_goldens_equals_their_scans(cuda):
    g = goldens()
    for n in NAMES:                                                 # alone: a one-image launch grid
        rec, scans = _entropy(cuda, [_item(n)])
        assert rec['status'].tolist() == [J.ENC_OK] and scans[0] == scan_of(g[n][1]), n
    order = np.random.RandomState(12).permutation(len(NAMES))
    names = [NAMES[i] for i in order]
    rec, scans = _entropy(cuda, [_item(n) for n in names], gap=16)  # all together, permuted
    for n, r, s in zip(names, rec, scans):
        want = scan_of(g[n][1])
        assert r['status'] == J.ENC_OK and r['size'] == len(want), (n, r)
        assert s == want, (n, next(i for i in range(len(want)) if s[i] != want[i]))


def test_entropy_encode_round_trips_the_decode_goldens(cuda):
    """Coefficients of files with optimised tables and restart intervals, as the project's host decoder reads them: encoded with
    the standard tables, decoded again by that decoder, they are the same coefficients."""
    from jpeg_cases import CASES as DECODE_CASES, UNSUPPORTED
    from test_jpeg_host import goldens as decode_goldens
    g = decode_goldens()
    names = [c[0] for c in DECODE_CASES if c[4] not in UNSUPPORTED and c[4] != 'L']          # (a grayscale scan is not written)
    assert names == ["1x1_420", "8x8_444", "8x8_420_flat", "5x7_422", "5x7_420", "17x17_420", "17x17_422", "17x17_444_checker",
                     "16x33_420_checker", "16x33_422_opt", "37x53_420_opt", "37x53_444", "37x53_422_rst_blocks", "48x64_420_rst_rows",
                     "48x64_420_flat", "48x64_444_q100", "120x160_420", "120x160_420_noise_rst", "120x160_422_checker", "3x5_420",
                     "2x4_422"]
    src = [J.entropy_decode(g[n][0]) for n in names]
    items = [(c.coefs, int(c.desc[0]['width']), int(c.desc[0]['height']), int(c.desc[0]['h_samp']), int(c.desc[0]['v_samp'])) for c in src]
    rec, scans = _entropy(cuda, items)
    sampling = {(1, 1): '4:4:4', (2, 1): '4:2:2', (2, 2): '4:2:0'}
    for n, c, it, r, s in zip(names, src, items, rec, scans):
        assert r['status'] == J.ENC_OK, (n, r)
        q = c.desc[0]['quant']
        np.testing.assert_array_equal(q[1], q[2])
        again = J.entropy_decode(J.jpeg_headers(it[1], it[2], sampling[it[3:]], (q[0], q[1])) + s)
        np.testing.assert_array_equal(again.coefs, c.coefs, err_msg=n)
        np.testing.assert_array_equal(again.desc[0]['quant'], q, err_msg=n)


def test_an_image_that_does_not_fit_is_reported_not_written(cuda):
    g = goldens()
    names = ["33x65_420_binary_q100", "120x160_420_binary_q100", "16x16_420_binary_q100"]      # one (quality, sampling)
    wants = [scan_of(g[n][1]) for n in names]
    caps = [_round16(len(wants[0]) + 64), len(wants[1]) - 1, _round16(len(wants[2]))]
    rec, scans = _entropy(cuda, [_item(n) for n in names], capacities=caps)
    assert rec['status'].tolist() == [J.ENC_OK, J.ENC_NO_FIT, J.ENC_OK]
    assert rec['size'].tolist() == [len(w) for w in wants]
    assert scans[0] == wants[0] and scans[1] is None and scans[2] == wants[2]
    # far too small: even the unstuffed stream exceeds the capacity; the size is then a lower bound
    rec, scans = _entropy(cuda, [_item(names[1])], capacities=[4096])
    assert rec['status'].tolist() == [J.ENC_NO_FIT_RAW] and 4096 < rec['size'][0] <= len(wants[1]) and scans == [None]
    # ONE encode call returns the three golden files, the middle one - and only it - through the fallback
    pixels = [g[n][0] for n in names]
    at, total = _place([p.size for p in pixels], 0, first=0)
    packed = np.zeros(total, np.uint8)
    for p, a in zip(pixels, at):
        packed[a:a + p.size] = p.reshape(-1)
    enc = J.JpegBatchEncoder(cuda)
    files = enc.encode(_device(packed, cuda), at, [p.shape[:2] for p in pixels], 3, 100, '4:2:0', capacities=caps)
    assert files == [g[n][1] for n in names] and enc.fallbacks == 1
    assert enc.copied_bytes == 3 * J.RECORD_BYTES + len(wants[0]) + len(wants[2])      # the records and the bytes used, no more


def test_encode_jpegs_equals_pillows_files(cuda):
    g = goldens()
    groups = {}
    for name, _, _, _, sub, quality, channels in CASES:
        if channels == 3:
            groups.setdefault((quality, sub), []).append(name)
    for (quality, sub), names in groups.items():
        files = J.encode_jpegs([g[n][0] for n in names], quality, sub, device=cuda)
        for n, f in zip(names, files):
            assert f == g[n][1], n
    # one encoder, a large batch then a smaller one: its buffers are reused; RGBA sources, alpha ignored
    enc = J.JpegBatchEncoder(cuda)
    for names in (["120x160_420_binary_q100", "33x65_420_binary_q100"], ["33x65_420_binary_q100"]):
        pixels = [g[n][0] for n in names]
        at, total = _place([p.size for p in pixels], 0, first=0)
        packed = np.zeros(total, np.uint8)
        for p, a in zip(pixels, at):
            packed[a:a + p.size] = p.reshape(-1)
        capacity = enc.capacity
        assert enc.encode(_device(packed, cuda), at, [p.shape[:2] for p in pixels], 3, 100, '4:2:0') == [g[n][1] for n in names]
        assert enc.fallbacks == 0
    assert enc.capacity == capacity
    for name in ("17x23_420_rgba_q75", "50x31_444_rgba_q95"):
        _, _, _, _, sub, quality, _ = _case(name)
        px = g[name][0]
        assert J.JpegBatchEncoder(cuda).encode(_device(px, cuda), [0], [px.shape[:2]], 4, quality, sub) == [g[name][1]], name


# ------------------------------------------------------------------------------------------------ the Detector
from test_detector_batch_gpu import _assert_same, _detector, _images, _variables, models  # noqa: E402,F401
from test_predict_images_gpu import SHAPES_A, _sources  # noqa: E402

H, W = 256, 384
SETTINGS = [(75, '4:2:0'), (95, '4:4:4')]


def _check_jpegs(got, drawn, quality, sub, msg):
    for i, (a, b) in enumerate(zip(got, drawn)):
        assert set(a) == (set(b) - {'annotated'}) | {'annotated_jpeg'}, (msg, i)
        assert isinstance(a['annotated_jpeg'], bytes)
        assert a['annotated_jpeg'] == J.pillow_encode(b['annotated'], quality, sub), (msg, i, quality, sub)
        a = dict(a)
        a.pop('annotated_jpeg')
        b = dict(b)
        b.pop('annotated')
        _assert_same(a, b, msg)


def test_predict_images_annotate_jpeg(cuda, models):
    det = _detector(models)
    sources = _sources(SHAPES_A, (1, 2, 3), 1)
    plain = det.predict_images(sources, size=(H, W))
    drawn = det.predict_images(sources, size=(H, W), annotate=True)
    keys = set(det._graphs)
    for quality, sub in SETTINGS:
        got = det.predict_images(sources, size=(H, W), annotate='jpeg', jpeg_quality=quality, jpeg_subsampling=sub)
        _check_jpegs(got, drawn, quality, sub, "predict_images")
    assert len(det._graphs) == len(keys) + 2                        # one entry per sampling
    before = set(det._graphs)
    got = det.predict_images(sources, size=(H, W), annotate='jpeg', jpeg_quality=30, jpeg_subsampling='4:2:0')
    _check_jpegs(got, drawn, 30, '4:2:0', "another quality")
    assert set(det._graphs) == before                               # another quality: a descriptor upload, the same graph
    eager = _detector(models, graph=False)
    _check_jpegs(eager.predict_images(sources, size=(H, W), annotate='jpeg'), drawn, 75, '4:2:0', "eager")
    assert not eager._graphs
    # annotate=True and annotate=False are what they were, and so are their cache keys
    for a, b in zip(det.predict_images(sources, size=(H, W), annotate=True), drawn):
        _assert_same(a, b, "annotate=True after 'jpeg':")
    for a, b in zip(det.predict_images(sources, size=(H, W)), plain):
        _assert_same(a, b, "annotate=False after 'jpeg':")
    assert set(det._graphs) == before and keys <= before
    assert all(k[-1] == 'annotate' or 'annotate' not in k for k in keys)


def test_predict_batch_annotate_jpeg(cuda, models):
    det = _detector(models)
    images = _images()
    plain = det.predict_batch(images, score_threshold=0.05)
    drawn = det.predict_batch(images, score_threshold=0.05, annotate=True)
    keys = set(det._graphs)
    assert keys == {(len(images), H, W, 0.05), (len(images), H, W, 0.05, 'annotate')}
    for quality, sub in SETTINGS:
        got = det.predict_batch(images, score_threshold=0.05, annotate='jpeg', jpeg_quality=quality, jpeg_subsampling=sub)
        _check_jpegs(got, drawn, quality, sub, "predict_batch")
    before = set(det._graphs)
    assert len(before) == len(keys) + 2
    _check_jpegs(det.predict_batch(images, score_threshold=0.05, annotate='jpeg', jpeg_quality=100), drawn, 100, '4:2:0', "quality 100")
    assert set(det._graphs) == before
    for a, b in zip(det.predict_batch(images, score_threshold=0.05, annotate=True), drawn):
        _assert_same(a, b, "annotate=True after 'jpeg':")
    for a, b in zip(det.predict_batch(images, score_threshold=0.05), plain):
        _assert_same(a, b, "annotate=False after 'jpeg':")
    assert set(det._graphs) == before


def test_predict_jpegs_annotate_jpeg(cuda, models):
    from test_jpeg_host import goldens as decode_goldens
    g = decode_goldens()
    jpegs = [g[n][0] for n in ("120x160_422_checker", "37x53_gray", "17x17_cmyk")]
    det = _detector(models)
    drawn = det.predict_jpegs(jpegs, size=(128, 128), score_threshold=0.0, annotate=True)
    for quality, sub in SETTINGS:
        got = det.predict_jpegs(jpegs, size=(128, 128), score_threshold=0.0, annotate='jpeg', jpeg_quality=quality, jpeg_subsampling=sub)
        _check_jpegs(got, drawn, quality, sub, "predict_jpegs")
