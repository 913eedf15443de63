"""GPU: mpn_jpeg_entropy_decode_device through `JpegBatchDecoder` with Scan entries. The yardsticks are the host
`entropy_decode` (coefficients, block for block) and tests/golden/jpeg_goldens.npz (pixels). No tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

from multiposenet_amd.inference import jpeg as J
from test_jpeg_entropy_host import PHASE_FILES, phase_sweep
from test_jpeg_host import goldens, supported_cases

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7
LONG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_entropy_goldens.npz")
_host = {}


def host(data):
    """The host stage's Coefficients for a file, computed once and shared by the tests."""
    if data not in _host:
        _host[data] = J.entropy_decode(data)
    return _host[data]


def long_files():
    with np.load(LONG) as z:
        return {str(n): z[f"{n}/jpeg"].tobytes() for n in z["names"]}


def stage(cuda, files, max_passes=J.MAX_PASSES, file_order=None):
    """The device's entropy stage and inverse DCT over `files` -> (decoder, statuses, pixels per image, coefficients per image)."""
    scans = [J.scan_prepare(f) for f in files]
    offsets, at = [], 16
    for s in scans:
        offsets.append(at)
        at = (at + s.shape[0] * s.shape[1] * 3 + 48 + 15) // 16 * 16
    sources = torch.full((at,), SENTINEL, dtype=torch.uint8, device=cuda)
    dec = J.JpegBatchDecoder(cuda, max_passes=max_passes)
    dec.decode_scans(scans, sources, offsets, torch.cuda.current_stream(cuda), file_order)
    torch.cuda.synchronize()
    out = sources.cpu().numpy()
    pixels = [out[o:o + s.shape[0] * s.shape[1] * 3].reshape(s.shape) for s, o in zip(scans, offsets)]
    return dec, [int(r['status']) for r in dec.records], pixels, [dec.scan_coefficients(k) for k in range(len(scans))]


def decode(cuda, files, wants, max_passes=J.MAX_PASSES):
    """`JpegBatchDecoder.decode` over Scan entries into a sentinel-filled buffer: every image equals its `want`, every other
    byte kept the sentinel. Returns the decoder."""
    entries = [J.prepare(f, entropy='device') for f in files]
    assert all(isinstance(e, J.Scan) for e in entries)
    offsets, at = [], 64
    for w in wants:
        offsets.append(at)
        at = (at + w.size + 48 + 15) // 16 * 16
    sources = torch.full((at + 48,), SENTINEL, dtype=torch.uint8, device=cuda)
    dec = J.JpegBatchDecoder(cuda, max_passes=max_passes)
    dec.decode(entries, sources, offsets)
    torch.cuda.synchronize()
    out = sources.cpu().numpy()
    outside = np.ones(out.size, bool)
    for w, off in zip(wants, offsets):
        np.testing.assert_array_equal(out[off:off + w.size].reshape(w.shape), w)
        outside[off:off + w.size] = False
    assert (out[outside] == SENTINEL).all(), "bytes outside the images were written"
    return dec


def check_exact(files, statuses, coefs):
    for k, f in enumerate(files):
        assert statuses[k] == J.ENT_OK, (k, statuses[k])
        np.testing.assert_array_equal(coefs[k], host(f).coefs, err_msg=str(k))


def test_all_supported_goldens_in_one_ragged_batch(cuda):
    g = goldens()
    names = [c[0] for c in supported_cases()]
    files = [g[n][0] for n in names]
    dec, statuses, pixels, coefs = stage(cuda, files)
    check_exact(files, statuses, coefs)
    for n, p, r in zip(names, pixels, dec.records):
        np.testing.assert_array_equal(p, g[n][1], err_msg=n)
        assert r['blocks'] == host(g[n][0]).coefs.shape[0] and r['passes'] == 1, n    # every golden scan lies inside one group
    dec = decode(cuda, files, [g[n][1] for n in names])
    assert dec.fallbacks == 0 and (dec.records['status'] == J.ENT_OK).all()


def test_phase_sweep_of_both_files_in_one_batch_of_256(cuda):
    files = [f for name in PHASE_FILES for f in phase_sweep(name)]
    assert len(files) == 256
    _, statuses, _, coefs = stage(cuda, files)
    g = goldens()
    for k in range(256):
        assert statuses[k] == J.ENT_OK, k
        np.testing.assert_array_equal(coefs[k], host(g[PHASE_FILES[k // 128]][0]).coefs, err_msg=str(k))


def test_each_case_alone_and_a_permuted_batch(cuda):
    g = goldens()
    names = [c[0] for c in supported_cases()]
    assert {"1x1_420", "8x8_420_flat", "37x53_422_rst_blocks"} <= set(names)
    for n in names:
        dec = decode(cuda, [g[n][0]], [g[n][1]])
        assert dec.fallbacks == 0, n
    order = np.random.RandomState(5).permutation(len(names))
    names = [names[i] for i in order]
    dec = decode(cuda, [g[n][0] for n in names], [g[n][1] for n in names])
    assert dec.fallbacks == 0


def test_streams_longer_than_one_group(cuda):
    files = long_files()
    assert sorted(files) == ["240x320_checker", "240x320_noise", "240x320_noise_opt", "240x320_smooth"]
    assert os.path.getsize(LONG) <= 200 * 1024 and sum(len(f) > 32768 for f in files.values()) == 3
    names = sorted(files)
    data = [files[n] for n in names]
    dec, statuses, _, coefs = stage(cuda, data)
    print("passes", dict(zip(names, dec.records['passes'].tolist())), "statuses", statuses)
    for k, n in enumerate(names):
        # the periodic checker never self-synchronises, but it is two groups long: after pass k the first k groups are exact
        assert statuses[k] == J.ENT_OK, (n, statuses[k])
        np.testing.assert_array_equal(coefs[k], host(files[n]).coefs, err_msg=n)
        assert 1 <= dec.records['passes'][k] <= -(-len(files[n]) // 32768)
    assert dec.records['passes'][names.index("240x320_checker")] == 2
    wants = [J.pillow_decode(f) for f in data]
    dec = decode(cuda, data, wants)
    assert dec.fallbacks == sum(s != J.ENT_OK for s in statuses)
    # with the mixed goldens around them, in one batch
    g = goldens()
    more = ["17x17_420", "48x64_420_rst_rows", "1x1_gray"]
    mixed = [g[more[0]][0], data[1], g[more[1]][0], data[3], data[0], g[more[2]][0], data[2]]
    _, statuses, _, coefs = stage(cuda, mixed)
    check_exact(mixed, statuses, coefs)


def test_files_staged_in_another_order_than_their_descriptors(cuda):
    """The workspace is divided in descriptor order, wherever the files lie: a short file in front of a long one's descriptor
    but behind it in the buffer, a reversed and a shuffled layout, two groups and restarts among them."""
    g = goldens()
    files = long_files()
    batch = [g["17x17_420"][0], files["240x320_noise"], g["48x64_420_rst_rows"][0], g["1x1_gray"][0], files["240x320_checker"],
             g["48x64_444_q100"][0], g["8x8_420_flat"][0]]
    n = len(batch)
    for order in (list(range(n))[::-1], [4, 0, 6, 1, 5, 3, 2], [n - 1] + list(range(n - 1))):
        _, statuses, pixels, coefs = stage(cuda, batch, file_order=order)
        check_exact(batch, statuses, coefs)
        for k in (0, 2, 3, 5, 6):
            name = ("17x17_420", None, "48x64_420_rst_rows", "1x1_gray", None, "48x64_444_q100", "8x8_420_flat")[k]
            np.testing.assert_array_equal(pixels[k], g[name][1], err_msg=name)


def test_one_pass_forces_the_fallback(cuda):
    files = long_files()
    names = sorted(files)
    data = [files[n] for n in names] + [goldens()["120x160_420"][0]]
    _, statuses, _, coefs = stage(cuda, data, max_passes=1)
    long = [len(f) > 32768 for f in data]
    assert sum(long) == 3
    # a group's first guess (its own start, block 0, index 0) is not where the previous group ends: one pass cannot settle
    assert [s == J.ENT_NOT_CONVERGED for s in statuses] == long, statuses
    for k, f in enumerate(data):
        if not long[k]:
            check_exact([f], [statuses[k]], [coefs[k]])
    dec = decode(cuda, data, [J.pillow_decode(f) for f in data], max_passes=1)
    assert dec.fallbacks == 3 and (dec.records['status'] == J.ENT_NOT_CONVERGED).sum() == 3
    assert (dec.records['passes'] == 1).all()


def test_damaged_files_in_the_middle_of_a_batch(cuda):
    g = goldens()
    names = ("48x64_444_q100", "120x160_420", "120x160_422_checker")
    good = [g[n][0] for n in ("17x17_420", "48x64_gray_rst", "37x53_444", "16x33_422_opt")]
    cuts = []
    for n in names:
        d = g[n][0]
        cuts += [d[:len(d) // 4], d[:len(d) // 2], d[:-3], d[:-1]]      # the last scan byte (and EOI) gone; the last file byte gone
    for c in cuts[:-1:4] + cuts[1::4] + cuts[2::4]:
        with pytest.raises(ValueError):
            J.entropy_decode(c)
    batch = good[:2] + cuts + good[2:]
    _, statuses, pixels, coefs = stage(cuda, batch)
    assert statuses[2:2 + len(cuts)] == [J.ENT_BAD_DATA] * len(cuts), statuses
    for k in (0, 1, len(batch) - 2, len(batch) - 1):
        check_exact([batch[k]], [statuses[k]], [coefs[k]])
    # decode(): the host stage's ValueError for a damaged stream ...
    for c in (cuts[0], cuts[5], cuts[10]):
        entries = [J.prepare(f, entropy='device') for f in (good[0], c, good[1])]
        sources = torch.zeros(1 << 17, dtype=torch.uint8, device=cuda)
        with pytest.raises(ValueError, match="BAD_DATA"):
            J.JpegBatchDecoder(cuda).decode(entries, sources, [0, 32768, 98304])
    # ... and a file that only lost the last byte of its EOI, which the host stage accepts, arrives through the fallback
    dec = decode(cuda, [good[0], cuts[3], good[1]], [J.pillow_decode(good[0]), g[names[0]][1], J.pillow_decode(good[1])])
    assert dec.fallbacks == 1 and dec.records['status'].tolist() == [J.ENT_OK, J.ENT_BAD_DATA, J.ENT_OK]
