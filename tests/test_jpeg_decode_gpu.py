"""GPU: mpn_jpeg_decode (dequantise, inverse DCT, fancy upsampling, YCbCr -> RGB) through `JpegBatchDecoder`, held byte for
byte to the pixels Pillow decoded (tests/golden/jpeg_goldens.npz). No tolerance anywhere."""
import numpy as np
import pytest
import torch

from multiposenet_amd.inference import jpeg as J
from test_jpeg_host import goldens, supported_cases

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7


def _run(cuda, entries, wants, gap=48):
    """Decodes `entries` into a sentinel-filled buffer with `gap` untouched bytes around every image; returns nothing, asserts
    that every image equals its golden and every other byte kept the sentinel."""
    offsets, at = [], 16 + gap
    for w in wants:
        offsets.append(at)
        at = (at + w.size + gap + 15) // 16 * 16
    total = at + gap
    sources = torch.full((total,), SENTINEL, dtype=torch.uint8, device=cuda)
    dec = J.JpegBatchDecoder(cuda)
    dec.decode(entries, sources, offsets)
    torch.cuda.synchronize()
    host = sources.cpu().numpy()
    outside = np.ones(total, bool)
    for w, off in zip(wants, offsets):
        np.testing.assert_array_equal(host[off:off + w.size].reshape(w.shape), w)
        outside[off:off + w.size] = False
    assert (host[outside] == SENTINEL).all(), "bytes outside the images were written"
    return dec


def test_all_supported_cases_in_one_ragged_batch_equal_the_goldens(cuda):
    g = goldens()
    names = [c[0] for c in supported_cases()]
    assert len(names) >= 20
    _run(cuda, [J.prepare(g[n][0]) for n in names], [g[n][1] for n in names])


def test_each_case_alone_equals_its_golden(cuda):
    g = goldens()
    for name, *_ in supported_cases():
        entry = J.prepare(g[name][0])
        assert isinstance(entry, J.Coefficients), name
        _run(cuda, [entry], [g[name][1]])


def test_a_permuted_batch_equals_the_goldens(cuda):
    g = goldens()
    names = [c[0] for c in supported_cases()]
    order = np.random.RandomState(5).permutation(len(names))
    names = [names[i] for i in order]
    dec = _run(cuda, [J.prepare(g[n][0]) for n in names], [g[n][1] for n in names], gap=16)
    # the same decoder again, with a smaller batch: its buffers are reused
    want = g[names[0]][1]
    sources = torch.full((32 + want.size + 32,), SENTINEL, dtype=torch.uint8, device=cuda)
    dec.decode([J.prepare(g[names[0]][0])], sources, [32])
    torch.cuda.synchronize()
    host = sources.cpu().numpy()
    np.testing.assert_array_equal(host[32:32 + want.size].reshape(want.shape), want)
    assert (host[:32] == SENTINEL).all() and (host[32 + want.size:] == SENTINEL).all()


def test_unsupported_streams_and_arrays_take_the_pixel_path(cuda):
    g = goldens()
    rng = np.random.RandomState(9)
    array = rng.randint(0, 256, (11, 13, 3)).astype(np.uint8)
    names = ["48x64_progressive", "17x17_420", "17x17_cmyk", "120x160_420"]
    entries = [J.prepare(g[n][0]) for n in names]
    assert [isinstance(e, J.Coefficients) for e in entries] == [False, True, False, True]
    entries.insert(2, array)
    wants = [g[n][1] for n in names]
    wants.insert(2, array)
    _run(cuda, entries, wants)
    # a batch with no JPEG entry at all launches nothing and still copies
    _run(cuda, [array, entries[0]], [array, wants[0]])


def test_a_descriptor_that_does_not_fit_is_refused_on_the_host(cuda):
    g = goldens()
    entry = J.prepare(g["48x64_420_flat"][0])
    sources = torch.zeros(48 * 64 * 3, dtype=torch.uint8, device=cuda)
    dec = J.JpegBatchDecoder(cuda)
    with pytest.raises(ValueError, match="does not fit"):
        dec.decode([entry], sources, [16])
    with pytest.raises(ValueError, match="multiple of 16"):
        dec.decode([entry], torch.zeros(48 * 64 * 3 + 64, dtype=torch.uint8, device=cuda), [8])


def test_a_larger_second_batch_grows_every_buffer_behind_a_queued_first(cuda):
    """One decoder, a batch of one 8x8 image (1 KB of staging), then - with no synchronise in between - a batch of all three
    kinds of entry that outgrows the staging, its device copy, the inverse-DCT planes and the device's coefficient buffer:
    replacing a buffer must wait for the work that is still queued on it. Both batches equal Pillow's pixels.
    What this holds is the decoder's bookkeeping of its buffers across growth: the buffers of the Scan path are first
    allocations here, not growth, and an allocator that recycles freed blocks in stream order can hide a missing synchronise."""
    g = goldens()
    dec = J.JpegBatchDecoder(cuda)
    small = g["8x8_444"][1]
    first = torch.full((16 + small.size + 16,), SENTINEL, dtype=torch.uint8, device=cuda)
    dec.decode([J.prepare(g["8x8_444"][0])], first, [16])
    before = {name: buf.numel() for name, buf in dec._buf.items()}
    assert before == {'stage': 1024, 'dev': 1024, 'work': 256} and dec.staged_bytes == 896
    array = np.random.RandomState(11).randint(0, 256, (17, 17, 3)).astype(np.uint8)
    entries = [J.prepare(g["120x160_420"][0]), J.prepare(g["37x53_422_rst_blocks"][0], entropy='device'), array]
    assert [type(e) for e in entries] == [J.Coefficients, J.Scan, np.ndarray]
    wants = [g["120x160_420"][1], g["37x53_422_rst_blocks"][1], array]
    offsets = [16, 16 + 57616, 16 + 57616 + 5904]              # 120 * 160 * 3 = 57600, 37 * 53 * 3 = 5883, each + a gap
    second = torch.full((offsets[2] + array.size + 16,), SENTINEL, dtype=torch.uint8, device=cuda)
    dec.decode(entries, second, offsets)
    torch.cuda.synchronize()
    assert all(dec._buf[name].numel() > n for name, n in before.items())
    assert dec._buf['scan_coefs'].numel() >= entries[1].total_blocks * 128 and dec.fallbacks == 0
    host = first.cpu().numpy()
    np.testing.assert_array_equal(host[16:16 + small.size].reshape(small.shape), small)
    assert (host[:16] == SENTINEL).all() and (host[16 + small.size:] == SENTINEL).all()
    host, outside = second.cpu().numpy(), np.ones(second.numel(), bool)
    for w, off in zip(wants, offsets):
        np.testing.assert_array_equal(host[off:off + w.size].reshape(w.shape), w)
        outside[off:off + w.size] = False
    assert (host[outside] == SENTINEL).all(), "bytes outside the images were written"
