"""CPU: the heatmap and mask overlays of `plot_maps=True` - the numpy restatement tests/plot_maps_ref.py against the golden
pictures the reference notebook's `plot_maps` made under Pillow and matplotlib, the Lanczos tables against Pillow's own
`resize(..., Image.LANCZOS)`, the colour table, the label stamps against `ImageDraw.text`, and every argument check, none of
which needs a device. Equality is every byte; nothing is compared with a tolerance."""
import ctypes
import os

import numpy as np
import pytest

import pil_resize_ref as P
import plot_maps_ref as R
from multiposenet_amd import _lib
from multiposenet_amd.inference import detector, maps, resample

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plot_maps_goldens.npz")
F = np.float32


def goldens():
    with np.load(GOLDEN) as z:
        return [(str(n), z[f"{n}/image"], z[f"{n}/heatmaps"], z[f"{n}/mask"], z[f"{n}/maps"]) for n in z["names"]]


def golden_meta():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in ("colour_table", "labels", "pillow_version", "matplotlib_version", "numpy_version")}


def test_restatement_equals_every_golden_exactly():
    cases = goldens()
    assert {c[0] for c in cases} >= {"exact_x2", "ragged", "tall_strip", "values", "saturated_frame"}
    for name, img, heat, mask, want in cases:
        h, w = img.shape[0] // 2, img.shape[1] // 2
        assert want.shape == (18 * h, w, 4) and want.dtype == np.uint8
        got = R.plot_maps(img, heat, mask)
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert (want[..., 3] == 255).all()


def test_golden_cases_cover_what_they_claim():
    by_name = {c[0]: c[1:] for c in goldens()}
    assert [by_name[n][0].shape[:2] + by_name[n][1].shape[:2] for n in ("exact_x2", "ragged", "tall_strip", "values", "saturated_frame")] == \
        [(128, 128, 32, 32), (50, 38, 13, 10), (24, 136, 6, 34), (64, 64, 16, 16), (32, 32, 8, 8)]
    widest = max(m.shape[1] + ox for m, (ox, _) in maps.label_stamps())
    tallest = max(m.shape[0] + oy for m, (_, oy) in maps.label_stamps())
    assert by_name["ragged"][0].shape[1] // 2 < widest                       # a stamp clipped at the right edge
    assert by_name["short_panels"][0].shape[0] // 2 < tallest                # a stamp cut at the next panel
    img, heat, mask, _ = by_name["values"]
    assert np.isnan(heat[..., 1]).all() and (heat[..., 2] == 1).all() and (heat[..., 0] == 0).any() and (heat[..., 0] == 1).any()
    assert heat[..., 5:].min() < -0.4 and heat[..., 5:].max() > 1.4 and mask.min() < 0 and mask.max() > 1
    frame = by_name["saturated_frame"][0]
    assert set(np.unique(frame)) == {0, 255}
    # the Lanczos lobes do leave [0, 255] on the checkerboard before the intermediate is clipped
    bounds, coeffs = resample.resample_tables(32, 16, 'lanczos')
    acc = [int((coeffs[i, :bounds[i, 1]].astype(np.int64) * frame[0, bounds[i, 0]:bounds[i, 0] + bounds[i, 1], 0]).sum()) for i in range(16)]
    assert min(acc) < 0 and max(acc) > (255 << 22)


def test_goldens_record_their_versions_and_labels():
    meta = golden_meta()
    assert str(meta["pillow_version"]) and str(meta["matplotlib_version"]) and str(meta["numpy_version"])
    assert [str(s) for s in meta["labels"]] == list(maps.LABELS) and len(maps.LABELS) == maps.PANELS == 18


@pytest.mark.parametrize("in_size,out_size", [(128, 64), (32, 64), (50, 25), (38, 19), (13, 25), (10, 19), (24, 12), (136, 68),
                                              (6, 12), (34, 68), (64, 32), (16, 32), (8, 16), (100, 50), (100, 27)])
def test_lanczos_tables_reproduce_pillow_on_single_band_inputs(in_size, out_size):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(in_size * 1000 + out_size)
    a = rng.randint(0, 256, (in_size, 7)).astype(np.uint8)
    a[: in_size // 2, 0] = np.where(np.arange(in_size // 2) % 2, 255, 0)      # overshoot in the first column
    want_v = np.asarray(Image.fromarray(a).resize((7, out_size), Image.LANCZOS))
    np.testing.assert_array_equal(R.lanczos(a, out_size, 7), want_v)
    want_h = np.asarray(Image.fromarray(np.ascontiguousarray(a.T)).resize((out_size, 7), Image.LANCZOS))
    np.testing.assert_array_equal(R.lanczos(np.ascontiguousarray(a.T), 7, out_size), want_h)
    both = rng.randint(0, 256, (in_size, in_size)).astype(np.uint8)
    np.testing.assert_array_equal(R.lanczos(both, out_size, out_size),
                                  np.asarray(Image.fromarray(both).resize((out_size, out_size), Image.LANCZOS)))


def test_lanczos_kernel_sizes_and_the_filter_argument():
    assert resample.resample_tables(32, 64, 'lanczos')[1].shape[1] == 7       # x2 enlargement
    assert resample.resample_tables(128, 64, 'lanczos')[1].shape[1] == 13     # x2 reduction
    assert 13 < resample.MAX_KSIZE
    with pytest.raises(ValueError, match="filter"):
        resample.resample_tables(8, 4, 'box')
    for b, c in (resample.resample_tables(64, 32, 'lanczos'), resample.resample_tables(7, 19, 'lanczos')):
        assert b.dtype == np.int32 and c.dtype == np.int32 and not b.flags.writeable and not c.flags.writeable
        for i in range(len(b)):
            assert abs(int(c[i, :b[i, 1]].sum()) - (1 << 22)) <= b[i, 1] and (c[i, b[i, 1]:] == 0).all()


@pytest.mark.parametrize("in_size,out_size", [(640, 256), (97, 256), (500, 384), (131, 384), (1, 5), (7, 7), (1080, 128)])
def test_bicubic_tables_are_bit_identical_to_what_they_were(in_size, out_size):
    """filter='bicubic' and the default are the tables predict_images has always used: P.resize (pinned against Pillow's
    default filter by tests/test_image_resize_host.py) runs on the default; the explicit name gives the same arrays."""
    b0, c0 = resample.resample_tables(in_size, out_size)
    b1, c1 = resample.resample_tables(in_size, out_size, 'bicubic')
    b2, c2 = resample.resample_tables(in_size, out_size, filter='bicubic')
    for b, c in ((b1, c1), (b2, c2)):
        assert b.dtype == b0.dtype and c.dtype == c0.dtype and c.shape == c0.shape
        np.testing.assert_array_equal(b, b0)
        np.testing.assert_array_equal(c, c0)
    Image = pytest.importorskip("PIL.Image")
    a = np.random.RandomState(in_size).randint(0, 256, (in_size, 5, 3)).astype(np.uint8)
    np.testing.assert_array_equal(P.resize(a, out_size, 5), np.asarray(Image.fromarray(a).resize((5, out_size))))


def test_colour_table_equals_the_goldens_table():
    want = golden_meta()["colour_table"]
    assert want.shape == (256, 4) and want.dtype == np.uint8
    np.testing.assert_array_equal(maps.colour_table(), want)
    np.testing.assert_array_equal(R.colour_table(), want)
    pm = maps.premultiplied_table()
    t = want.astype(np.int64)
    v = t[:, :3] * t[:, 3:] + 128
    np.testing.assert_array_equal(pm[:, :3], ((v >> 8) + v) >> 8)
    np.testing.assert_array_equal(pm[:, 3], want[:, 3])


def test_index_rule_on_the_edges():
    x = np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -9, 1 / 256, 255 / 256, -2.0 ** -30, -0.5, 1.5, np.inf, -np.inf, np.nan], F)
    t = R.colour_table()
    want = [t[0], t[255], t[255], t[0], t[1], t[255], t[0], t[0], t[255], t[255], t[0], np.zeros(4, np.uint8)]
    np.testing.assert_array_equal(R.colourise(x), np.stack(want))


def test_every_stamp_on_white_equals_imagedraw_text():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageDraw
    stamps = maps.label_stamps()
    assert len(stamps) == 18
    for (mask, (ox, oy)), text in zip(stamps, maps.LABELS):
        assert mask.dtype == np.uint8 and mask.ndim == 2 and mask.size > 0 and mask.max() > 128
        for x0, y0, size in ((0, 0, (120, 20)), (3, 5, (120, 20)), (0, 0, (19, 7))):       # the last clips the stamp
            im = Image.new('RGBA', size, (255, 255, 255, 255))
            ImageDraw.Draw(im, 'RGBA').text((x0, y0), text, fill='red')
            got = np.full((size[1], size[0], 4), 255, np.uint8)
            R.blend_stamp(got, mask, x0 + ox, y0 + oy)
            np.testing.assert_array_equal(got, np.asarray(im), err_msg=text)


def test_alpha_composite_and_rgba_resize_equal_pillow_on_random_pixels():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(3)
    a, b = rng.randint(0, 256, (2, 40, 52, 4)).astype(np.uint8)
    a[:8, :, 3], a[8:16, :, 3], b[:4, :, 3], b[4:12, :, 3] = 0, 255, 0, 255
    np.testing.assert_array_equal(R.alpha_composite(a, b), np.asarray(Image.alpha_composite(Image.fromarray(a), Image.fromarray(b))))
    for size in ((80, 104), (20, 26), (61, 33)):
        want = np.asarray(Image.fromarray(b).resize((size[1], size[0]), Image.LANCZOS))
        np.testing.assert_array_equal(R.lanczos_rgba(b, *size), want)


def test_tables_and_descriptor_are_host_arithmetic():
    tables, desc = maps.tables_for(50, 38, 13, 10)
    assert tables.dtype == np.int32 and desc.dtype == np.int32 and desc.size == maps.DESC_WORDS
    assert _lib.lib().mpn_plot_maps_desc_bytes() == maps.DESC_WORDS * 4
    for i, (n_in, n_out) in enumerate(((38, 19), (50, 25), (10, 19), (13, 25))):
        bounds, coeffs = resample.resample_tables(n_in, n_out, 'lanczos')
        at_b, at_c, ksize = desc[3 * i:3 * i + 3]
        assert ksize == coeffs.shape[1] and at_b % 4 == 0 and at_c % 4 == 0
        np.testing.assert_array_equal(tables[at_b:at_b + bounds.size].reshape(bounds.shape), bounds)
        np.testing.assert_array_equal(tables[at_c:at_c + coeffs.size].reshape(coeffs.shape), coeffs)
    np.testing.assert_array_equal(tables[desc[12]:desc[12] + 256].view(np.uint8).reshape(256, 4), maps.premultiplied_table())
    sdesc = tables[desc[13]:desc[13] + 18 * maps.STAMP_WORDS].reshape(18, maps.STAMP_WORDS)
    pixels = tables[desc[14]:].view(np.uint8)[:desc[15]]
    for (mask, (ox, oy)), d in zip(maps.label_stamps(), sdesc):
        assert tuple(d[1:5]) == (mask.shape[1], mask.shape[0], ox, oy)
        np.testing.assert_array_equal(pixels[d[0]:d[0] + mask.size].reshape(mask.shape), mask)
    assert desc[13] % 4 == 0 and desc[14] + (desc[15] + 3) // 4 <= tables.size
    lib = _lib.lib()
    assert lib.mpn_plot_maps_workspace_bytes(2, 50, 38, 13, 10) == 2 * 20 * 4 * (50 + 18 * 13)
    assert lib.mpn_plot_maps_workspace_bytes(0, 50, 38, 13, 10) == 0 and lib.mpn_plot_maps_workspace_bytes(1, 1, 38, 13, 10) == 0
    assert lib.mpn_plot_maps_workspace_bytes(1, 128, 128, 3641, 32) == 0


def test_entry_point_validates_before_any_hip_call():
    P16 = ctypes.c_void_p(4096)
    tables, desc = maps.tables_for(128, 128, 32, 32)
    words = tables.size
    work = _lib.lib().mpn_plot_maps_workspace_bytes(1, 128, 128, 32, 32)

    def call(frames=P16, heat=P16, tab=P16, d=None, n=words, b=1, H=128, W=128, hh=32, hw=32, out=P16, ws=P16, nws=work):
        d = desc if d is None else d
        _lib.call("mpn_plot_maps", frames, heat, None, None, tab, n, d.ctypes.data, b, H, W, hh, hw, out, ws, nws, None)

    with pytest.raises(ValueError, match="null"):
        call(frames=None)
    with pytest.raises(ValueError, match="null"):
        call(out=None)
    for kw in ({"b": 0}, {"b": 65536}, {"H": 1}, {"W": 1}, {"hh": 0}, {"hw": 0}, {"hh": 3641}):
        with pytest.raises(ValueError, match="BAD_SHAPE"):
            call(**kw)
    with pytest.raises(ValueError, match="aligned"):
        call(out=ctypes.c_void_p(4100))
    with pytest.raises(_lib.MpnError, match="workspace"):
        call(nws=work - 1)
    with pytest.raises(ValueError, match="coefficient table"):
        call(n=words - 4000)                                         # the tables end before the descriptor's offsets
    for word, value in ((0, -4), (1, words), (2, 0), (2, resample.MAX_KSIZE + 1), (9, words - 3)):
        bad = desc.copy()
        bad[word] = value
        with pytest.raises(ValueError, match="coefficient table"):
            call(d=bad)
    for word, value in ((12, words - 255), (12, -1), (13, words), (13, desc[13] + 1), (14, words), (15, 4 * words), (15, -1)):
        bad = desc.copy()
        bad[word] = value
        with pytest.raises(ValueError, match="colour table or the stamps"):
            call(d=bad)


def test_argument_checks_need_no_device():
    img, heat, mask = np.zeros((64, 64, 3), np.uint8), np.zeros((16, 16, 17), F), np.zeros((16, 16), F)
    maps.check_arrays(img, heat, mask)
    for bad in ((img.astype(F), heat, mask), (img, heat.astype(np.float64), mask), (img, heat, mask.astype(np.float64)),
                (img[..., :2], heat, mask), (img[0], heat, mask), (img[:1], heat, mask), (img, heat[..., :16], mask),
                (img, heat, mask[:8]), (img, heat[0], mask), (img.tolist(), heat, mask)):
        with pytest.raises(ValueError):
            maps.check_arrays(*bad)
        with pytest.raises(ValueError):
            maps.plot_maps(*bad)
    with pytest.raises(ValueError, match="at least"):
        maps.tables_for(1, 64, 16, 16)
    # the Detector's keyword: a graph without heatmap outputs has nothing to plot
    assert detector.check_plot_maps(False, False) is False and detector.check_plot_maps(True, True) is True
    assert detector.check_plot_maps(False, True) is False
    with pytest.raises(ValueError, match="heatmap outputs"):
        detector.check_plot_maps(True, False)
    with pytest.raises(ValueError, match="False or True"):
        detector.check_plot_maps('jpeg', True)
    import inspect
    for name in ("predict_batch", "predict_images", "predict_jpegs"):
        assert inspect.signature(getattr(detector.Detector, name)).parameters["plot_maps"].default is False
