"""CPU: the restatement tests/crops_ref.py against Pillow's `resize(box=)`, `inference.PersonCrops`, the `crops=` keyword of
the Detector's predict_* methods and its place in the entries' keys, the size helpers and every argument check of the C entry
point, which run before any HIP call, and the flags of track_frames."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import crops_cases as C
import crops_ref as R
from multiposenet_amd import _lib
from multiposenet_amd.inference import Detector, PersonCropper, PersonCrops, person_crops
from multiposenet_amd.inference import crops as crops_stage
from multiposenet_amd.inference.detector import _Options
from multiposenet_amd.inference.record import RecordLayout
from test_detector_options_host import B, CAP, H, THR, W, _detector, _key_of, _table

DEFAULTS = dict(size=(256, 128), pad=0.0, fit='stretch', fill=(0, 0, 0), format='rgb', jpeg_quality=75, jpeg_subsampling='4:2:0',
                max_boxes=25)


# ------------------------------------------------------------------ the reference
def test_the_cases_hit_what_they_are_meant_to():
    C.check_cases(R)
    sizes = {c['size'] for c in C.cases()}
    frames = {im.shape[:2] for c in C.cases() for im in c['images']}
    assert sizes == {(16, 8), (24, 16), (8, 8)} and frames == {(37, 53), (64, 48), (208, 16)}


@pytest.mark.parametrize("fit", R.FITS)
def test_reference_equals_pillow_resize_with_a_box(fit):
    from PIL import Image
    checked = 0
    for c in C.cases():
        H_, W_ = c['size']
        for image, rows in zip(c['images'], c['boxes']):
            for box in rows:
                got, info = R.crop(image, box, c['size'], c['pad'], fit, c['fill'])
                if info['empty'] or info['too_large']:
                    assert (got == np.asarray(c['fill'], np.uint8)).all(), c['name']
                    continue
                top, left, new_h, new_w = info['placed']
                part = Image.fromarray(image).resize((new_w, new_h), Image.BICUBIC, box=tuple(info['rect']))
                canvas = Image.new('RGB', (W_, H_), c['fill'])
                canvas.paste(part, (left, top))
                np.testing.assert_array_equal(got, np.asarray(canvas), err_msg=f"{c['name']} {fit} {info}")
                if fit == 'stretch':
                    assert (top, left, new_h, new_w) == (0, 0, H_, W_)
                checked += 1
    assert checked >= 25


def test_the_plain_loops_and_the_numpy_sums_are_one_function():
    for c in C.cases()[:4]:
        for image, rows in zip(c['images'], c['boxes']):
            for box in rows:
                a, _ = R.crop(image, box, c['size'], c['pad'], 'pad', c['fill'], fast=False)
                b, _ = R.crop(image, box, c['size'], c['pad'], 'pad', c['fill'], fast=True)
                np.testing.assert_array_equal(a, b, err_msg=c['name'])


def test_unscaled_taps_are_the_identity_and_the_rounding_is_half_to_even():
    taps = R.axis_taps(10.0, 26.0, 64, 16)
    assert all(k[first_k] == 1 << 22 and sum(abs(v) for v in k) == 1 << 22
               for yy, (first, k) in enumerate(taps) for first_k in [10 + yy - first])
    assert R.placement(32.0, 9.0, 16, 8, 'pad') == (0, 2, 16, 4) and R.placement(32.0, 15.0, 16, 8, 'pad') == (0, 0, 16, 8)
    assert R.placement(1e-300, 1e-300, 16, 8, 'pad')[2:] == (8, 8) and R.placement(5e-324, 3.0, 16, 8, 'pad')[2:] == (1, 8)
    assert R.ksize_of(0.0, 128.0, 8) == 65 and R.ksize_of(0.0, 128.5, 8) == 67 and R.ksize_of(0.0, 4.0, 16) == 5


# ------------------------------------------------------------------ the parameter class
def test_defaults_repr_equality_and_immutability():
    a = PersonCrops()
    assert list(PersonCrops.__slots__) == list(DEFAULTS) and a.astuple() == tuple(DEFAULTS.values())
    assert list(inspect.signature(PersonCrops).parameters) == list(DEFAULTS)
    assert repr(a) == ("PersonCrops(size=(256, 128), pad=0.0, fit='stretch', fill=(0, 0, 0), format='rgb', jpeg_quality=75, "
                       "jpeg_subsampling='4:2:0', max_boxes=25)")
    assert not hasattr(a, '__dict__')
    assert a == PersonCrops(**DEFAULTS) and hash(a) == hash(PersonCrops(**DEFAULTS)) and a != a.astuple()
    changed = dict(size=(64, 32), pad=0.25, fit='pad', fill=(0, 0, 1), format='jpeg', jpeg_quality=90, jpeg_subsampling='4:4:4',
                   max_boxes=32)
    for name, value in changed.items():
        other = PersonCrops(**{name: value})
        assert other != a and getattr(other, name) == value, name
    assert len({a, PersonCrops(), PersonCrops(pad=0.5)}) == 2
    assert PersonCrops(size=[8, 256]).size == (8, 256) and PersonCrops(size=np.array([512, 8])).size == (512, 8)
    assert PersonCrops(fill=[1, 2, 3]).fill == (1, 2, 3) and PersonCrops(fill=(1, 2, 3)).fill_word == 1 | 2 << 8 | 3 << 16
    assert PersonCrops(pad=1).pad == 1.0 and PersonCrops(pad=4).pad == 4.0 and PersonCrops(size=(16, 8)).crop_bytes == 384
    for change in (lambda: setattr(a, 'pad', 1.0), lambda: setattr(a, 'other', 1), lambda: delattr(a, 'pad')):
        with pytest.raises(AttributeError, match="^PersonCrops is immutable$"):
            change()


@pytest.mark.parametrize("name,bad", [
    ('size', (256,)), ('size', 256), ('size', (250, 128)), ('size', (256, 100)), ('size', (0, 128)), ('size', (520, 128)),
    ('size', (256, 264)), ('size', (256.0, 128)), ('size', (True, 8)), ('pad', -0.1), ('pad', 4.5), ('pad', float('nan')),
    ('pad', float('inf')), ('pad', 'wide'), ('pad', True), ('fit', 'crop'), ('fit', 0), ('fill', (0, 0)), ('fill', (0, 0, 256)),
    ('fill', (0.5, 0, 0)), ('fill', 7), ('format', 'png'), ('format', None), ('jpeg_quality', 0), ('jpeg_quality', 101),
    ('jpeg_quality', 75.5), ('jpeg_quality', 'high'), ('jpeg_subsampling', '4:1:1'), ('jpeg_subsampling', 2), ('max_boxes', 0),
    ('max_boxes', 129), ('max_boxes', 25.0),
])
def test_every_range_error_names_the_argument_and_the_value(name, bad):
    with pytest.raises(ValueError, match="^PersonCrops: " + name + " must .*" + re.escape(f"(got {bad!r})") + "$"):
        PersonCrops(**{name: bad})


# ------------------------------------------------------------------ the Detector's keys and checks
def test_signatures_and_exports():
    from multiposenet_amd import inference
    assert inference.PersonCrops is crops_stage.PersonCrops and inference.person_crops is crops_stage.person_crops
    assert inference.PersonCropper is crops_stage.PersonCropper and callable(PersonCropper.__call__)
    assert list(inspect.signature(person_crops).parameters) == ['image', 'outputs', 'spec']
    for method in ('predict_batch', 'predict_images', 'predict_jpegs'):
        sig = inspect.signature(getattr(Detector, method)).parameters
        assert sig['crops'].default is None and list(sig)[-1] == 'track_eval', method
        assert list(sig).index('crops') < list(sig).index('track_eval')
        doc = getattr(Detector, method).__doc__
        assert "crops:" in doc and "never the" in doc and "overlays" in doc, method
    assert 'crops' not in inspect.signature(Detector.__call__).parameters
    assert "un-anonymised pixel" in Detector.predict_batch.__doc__
    assert RecordLayout.PARTS == ('record', 'oks', 'track', 'nms', 'track_eval', 'zones', 'trails', 'density')
    assert 'crops' not in RecordLayout.__slots__


def test_options_field_and_tail():
    from multiposenet_amd.inference import Anonymize
    det = _detector(True)
    spec = PersonCrops()
    given = dict(score_threshold=THR, return_heatmaps=True, annotate=False, jpeg_quality=75, jpeg_subsampling='4:2:0',
                 plot_maps=False, groundtruth=None, flip=False, scales=None, track=None, track_style=None)
    opts, _ = det._options(lambda: (B, H, W), **given)              # `crops` may be absent
    assert opts.crops is None and opts.tail(B) == ()
    opts, _ = det._options(lambda: (B, H, W), crops=spec, **given)
    assert opts.crops is spec and opts.tail(B) == ('crops', spec)
    assert _Options._fields[-6:] == ('crops', 'density', 'trails', 'zones', 'anonymize', 'pose_nms')
    anon = Anonymize()
    opts, _ = det._options(lambda: (B, H, W), crops=spec, anonymize=anon, **dict(given, annotate=True))
    assert opts.tail(B) == ('annotate', 'anonymize', anon, 'crops', spec)


@pytest.mark.parametrize("use_graph", [True, False])
def test_entry_keys_are_the_literal_tuples(use_graph):
    det = _detector(use_graph)
    batch = np.zeros((B, H, W, 3), np.uint8)
    frames = [np.zeros((50, 70, 3), np.uint8), np.zeros((64, 33, 3), np.uint8)]
    base = (B, H, W, THR) if use_graph else ('eager', B, H, W)
    spec = PersonCrops(size=(64, 32), fit='pad')
    for options, tail in _table():
        assert _key_of(det.predict_batch, batch, score_threshold=THR, crops=None, **options) == base + tail      # None changes nothing
        key = _key_of(det.predict_batch, batch, score_threshold=THR, crops=spec, **options)
        assert key == base + tail + ('crops', spec), options
        key = _key_of(det.predict_images, frames, size=(H, W), score_threshold=THR, crops=PersonCrops(size=(64, 32), fit='pad'), **options)
        assert key == ('images', B, H, W, THR, CAP) + tail + ('crops', spec), options
    assert _key_of(det.predict_batch, batch, score_threshold=THR, crops=PersonCrops(format='jpeg')) != \
        _key_of(det.predict_batch, batch, score_threshold=THR, crops=PersonCrops())


def test_argument_checks_and_their_order():
    det = _detector(True)
    batch, frames = np.zeros((B, H, W, 3), np.uint8), [np.zeros((50, 70, 3), np.uint8)] * B
    for method, first in ((det.predict_batch, batch), (det.predict_images, frames)):
        for bad in ('person', dict(size=(8, 8)), (256, 128)):
            with pytest.raises(ValueError, match="crops must be None or an inference.PersonCrops"):
                method(first, crops=bad)
        with pytest.raises(ValueError, match=r"crops=: the PersonCrops was made for max_boxes = 32, this Detector's is 25"):
            method(first, crops=PersonCrops(max_boxes=32))
        with pytest.raises(ValueError, match="flip must be"):      # checked last
            method(first, flip=1, crops='x')
        with pytest.raises(ValueError, match="anonymize must be"):
            method(first, annotate=True, anonymize='x', crops='x')
    with pytest.raises(ValueError, match="empty batch"):
        det.predict_jpegs([], crops='x')
    nodet = _detector(True)
    nodet.retinanet = None
    with pytest.raises(ValueError, match="crops= needs the person detector"):
        nodet.predict_batch(batch, crops=PersonCrops())
    many = _detector(True)
    many.params = {'max_boxes': 128}
    with pytest.raises(ValueError, match=r"crops=: 33 x 128 slots are more than mpn_person_crops takes"):
        many.predict_batch(np.zeros((33, H, W, 3), np.uint8), crops=PersonCrops(max_boxes=128))
    key = _key_of(det.predict_batch, batch, crops=PersonCrops())   # it does not need annotate
    assert key[-2] == 'crops'


# ------------------------------------------------------------------ the C ABI, without a GPU
def test_size_helpers_against_their_formulas():
    l = _lib.lib()
    assert l.mpn_person_crops_desc_bytes() == 32 == l.mpn_draw_desc_bytes()
    assert crops_stage.INFO.itemsize == 64 and crops_stage.TAP_WORDS == 68 >= 3 + 65
    for b, m, h, w in ((16, 25, 256, 128), (1, 1, 8, 8), (32, 128, 512, 256), (4096, 1, 16, 8)):
        assert l.mpn_person_crops_info_bytes(b, m) == b * m * 64
        assert l.mpn_person_crops_workspace_bytes(b, m, h, w) == b * m * (h + w) * 68 * 4
    for b, m in ((0, 25), (1, 0), (1, 129), (-1, 25), (4097, 1), (64, 65), (33, 128)):
        assert l.mpn_person_crops_info_bytes(b, m) == 0 and l.mpn_person_crops_workspace_bytes(b, m, 256, 128) == 0, (b, m)
    for h, w in ((0, 128), (4, 128), (260, 128), (520, 128), (256, 0), (256, 100), (256, 264), (-8, 8)):
        assert l.mpn_person_crops_workspace_bytes(1, 25, h, w) == 0, (h, w)
    # the tile rule: the largest tile whose tile * 16 + 64 rows of W * 3 bytes fit the block's 160 KiB of LDS
    assert crops_stage.LDS_BYTES == 160 * 1024
    for (h, w), tile in (((256, 128), 22), ((512, 256), 9), ((8, 8), 8), ((512, 8), 422), ((16, 256), 9), ((8, 256), 8)):
        assert crops_stage.tile_rows(h, w) == tile, (h, w)
        assert (tile * 16 + 64) * w * 3 <= crops_stage.LDS_BYTES
        assert tile == h or ((tile + 1) * 16 + 64) * w * 3 > crops_stage.LDS_BYTES


def test_every_argument_check_runs_before_any_hip_call():
    l = _lib.lib()
    P, Q = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    b, m, h, w = 2, 25, 16, 8
    record, work = l.mpn_pose_gather_record_bytes(b, m), l.mpn_person_crops_workspace_bytes(b, m, h, w)

    def call(sources=P, sources_bytes=1000, descs=P, rec=P, record_bytes=record, B_=b, M=m, H_=h, W_=w, pad=0.0, fit=0, fill=0,
             out=P, info=P, workspace=P, workspace_bytes=work):
        return _lib.call("mpn_person_crops", sources, sources_bytes, descs, rec, record_bytes, B_, M, H_, W_, pad, fit, fill, out,
                         info, workspace, workspace_bytes, None)
    for null in ('sources', 'descs', 'rec', 'out', 'info', 'workspace'):
        with pytest.raises(ValueError, match="BAD_ARG: person_crops: null pointer"):
            call(**{null: None})
    for bad in (dict(B_=0), dict(B_=65536), dict(M=0), dict(M=129), dict(B_=64, M=65), dict(H_=0), dict(H_=12), dict(H_=520),
                dict(W_=4), dict(W_=20), dict(W_=264)):
        with pytest.raises(ValueError, match="BAD_SHAPE: person_crops"):
            call(**bad)
    for bad in (dict(pad=-0.5), dict(pad=4.5), dict(pad=float('nan')), dict(pad=float('inf'))):
        with pytest.raises(ValueError, match="BAD_ARG: person_crops: pad"):
            call(**bad)
    for bad in (dict(fit=-1), dict(fit=2)):
        with pytest.raises(ValueError, match="BAD_ARG: person_crops: fit"):
            call(**bad)
    for bad in (dict(fill=-1), dict(fill=1 << 24)):
        with pytest.raises(ValueError, match="BAD_ARG: person_crops: fill"):
            call(**bad)
    for name in ('descs', 'rec', 'out', 'info', 'workspace'):
        with pytest.raises(ValueError, match="BAD_ALIGN: person_crops"):
            call(**{name: Q})
    for bad in (dict(record_bytes=record - 1), dict(workspace_bytes=work - 1), dict(sources_bytes=2)):
        with pytest.raises(_lib.MpnError, match="WORKSPACE: person_crops"):
            call(**bad)


def test_collect_takes_a_count():
    from multiposenet_amd.inference.jpeg import JpegBatchEncoder
    parameters = inspect.signature(JpegBatchEncoder.collect).parameters
    assert list(parameters) == ['self', 'plan', 'sources', 'count'] and parameters['count'].default is None


# ------------------------------------------------------------------ track_frames
def test_command_line_flags():
    import argparse
    ap = argparse.ArgumentParser()
    crops_stage.add_arguments(ap)
    assert crops_stage.from_arguments(ap, ap.parse_args([])) is None
    assert crops_stage.from_arguments(ap, ap.parse_args(["--crops-out", "d"])) == PersonCrops(format='jpeg')
    got = crops_stage.from_arguments(ap, ap.parse_args(["--crops-out", "d", "--crop-size", "64", "32", "--crop-pad", "0.1", "--crop-fit",
                                                         "pad", "--crop-quality", "90"]), 32)
    assert got == PersonCrops(size=(64, 32), pad=0.1, fit='pad', format='jpeg', jpeg_quality=90, max_boxes=32)
    for bad in (["--crops-out", "d", "--crop-size", "60", "32"], ["--crops-out", "d", "--crop-quality", "0"], ["--crop-pad", "0.1"]):
        with pytest.raises(SystemExit):
            crops_stage.from_arguments(ap, ap.parse_args(bad))
    with pytest.raises(SystemExit):
        ap.parse_args(["--crops-out", "d", "--crop-fit", "crop"])
    assert crops_stage.crop_file_names("frame_007.jpg", np.array([0, 12, 0]), 3) == ["frame_007_0.jpg", "frame_007_id12.jpg", "frame_007_2.jpg"]
    assert crops_stage.crop_file_names("a.b.png", None, 2) == ["a.b_0.jpg", "a.b_1.jpg"]
    from multiposenet_amd import track_frames
    assert "--crops-out DIR" in track_frames.__doc__ and "not\nencoded again" in track_frames.__doc__
