"""GPU: mpn_person_crops against the restatement tests/crops_ref.py (held against Pillow on the CPU by
tests/test_person_crops_host.py): every byte of the crops, the info rows and the zeroed unused slots over the handmade cases
for both fits, the same launch replayed from one captured graph over two records, the one-frame host call, and the JPEG files
against Pillow's. Byte for byte throughout."""
import numpy as np
import pytest
import torch

import crops_cases as C
import crops_ref as R

pytestmark = pytest.mark.gpu

MARK = 0xAB                              # the outputs are pre-filled: an unwritten byte shows


def _spec(case, fit, **kw):
    from multiposenet_amd.inference import PersonCrops
    return PersonCrops(size=case['size'], pad=case['pad'], fit=fit, fill=case['fill'], max_boxes=case['max_boxes'], **kw)


def _pack(images):
    offsets = np.concatenate([[0], np.cumsum([im.size for im in images])]).astype(np.int64)
    return np.concatenate([im.reshape(-1) for im in images]), offsets[:-1].tolist()


def _record(boxes, max_boxes):
    from multiposenet_amd.pose_metrics import fill_record
    return fill_record([{'boxes': b, 'scores': np.zeros(len(b), np.float32)} for b in boxes], len(boxes), max_boxes)[0]


def _launch(buffers, images, boxes):
    from multiposenet_amd.inference import crops as crops_stage
    dev = buffers.device
    packed, offsets = _pack(images)
    buffers.place([im.shape[:2] for im in images], offsets)
    buffers.out.fill_(MARK)
    buffers.info.fill_(MARK)
    buffers.launch(torch.from_numpy(packed).to(dev), torch.from_numpy(_record(boxes, buffers.max_boxes)).to(dev))
    torch.cuda.synchronize()
    height, width = buffers.spec.size
    return (buffers.out.cpu().numpy().reshape(buffers.slots, height, width, 3),
            buffers.info.cpu().numpy().view(crops_stage.INFO))


def _want_info(info, spec):
    """The reference's info as the rows mpn_person_crops writes."""
    from multiposenet_amd.inference import crops as crops_stage
    rows = np.zeros(len(info['used']), crops_stage.INFO)
    rows['rect'], rows['placed'] = info['rect'], info['placed']
    rows['flags'] = (info['used'] * crops_stage.USED | info['empty'] * crops_stage.EMPTY | info['too_large'] * crops_stage.TOO_LARGE |
                     info['clipped'] * crops_stage.CLIPPED)
    return rows


def _compare(got, info, want, want_info, spec, msg):
    assert got.shape == want.shape and got.dtype == np.uint8, msg
    diff = (got != want).any(axis=(1, 2, 3))
    assert not diff.any(), (msg, "slots", np.flatnonzero(diff).tolist(), int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    rows = _want_info(want_info, spec)
    for key in ('rect', 'placed', 'flags'):
        assert info[key].tobytes() == rows[key].tobytes(), (msg, key, info[key].tolist(), rows[key].tolist())
    used = want_info['used']
    assert not info[~used].view(np.uint8).any(), (msg, "an unused info row is not zeros")
    assert not got[~used].any(), (msg, "an unused slot is not zeros")
    live = used & ~want_info['empty']
    for s in np.flatnonzero(live):
        x0, y0, x1, y1 = want_info['rect'][s]
        _, _, new_h, new_w = want_info['placed'][s]
        assert (info['ksize_x'][s], info['ksize_y'][s]) == (R.ksize_of(x0, x1, new_w), R.ksize_of(y0, y1, new_h)), (msg, s)


@pytest.fixture(scope="module")
def wanted():
    """The reference over every case and fit, computed once: {(name, fit): (crops, info)}."""
    out = {}
    for c in C.cases():
        for fit in R.FITS:
            out[c['name'], fit] = R.person_crops(c['images'], c['boxes'], len(c['images']) * c['max_boxes'], c['size'], c['pad'], fit,
                                                 c['fill'])
    return out


@pytest.mark.parametrize("fit", R.FITS)
def test_kernel_equals_the_reference_on_every_handmade_case(cuda, wanted, fit):
    from multiposenet_amd.inference.crops import CropBuffers
    seen = {'empty': 0, 'too_large': 0, 'clipped': 0, 'resized': 0}
    for c in C.cases():
        spec = _spec(c, fit)
        buffers = CropBuffers(len(c['images']), c['max_boxes'], spec, torch.device("cuda:0"))
        got, info = _launch(buffers, c['images'], c['boxes'])
        want, want_info = wanted[c['name'], fit]
        _compare(got, info, want, want_info, spec, (c['name'], fit))
        for key in ('empty', 'too_large', 'clipped'):
            seen[key] += int(want_info[key].sum())
        seen['resized'] += int((want_info['used'] & ~want_info['empty'] & ~want_info['too_large']).sum())
    assert seen['empty'] >= 3 and seen['too_large'] >= 1 and seen['clipped'] >= 2 and seen['resized'] >= 25, seen


def test_one_captured_graph_serves_two_records(cuda, wanted):
    """Grids depend on (b, max_boxes, size) alone: the launch captured over one record and batch, replayed over another."""
    from multiposenet_amd.inference.crops import CropBuffers
    cases = {c['name']: c for c in C.cases()}
    first, second = cases["every_slot"], dict(cases["every_slot"])
    second['images'] = [C.frame(91, 37, 53), C.frame(92, 37, 53)]
    second['boxes'] = [cases["inside_fractional"]['boxes'][0], np.zeros((0, 4), np.float32)]
    dev = torch.device("cuda:0")
    spec = _spec(first, 'pad')
    buffers = CropBuffers(2, first['max_boxes'], spec, dev)
    sources = torch.zeros(2 * 37 * 53 * 3, dtype=torch.uint8, device=dev)
    record = torch.zeros(len(_record(first['boxes'], first['max_boxes'])), dtype=torch.uint8, device=dev)

    def put(case):
        packed, offsets = _pack(case['images'])
        buffers.place([im.shape[:2] for im in case['images']], offsets)
        sources.copy_(torch.from_numpy(packed))
        record.copy_(torch.from_numpy(_record(case['boxes'], case['max_boxes'])))
    put(first)
    buffers.launch(sources, record)                                # eager once, then captured
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buffers.launch(sources, record)
    from multiposenet_amd.inference import crops as crops_stage
    for case in (first, second, first):
        put(case)
        buffers.out.fill_(MARK)
        buffers.info.fill_(MARK)
        graph.replay()
        torch.cuda.synchronize()
        got = buffers.out.cpu().numpy().reshape(buffers.slots, 8, 8, 3)
        info = buffers.info.cpu().numpy().view(crops_stage.INFO)
        want, want_info = R.person_crops(case['images'], case['boxes'], buffers.slots, case['size'], case['pad'], 'pad', case['fill'])
        _compare(got, info, want, want_info, spec, "replay")
    assert want_info['used'].all()


@pytest.mark.parametrize("size", [(256, 128), (512, 256), (8, 256)])
def test_crops_at_the_default_and_the_largest_size(cuda, size):
    """Sizes whose tiles take more than 64 KB of LDS (22 and 9 rows a tile), with more than one tile, and one whose tile is the
    whole crop; a box enlarged, one reduced 2.3x and one reduced past 16x on the 300 rows of the frame at 8 output rows."""
    from multiposenet_amd.inference import PersonCrops
    from multiposenet_amd.inference.crops import CropBuffers
    image = C.frame(5, 300, 200)
    boxes = [np.stack([C.box(300, 200, 20.5, 30.25, 120, 90.75), C.box(300, 200, 0, 0, 300, 200), C.box(300, 200, 100, 100, 104, 103),
                       C.box(300, 200, 150, -20, 330, 150)]).astype(np.float32)]
    for fit in R.FITS:
        spec = PersonCrops(size=size, pad=0.05, fit=fit, fill=C.FILL, max_boxes=5)
        got, info = _launch(CropBuffers(1, 5, spec, torch.device("cuda:0")), [image], boxes)
        want, want_info = R.person_crops([image], boxes, 5, size, 0.05, fit, C.FILL)
        _compare(got, info, want, want_info, spec, (size, fit))
        assert want_info['too_large'].any() == (size[0] == 8) and want_info['clipped'].sum() == 2


def test_person_crops_on_result_dicts(cuda, wanted):
    from multiposenet_amd.inference import person_crops
    for name in ("inside_fractional", "pad_clipped", "empty", "tall_and_wide"):
        c = next(c for c in C.cases() if c['name'] == name)
        for fit in R.FITS:
            spec = _spec(c, fit)
            got, info = person_crops(c['images'][0], {'boxes': c['boxes'][0]}, spec)
            n = len(c['boxes'][0])
            want, want_info = wanted[name, fit]
            assert got.shape == (n,) + c['size'] + (3,) and got.dtype == np.uint8
            np.testing.assert_array_equal(got, want[:n], err_msg=f"{name} {fit}")
            assert set(info) == {'rect', 'placed', 'empty', 'too_large', 'clipped'}
            assert info['rect'].dtype == np.float64 and info['placed'].dtype == np.int32 and info['empty'].dtype == np.bool_
            for key in info:
                assert info[key].tobytes() == want_info[key][:n].astype(info[key].dtype).tobytes(), (name, fit, key)
    nobody = person_crops(C.frame(1, 37, 53), {'boxes': np.zeros((0, 4), np.float32)}, spec)
    assert nobody[0].shape == (0,) + c['size'] + (3,) and nobody[1]['rect'].shape == (0, 4) and nobody[1]['empty'].shape == (0,)
    with pytest.raises(ValueError, match="image must be uint8"):
        person_crops(np.zeros((4, 4), np.uint8), {'boxes': np.zeros((0, 4))}, spec)


@pytest.mark.parametrize("quality,sampling", [(75, '4:2:0'), (92, '4:4:4')])
def test_jpeg_files_equal_pillows(cuda, wanted, quality, sampling):
    import io

    from PIL import Image

    from multiposenet_amd.inference import person_crops
    checked = 0
    for name in ("pad_clipped", "tall_and_wide", "three_sizes"):
        c = next(c for c in C.cases() if c['name'] == name)
        spec = _spec(c, 'pad', format='jpeg', jpeg_quality=quality, jpeg_subsampling=sampling)
        files, info = person_crops(c['images'][0], {'boxes': c['boxes'][0]}, spec)
        want, _ = wanted[name, 'pad']
        assert isinstance(files, list) and len(files) == len(c['boxes'][0]) == len(info['empty'])
        for data, pixels in zip(files, want):
            buf = io.BytesIO()
            Image.fromarray(pixels).save(buf, "JPEG", quality=quality, subsampling={'4:4:4': 0, '4:2:0': 2}[sampling])
            assert isinstance(data, bytes) and data == buf.getvalue(), (name, quality, sampling)
            checked += 1
    assert checked >= 6
