"""GPU: mpn_draw_trails through `trails.TrackTrails.launch_draw` against tests/trails_ref.py's `draw` (which
tests/test_trails_host.py holds against Pillow) on the table of tests/trails_cases.py: every byte of the packed RGBA buffer,
the padding between the frames and the bytes behind them included - what no segment covers is unchanged. The launch is in
place: the frames are filled anew before every launch."""
import numpy as np
import pytest

import trails_cases as cases
import trails_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64                                                          # bytes behind the last frame, which must stay as they are


def _trails(setting, max_boxes):
    from multiposenet_amd.trails import TrackTrails
    return TrackTrails(frame_size=(33, 67), max_boxes=max_boxes, **setting)


def _packed(images, seed=0):
    """(descriptors, the packed RGBA buffer of seeded frames, [(offset, h, w)])."""
    from multiposenet_amd.inference import draw
    shapes = [(im['h'], im['w']) for im in images]
    desc, frames, nbytes = draw.layout(shapes, [0] * len(shapes))
    buf = np.random.RandomState(seed).randint(0, 256, nbytes + GUARD).astype(np.uint8)
    for k, (at, h, w) in enumerate(frames):
        buf[at:at + h * w * 4] = cases.background(h, w, seed + k).reshape(-1)
    return desc, buf, frames


def _expected(buf, frames, images, setting, rows_of_image=None):
    want = buf.copy()
    for k, ((at, h, w), im) in enumerate(zip(frames, images)):
        keep = len(im['track_ids']) if rows_of_image is None else rows_of_image[k]
        t = {key: value[:keep] for key, value in im['trails'].items()}
        rgba = want[at:at + h * w * 4].reshape(h, w, 4)
        ref.draw(rgba, t, im['track_ids'][:keep], setting['length'], cases.palette_of(setting), setting['fade'], setting['min_alpha'])
    return want


def _draw(trails, images, cuda, header=None, seed=0, start=None):
    """One launch over the images' seeded frames (start: over that buffer instead) -> (the buffer behind it, the buffer before
    it, the frames' places)."""
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    from multiposenet_amd.trails import rows_of
    from multiposenet_amd.zones import track_rows_of
    b = len(images)
    outputs = [{'scores': np.zeros(len(im['track_ids']), np.float32), 'track_ids': im['track_ids'], 'trails': im['trails']}
               for im in images]
    record, _ = fill_record(outputs, b, trails.max_boxes)
    if header is not None:
        record[:4 * (1 + b)].view(np.int32)[:] = header
    desc, buf, frames = _packed(images, seed)
    if start is not None:
        buf = start
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)       # noqa: E731
    out = up(buf)
    trails.launch_draw(up(desc), up(record), up(track_rows_of(outputs, b, trails.max_boxes)),
                       up(rows_of(outputs, b, trails.max_boxes, trails.length)), out, b)
    return out.cpu().numpy(), buf, frames


@pytest.mark.parametrize("index", range(len(cases.SETTINGS)))
def test_each_frame_and_the_ragged_batch_equal_the_reference(cuda, index):
    setting = cases.SETTINGS[index]
    images = cases.draw_images(setting)
    trails = _trails(setting, 8)
    changed = 0
    for k, im in enumerate(images):                                 # 1x1, 5x7 and 33x67, each alone
        got, before, frames = _draw(trails, [im], cuda, seed=k)
        want = _expected(before, frames, [im], setting)
        np.testing.assert_array_equal(got, want, err_msg=f"{setting} {im['name']}")
        changed += int((want != before).any())
    assert changed >= 6
    got, before, frames = _draw(trails, images, cuda, seed=100)     # and all of them as one ragged batch
    want = _expected(before, frames, images, setting)
    np.testing.assert_array_equal(got, want, err_msg=f"{setting} ragged")
    assert got[-GUARD:].tobytes() == before[-GUARD:].tobytes()


def test_the_launch_blends_again_on_frames_it_already_drew(cuda):
    """In place and not idempotent with fade: a second launch over its own output is the reference applied twice."""
    setting = cases.SETTINGS[0]
    im = cases.draw_images(setting)[6]                              # 33x67, handmade
    trails = _trails(setting, 8)
    got, before, frames = _draw(trails, [im], cuda)
    once = _expected(before, frames, [im], setting)
    twice = _expected(once, frames, [im], setting)
    assert (once != twice).any() and got.tobytes() == once.tobytes()
    again, _, _ = _draw(trails, [im], cuda, start=got)
    np.testing.assert_array_equal(again, twice)


def test_one_slot_per_image(cuda):
    setting = dict(length=5, fade=True, min_alpha=64, palette=None)
    images = []
    for k, (h, w) in enumerate(cases.SIZES):
        ids, t = cases.trails_of(5, [(k + 1, True, [(w - 1, h - 1), (0.5, 0.5), (w / 2, 0), (w, h / 2)])])
        images.append({'h': h, 'w': w, 'track_ids': ids, 'trails': t})
    got, before, frames = _draw(_trails(setting, 1), images, cuda)
    want = _expected(before, frames, images, setting)
    assert (want != before).any()
    np.testing.assert_array_equal(got, want)


def test_64_images_of_64_slots_at_length_64(cuda):
    """The largest launch: 4096 rows, every slot of every image a trail, a few of them full rings of 65 points."""
    K = 64
    setting = dict(length=K, fade=True, min_alpha=0, palette=None)
    rng = np.random.RandomState(5)
    images = []
    for k in range(64):
        h, w = cases.SIZES[2] if k % 21 == 0 else (cases.SIZES[0] if k == 1 else cases.SIZES[1])
        persons = []
        for r in range(64):
            n = K + 1 if r % 16 == k % 16 else int(rng.randint(0, 4))
            pts = np.round(rng.uniform(-0.25, 1.25, (n, 2)) * (w, h) * 2) / 2
            persons.append((int(rng.randint(1, 500)), bool(r % 7), [tuple(p) for p in pts]))
        ids, t = cases.trails_of(K, persons)
        images.append({'h': h, 'w': w, 'track_ids': ids, 'trails': t})
    got, before, frames = _draw(_trails(setting, 64), images, cuda)
    want = _expected(before, frames, images, setting)
    assert sum(int((want[at:at + h * w * 4] != before[at:at + h * w * 4]).any()) for at, h, w in frames) >= 60
    np.testing.assert_array_equal(got, want)


def test_a_header_that_names_more_rows_than_the_record_holds(cuda):
    """The counts are clamped to max_boxes and the total to b * max_boxes; a total below the counts cuts the last image short."""
    setting = cases.SETTINGS[0]
    images = [im for im in cases.draw_images(setting) if im['name'].endswith('#0')][1:]      # 5x7 and 33x67, 8 rows each
    assert [len(im['track_ids']) for im in images] == [8, 8]
    trails = _trails(setting, 8)
    honest, before, frames = _draw(trails, images, cuda)
    want = _expected(before, frames, images, setting)
    np.testing.assert_array_equal(honest, want)
    got, _, _ = _draw(trails, images, cuda, header=[1 << 30, 100, 1 << 20])
    np.testing.assert_array_equal(got, want)
    got, _, _ = _draw(trails, images, cuda, header=[-5, 8, 8])
    np.testing.assert_array_equal(got, before)
    got, _, _ = _draw(trails, images, cuda, header=[9, 8, 8])       # the second image has one row: its first trail
    np.testing.assert_array_equal(got, _expected(before, frames, images, setting, rows_of_image=[8, 1]))


def test_a_descriptor_outside_the_buffer_leaves_the_frame_alone(cuda):
    import torch
    from multiposenet_amd.pose_metrics import fill_record
    from multiposenet_amd.trails import rows_of
    from multiposenet_amd.zones import track_rows_of
    setting = cases.SETTINGS[0]
    im = cases.draw_images(setting)[6]
    trails = _trails(setting, 8)
    outputs = [{'scores': np.zeros(8, np.float32), 'track_ids': im['track_ids'], 'trails': im['trails']}]
    record, _ = fill_record(outputs, 1, 8)
    desc, buf, frames = _packed([im])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)       # noqa: E731
    for bad in ((4, 34), (5, 68), (4, 0), (5, -1)):                 # a frame that is larger than the buffer holds; no frame
        d = desc.copy()
        d[0, bad[0]] = bad[1]
        out = up(buf[:len(buf) - GUARD])
        trails.launch_draw(up(d), up(record), up(track_rows_of(outputs, 1, 8)), up(rows_of(outputs, 1, 8, 5)), out, 1)
        assert out.cpu().numpy().tobytes() == buf[:len(buf) - GUARD].tobytes(), bad
