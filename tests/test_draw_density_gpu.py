"""GPU: mpn_draw_density through `density.DensityMap.launch_draw` against tests/density_ref.py's `draw` (which
tests/test_density_host.py holds against Pillow) on the settings of tests/density_cases.py: every byte of the packed RGBA buffer,
the padding between the frames and the bytes behind them included - what the map does not cover is unchanged. The launch is in
place: the frames are filled anew before every launch."""
import numpy as np
import pytest

import density_cases as cases
import density_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64                                                          # bytes behind the last frame, which must stay as they are
MAX_BOXES = 3


def _density(setting, **more):
    from multiposenet_amd.density import DensityMap
    keep = {k: setting[k] for k in ('cell', 'smooth', 'full_scale', 'opacity', 'colormap')}
    return DensityMap(frame_size=setting['size'], max_boxes=MAX_BOXES, **dict(keep, **more))


def _packed(shapes, seed=0):
    """(descriptors, the packed RGBA buffer of seeded frames, [(offset, h, w)])."""
    from multiposenet_amd.inference import draw
    desc, frames, nbytes = draw.layout(shapes, [0] * len(shapes))
    buf = np.random.RandomState(seed).randint(0, 256, nbytes + GUARD).astype(np.uint8)
    for k, (at, h, w) in enumerate(frames):
        buf[at:at + h * w * 4] = cases.background(h, w, seed + k).reshape(-1)
    return desc, buf, frames


def _rows(grids, show='dwell'):
    """mpn_density_map's out for these grids: no persons, the image rows' maxima."""
    out = np.zeros(len(grids) * MAX_BOXES * ref.ROW.itemsize + len(grids) * ref.IMAGE.itemsize, np.uint8)
    images = out[len(grids) * MAX_BOXES * ref.ROW.itemsize:].view(ref.IMAGE)
    images['max_visits' if show == 'visits' else 'max_dwell'] = [most for _, _, most in grids]
    images['max_dwell' if show == 'visits' else 'max_visits'] = 77  # the plane that is not shown says nothing
    return out


def _draw(density, grids, cuda, seed=0, start=None, shapes=None, desc=None, draw=ref.draw):
    """One launch over seeded frames (start: over that buffer instead) -> (the buffer behind it, the buffer before it, what the
    reference makes of it)."""
    import torch
    b = len(grids)
    made, buf, frames = _packed(shapes or [density.frame_size] * b, seed)
    desc = made if desc is None else desc
    if start is not None:
        buf = start
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)       # noqa: E731
    out = up(buf)
    snapshots = np.stack([grid for _, grid, _ in grids]).astype(np.uint32)
    density.launch_draw(up(desc), up(snapshots.reshape(-1).view(np.uint8)), up(_rows(grids, density.show)), out, b)
    want = buf.copy()
    for (at, h, w), (_, grid, most) in zip(frames, grids):
        if (h, w) != density.frame_size:
            continue
        rgba = want[at:at + h * w * 4].reshape(h, w, 4)
        rgba[:] = draw(rgba, grid, most, density.cell, density.smooth, density.full_scale, density.opacity, density.colormap)
    return out.cpu().numpy(), buf, want


@pytest.mark.parametrize("index", range(len(cases.SETTINGS + cases.ONE_CELL)))
def test_each_frame_and_the_batch_equal_the_reference(cuda, index):
    setting = (cases.SETTINGS + cases.ONE_CELL)[index]
    grids = cases.draw_grids(setting)
    density = _density(setting)
    changed = 0
    for k, grid in enumerate(grids):
        got, before, want = _draw(density, [grid], cuda, seed=k)
        np.testing.assert_array_equal(got, want, err_msg=f"{setting} {grid[0]}")
        changed += int((want != before).any())
    assert changed == 2                                             # the empty grid leaves its frame alone
    got, before, want = _draw(density, grids, cuda, seed=100)
    np.testing.assert_array_equal(got, want, err_msg=f"{setting} batch")
    assert got[-GUARD:].tobytes() == before[-GUARD:].tobytes() and (want != before).any()


def test_the_visits_plane_reads_its_own_maximum(cuda):
    setting = cases.SETTINGS[0]
    grids = cases.draw_grids(setting)
    got, before, want = _draw(_density(setting, show='visits'), grids, cuda)
    np.testing.assert_array_equal(got, want)
    assert (want != before).any()


def test_a_frame_of_one_pixel(cuda):
    setting = dict(size=(1, 1), cell=4, smooth=True, full_scale=0, opacity=200, colormap=cases.RAINBOW)
    density = _density(setting)
    for value in (9, 0):
        got, before, want = _draw(density, [('one', np.full((1, 1), value, np.uint32), value)], cuda)
        np.testing.assert_array_equal(got, want)
        assert (want != before).any() == (value > 0)


@pytest.mark.parametrize("smooth", [True, False])
def test_a_large_frame(cuda, smooth):
    """1024 x 1024 at cell = 8, the largest grid: against the array form of the reference, which tests/test_density_host.py holds
    against its loops."""
    setting = dict(size=(1024, 1024), cell=8, smooth=smooth, full_scale=0, opacity=160, colormap=None)
    rng = np.random.RandomState(3)
    grid = (rng.randint(0, 1000, (128, 128)) * (rng.rand(128, 128) < 0.5)).astype(np.uint32)
    grid[:16, :16] = 0                                              # a corner the map leaves alone
    got, before, want = _draw(_density(setting), [('large', grid, int(grid.max()))], cuda, draw=ref.draw_arrays)
    np.testing.assert_array_equal(got, want)
    frame = slice(0, 1024 * 1024 * 4)
    same = (want[frame] == before[frame]).reshape(1024, 1024, 4).all(axis=2)
    assert same[:60, :60].all() and (~same).sum() > 1024 * 1024 // 4


def test_images_that_must_be_left_alone(cuda):
    """A descriptor of another size than the map's frames, and one that reaches outside the buffer: neither image is touched,
    the others are drawn."""
    setting = cases.SETTINGS[2]
    grids = cases.draw_grids(setting)[:2] * 2
    density = _density(setting)
    h, w = setting['size']
    shapes = [(h, w), (h - 1, w), (h, w), (h, w)]
    got, before, want = _draw(density, grids, cuda, shapes=shapes)
    np.testing.assert_array_equal(got, want)
    assert (want != before).any()
    desc, buf, frames = _packed([(h, w)] * 4)
    outside = desc.copy()
    outside.view(np.int64).reshape(4, 4)[3, 1] = (len(buf) + 15) // 16 * 16 - 16        # its last rows lie behind the buffer
    got, before, want = _draw(density, grids, cuda, desc=outside)
    at, _, _ = frames[3]
    want[at:at + h * w * 4] = before[at:at + h * w * 4]
    np.testing.assert_array_equal(got, want)


def test_a_second_launch_blends_again(cuda):
    setting = cases.SETTINGS[0]
    grids = cases.draw_grids(setting)[:1]
    density = _density(setting)
    once, before, want = _draw(density, grids, cuda)
    twice, _, want_twice = _draw(density, grids, cuda, start=once.copy())
    np.testing.assert_array_equal(once, want)
    np.testing.assert_array_equal(twice, want_twice)
    assert (twice != once).any()
