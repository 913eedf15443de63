"""Case table of the JPEG goldens: (name, seed, (height, width), content, mode, quality, extra `Image.save` arguments).

content: 'smooth' (gradients), 'noise' (uniform random bytes), 'flat' (one colour: DC-only blocks), 'checker' (a saturated
0 / 255 checkerboard, one pixel per square: the inverse DCT overshoots the 8-bit range). mode: '444', '422', '420' (Pillow's
subsampling 0, 1, 2), 'L' (grayscale), and the two streams the device path must classify and leave to the library:
'progressive' and 'cmyk'."""
import numpy as np

SUBSAMPLING = {'444': 0, '422': 1, '420': 2}
UNSUPPORTED = {'progressive': 'progressive', 'cmyk': 'components'}     # mode -> jpeg_info's reason

CASES = [
    ("1x1_420", 1, (1, 1), 'noise', '420', 75, {}),
    ("1x1_gray", 2, (1, 1), 'noise', 'L', 75, {}),
    ("8x8_444", 3, (8, 8), 'noise', '444', 95, {}),
    ("8x8_420_flat", 4, (8, 8), 'flat', '420', 75, {}),
    ("5x7_422", 5, (5, 7), 'noise', '422', 75, {}),
    ("5x7_420", 6, (5, 7), 'smooth', '420', 30, {}),
    ("17x17_420", 7, (17, 17), 'noise', '420', 95, {}),
    ("17x17_422", 8, (17, 17), 'smooth', '422', 100, {}),
    ("17x17_444_checker", 9, (17, 17), 'checker', '444', 100, {}),
    ("16x33_420_checker", 10, (16, 33), 'checker', '420', 75, {}),
    ("16x33_422_opt", 11, (16, 33), 'noise', '422', 75, {'optimize': True}),
    ("16x33_gray_checker", 12, (16, 33), 'checker', 'L', 30, {}),
    ("37x53_420_opt", 13, (37, 53), 'noise', '420', 30, {'optimize': True}),
    ("37x53_444", 14, (37, 53), 'smooth', '444', 75, {}),
    ("37x53_422_rst_blocks", 15, (37, 53), 'noise', '422', 95, {'restart_marker_blocks': 3}),
    ("37x53_gray", 16, (37, 53), 'smooth', 'L', 95, {}),
    ("48x64_420_rst_rows", 17, (48, 64), 'noise', '420', 75, {'restart_marker_rows': 1}),
    ("48x64_420_flat", 18, (48, 64), 'flat', '420', 100, {}),
    ("48x64_444_q100", 19, (48, 64), 'noise', '444', 100, {}),
    ("48x64_gray_rst", 20, (48, 64), 'noise', 'L', 75, {'restart_marker_blocks': 5, 'optimize': True}),
    ("120x160_420", 21, (120, 160), 'smooth', '420', 75, {}),
    ("120x160_420_noise_rst", 22, (120, 160), 'noise', '420', 30, {'restart_marker_rows': 2}),
    ("120x160_422_checker", 23, (120, 160), 'checker', '422', 95, {}),
    ("3x5_420", 24, (3, 5), 'noise', '420', 95, {}),
    ("2x4_422", 25, (2, 4), 'noise', '422', 95, {}),
    ("48x64_progressive", 26, (48, 64), 'smooth', 'progressive', 75, {}),
    ("17x17_cmyk", 27, (17, 17), 'noise', 'cmyk', 75, {}),
]


def source(seed, shape, content):
    """The seeded uint8 [h, w, 3] image a case encodes."""
    h, w = shape
    rng = np.random.RandomState(seed)
    if content == 'noise':
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if content == 'flat':
        return np.broadcast_to(rng.randint(0, 256, 3).astype(np.uint8), (h, w, 3)).copy()
    yy, xx = np.mgrid[0:h, 0:w]
    if content == 'checker':
        return np.repeat((((xx + yy) & 1) * 255)[:, :, None], 3, axis=2).astype(np.uint8)
    if content == 'smooth':
        ph = rng.rand(3) * 6.0
        return np.stack([127.5 + 127.5 * np.sin(ph[0] + xx / 9.0), 127.5 + 127.5 * np.cos(ph[1] + yy / 7.0),
                         127.5 + 127.5 * np.sin(ph[2] + (xx + yy) / 13.0)], axis=2).astype(np.uint8)
    raise ValueError(content)
