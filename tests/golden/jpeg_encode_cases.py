"""Case table of the JPEG-encode goldens: (name, seed, (height, width), content, subsampling, quality, channels).

content: 'noise' (uniform random bytes), 'ramp' (smooth gradients), 'binary' (every byte 0 or 255 at random: saturates the DCT
range, fills the scan with 0xFF bytes and, at quality 100, reaches AC symbols of size 10). channels 4: an RGBA source with a
random alpha that the encoder must ignore; its yardstick is Pillow on `convert("RGB")`."""
import numpy as np

SUBSAMPLING = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}
SIZES = [(1, 1), (8, 8), (9, 9), (16, 16), (17, 23), (24, 8), (8, 24), (33, 65), (40, 56), (50, 31)]
CONTENTS = ('noise', 'ramp', 'binary')
QUALITIES = (10, 75, 95, 100)


def _table():
    cases, k = [], 0
    for size in SIZES:
        for sub in SUBSAMPLING:
            content, quality = CONTENTS[(k + k // 3) % 3], QUALITIES[k % 4]
            cases.append((f"{size[0]}x{size[1]}_{sub.replace(':', '')}_{content}_q{quality}", 100 + k, size, content, sub, quality, 3))
            k += 1
    cases += [
        ("120x160_444_binary_q100", 200, (120, 160), 'binary', '4:4:4', 100, 3),
        ("120x160_420_binary_q100", 201, (120, 160), 'binary', '4:2:0', 100, 3),
        ("33x65_420_binary_q100", 202, (33, 65), 'binary', '4:2:0', 100, 3),
        ("40x56_420_noise_q10", 203, (40, 56), 'noise', '4:2:0', 10, 3),
        ("40x56_422_ramp_q10", 204, (40, 56), 'ramp', '4:2:2', 10, 3),
        ("17x23_420_rgba_q75", 205, (17, 23), 'noise', '4:2:0', 75, 4),
        ("50x31_444_rgba_q95", 206, (50, 31), 'ramp', '4:4:4', 95, 4),
    ]
    return cases


CASES = _table()


def source(seed, shape, content, channels=3):
    """The seeded uint8 [h, w, channels] image a case encodes."""
    h, w = shape
    rng = np.random.RandomState(seed)
    if content == 'noise':
        rgb = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    elif content == 'binary':
        rgb = (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    elif content == 'ramp':
        yy, xx = np.mgrid[0:h, 0:w]
        ph = rng.rand(3) * 6.0
        rgb = np.stack([127.5 + 127.5 * np.sin(ph[0] + xx / 9.0), 127.5 + 127.5 * np.cos(ph[1] + yy / 7.0),
                        127.5 + 127.5 * np.sin(ph[2] + (xx + yy) / 13.0)], axis=2).astype(np.uint8)
    else:
        raise ValueError(content)
    if channels == 4:
        alpha = rng.randint(0, 255, (h, w, 1)).astype(np.uint8)          # never 255: an encoder that blends would show
        rgb = np.concatenate([rgb, alpha], axis=2)
    return rgb
