"""Case table of the progressive / CMYK JPEG goldens: (name, seed, (height, width), content, mode, quality, extra
`Image.save` arguments), the smallest shapes that reach every branch of the multi-scan host stage and of the four-component
device path.

content: as jpeg_cases.py ('noise', 'smooth', 'checker', 'flat': one colour, so every AC band is one long end-of-band run).
mode: 'p444', 'p422', 'p420' (progressive RGB at Pillow's subsampling 0, 1, 2), 'pL' (progressive grayscale), 'cmyk' (baseline
Adobe CMYK) and 'pcmyk' (progressive Adobe CMYK). Every progressive case appears with optimize=False and optimize=True.
Restart intervals (restart_marker_blocks) are chosen so that they do not divide the MCU row, nor the block row of the
single-component scans; restart_marker_rows makes Pillow redefine DRI between scans.

DAMAGED: (name, the case it is made from, kind, which): 'cut' = the file ends in the middle of the entropy-coded data of
scan `which`; 'flip' = one byte in the middle of the `which`-th AC refinement scan is inverted."""
from jpeg_cases import source  # noqa: F401  (the maker and the tests take it from here)

SUBSAMPLING = {'p444': 0, 'p422': 1, 'p420': 2}

_BASE = [
    ("1x1_p420", 101, (1, 1), 'noise', 'p420', 75, {}),
    ("1x1_pL", 102, (1, 1), 'noise', 'pL', 75, {}),
    ("8x8_p444", 103, (8, 8), 'noise', 'p444', 95, {}),
    ("8x8_p420_checker", 104, (8, 8), 'checker', 'p420', 30, {}),
    ("17x17_p420", 105, (17, 17), 'noise', 'p420', 95, {}),
    ("17x17_p422", 106, (17, 17), 'smooth', 'p422', 75, {}),
    ("17x17_p444_checker", 107, (17, 17), 'checker', 'p444', 30, {}),
    ("17x17_pL", 108, (17, 17), 'noise', 'pL', 95, {}),
    ("17x17_p444_rst5", 109, (17, 17), 'noise', 'p444', 75, {'restart_marker_blocks': 5}),
    ("37x53_p422", 110, (37, 53), 'noise', 'p422', 30, {}),
    ("37x53_p444", 111, (37, 53), 'smooth', 'p444', 95, {}),
    ("37x53_p420_checker", 112, (37, 53), 'checker', 'p420', 75, {}),
    ("37x53_pL", 113, (37, 53), 'smooth', 'pL', 30, {}),
    ("37x53_p420_rst3", 114, (37, 53), 'noise', 'p420', 95, {'restart_marker_blocks': 3}),
    ("37x53_p422_rst_rows", 115, (37, 53), 'noise', 'p422', 95, {'restart_marker_rows': 1}),
    ("37x53_pL_rst3", 116, (37, 53), 'noise', 'pL', 75, {'restart_marker_blocks': 3}),
    ("120x160_p420", 117, (120, 160), 'smooth', 'p420', 75, {}),
    ("120x160_p444", 118, (120, 160), 'noise', 'p444', 95, {}),
    ("120x160_p422_checker", 119, (120, 160), 'checker', 'p422', 30, {}),
    ("120x160_p420_flat", 120, (120, 160), 'flat', 'p420', 75, {}),
    ("17x17_pcmyk", 121, (17, 17), 'noise', 'pcmyk', 75, {}),
    ("37x53_pcmyk", 122, (37, 53), 'smooth', 'pcmyk', 95, {}),
    ("17x17_pcmyk_rst2", 123, (17, 17), 'noise', 'pcmyk', 30, {'restart_marker_blocks': 2}),
]

CASES = []
for _name, _seed, _shape, _content, _mode, _quality, _extra in _BASE:
    CASES.append((_name, _seed, _shape, _content, _mode, _quality, dict(_extra, optimize=False)))
    CASES.append((_name + "_opt", _seed, _shape, _content, _mode, _quality, dict(_extra, optimize=True)))
CASES += [
    ("17x17_cmyk", 131, (17, 17), 'noise', 'cmyk', 75, {}),
    ("37x53_cmyk", 132, (37, 53), 'smooth', 'cmyk', 95, {}),
    ("37x53_cmyk_opt_rst", 133, (37, 53), 'checker', 'cmyk', 30, {'optimize': True, 'restart_marker_blocks': 3}),
]

DAMAGED_FROM = "37x53_p420_rst3"
DAMAGED = [(f"cut_scan{k}", DAMAGED_FROM, 'cut', k) for k in range(10)] + [("flip_ac_refine", DAMAGED_FROM, 'flip', 0)]


def scans(data):
    """[(Ss, Se, Ah, Al, number of components, first entropy-coded byte, one past the last)] of every scan of a JPEG."""
    out, pos = [], 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        if m == 0xD9:
            break
        length = (data[pos + 2] << 8) | data[pos + 3]
        if m != 0xDA:
            pos += 2 + length
            continue
        ns = data[pos + 4]
        ss, se, a = data[pos + 5 + 2 * ns], data[pos + 6 + 2 * ns], data[pos + 7 + 2 * ns]
        start = end = pos + 2 + length
        while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
            end += 1
        out.append((ss, se, a >> 4, a & 15, ns, start, end))
        pos = end
    return out


def damage(data, kind, which):
    """The damaged file of one DAMAGED entry, made from the bytes of its case."""
    sc = scans(data)
    if kind == 'cut':
        return data[:(sc[which][5] + sc[which][6]) // 2]
    refine = [s for s in sc if s[0] > 0 and s[2] > 0]
    at = (refine[which][5] + refine[which][6]) // 2
    return data[:at] + bytes([data[at] ^ 0xFF]) + data[at + 1:]

