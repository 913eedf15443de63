"""Freeze what the host JPEG entry points answer for damaged input: mpn_jpeg_info, mpn_jpeg_entropy_decode,
mpn_jpeg_scan_prepare, mpn_jpeg_scans_info and mpn_jpeg_scans_decode of the BUILT LIBRARY are run over every file of
jpeg_goldens.npz and jpeg_progressive_goldens.npz (its damaged files included) and over seeded mutations of each, and
their return codes, verdicts and a checksum of every defined output are stored in `tests/golden/jpeg_host_verdicts.npz`.

The inputs are not stored: `files()` and `mutations()` regenerate them from the two archives. Per file, mutation 0 is the file itself,
1 .. HEADER are single-byte replacements in [2, first SOS + 16), the next ANYWHERE are replacements anywhere, the last
PREFIXES are prefixes of the file.

Stored per input: `rc` [5] (ENTRY_POINTS' order), `verdict` [4] (VERDICTS' order, 0 where the call failed) and `crc`, one
CRC32 chained over what the calls define: with rc == 0 the bytes of mpn_jpeg_header, mpn_jpeg_scan_desc and
mpn_jpeg_scans_header, with a decode's rc == 0 its coefficients and its mpn_jpeg_desc. The decode calls get 64 int16
guard words behind coef_bytes, which must survive.

The archive was written by the library as it stood BEFORE the two host parsers became one: it is the record of what each
entry point answered then, and is regenerated only when an answer is changed on purpose.

Run (the library built):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpeg_host_verdicts.py
"""
import ctypes
import os
import sys
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OUT = os.path.join(HERE, "jpeg_host_verdicts.npz")
HEADER, ANYWHERE, PREFIXES = 400, 60, 40
PER_FILE = 1 + HEADER + ANYWHERE + PREFIXES
SEED = 20261018
ENTRY_POINTS = ('mpn_jpeg_info', 'mpn_jpeg_entropy_decode', 'mpn_jpeg_scan_prepare', 'mpn_jpeg_scans_info', 'mpn_jpeg_scans_decode')
VERDICTS = ('supported', 'reason', 'route', 'scans.reason')
GUARD = 0x5A5A


def files():
    """[(name, bytes)]: the baseline goldens, the progressive / CMYK goldens, then the damaged files of the latter."""
    out = []
    with np.load(os.path.join(HERE, "jpeg_goldens.npz")) as z:
        out += [(str(n), z[f"{n}/jpeg"].tobytes()) for n in z["names"]]
    with np.load(os.path.join(HERE, "jpeg_progressive_goldens.npz")) as z:
        out += [(str(n), z[f"{n}/jpeg"].tobytes()) for n in z["names"]]
        out += [(f"damaged/{n}", z[f"damaged/{n}"].tobytes()) for n in z["damaged"]]
    return out


def mutations(index, data):
    """The PER_FILE inputs made from file `index` of `files()`, in mutation order."""
    rng = np.random.RandomState(SEED + index)
    sos = data.find(b"\xff\xda")
    header_end = min((sos if sos >= 0 else len(data)) + 16, len(data))
    out = [data]
    for first, end, count in ((2, header_end, HEADER), (0, len(data), ANYWHERE)):
        for _ in range(count):
            b = bytearray(data)
            b[int(rng.randint(first, end))] = int(rng.randint(0, 256))
            out.append(bytes(b))
    out += [data[:int(n)] for n in rng.randint(0, len(data), PREFIXES)]
    return out


_scratch = [np.empty(64, np.uint16)]     # grow-only: a damaged header may claim 2^28 pixels, and filling that per input is the cost


def _decode(fn, data, total_blocks):
    """A decode entry point with guard words behind coef_bytes -> (rc, the bytes it defined)."""
    from multiposenet_amd.inference import jpeg as J
    if _scratch[0].size < total_blocks * 64 + 64:
        _scratch[0] = np.empty(total_blocks * 64 + 64, np.uint16)
    coefs = _scratch[0][:total_blocks * 64 + 64]        # (a decode that succeeds defines all of it; only the guard is set)
    coefs[-64:] = GUARD
    desc = np.zeros(1, J.DESC)
    rc = fn(data, len(data), coefs.ctypes.data_as(ctypes.c_void_p), total_blocks * 128, desc.ctypes.data_as(ctypes.c_void_p))
    assert (coefs[-64:] == GUARD).all(), "written past coef_bytes"
    return rc, (coefs[:-64].tobytes() + desc.tobytes() if rc == 0 else b"")


def answers(lib, data):
    """One input through the five entry points -> (rc [5], verdict [4], crc)."""
    from multiposenet_amd.inference import jpeg as J
    h, s, p = J._Header(), J._ScansHeader(), np.zeros(1, J.SCAN_DESC)
    rc = [0] * 5
    rc[0] = lib.mpn_jpeg_info(data, len(data), ctypes.byref(h))
    rc[2] = lib.mpn_jpeg_scan_prepare(data, len(data), p.ctypes.data_as(ctypes.c_void_p))
    rc[3] = lib.mpn_jpeg_scans_info(data, len(data), ctypes.byref(s))
    rc[1], one = _decode(lib.mpn_jpeg_entropy_decode, data, h.total_blocks if rc[0] == 0 and h.supported else 0)
    rc[4], many = _decode(lib.mpn_jpeg_scans_decode, data, s.total_blocks if rc[3] == 0 and s.route != 2 else 0)
    defined = (bytes(h) if rc[0] == 0 else b"", one, p.tobytes() if rc[2] == 0 else b"", bytes(s) if rc[3] == 0 else b"", many)
    crc = 0
    for part in defined:
        crc = zlib.crc32(part, crc)
    verdict = [h.supported if rc[0] == 0 else 0, h.reason if rc[0] == 0 else 0, s.route if rc[3] == 0 else 0, s.reason if rc[3] == 0 else 0]
    return rc, verdict, crc


def run():
    """{'names', 'rc' [files, PER_FILE, 5] int8, 'verdict' [files, PER_FILE, 4] int8, 'crc' [files, PER_FILE] uint32}"""
    from multiposenet_amd import _lib
    lib = _lib.lib()
    fs = files()
    rc = np.zeros((len(fs), PER_FILE, 5), np.int8)
    verdict = np.zeros((len(fs), PER_FILE, 4), np.int8)
    crc = np.zeros((len(fs), PER_FILE), np.uint32)
    for i, (_, data) in enumerate(fs):
        for m, bad in enumerate(mutations(i, data)):
            rc[i, m], verdict[i, m], crc[i, m] = answers(lib, bad)
    return {'names': np.array([n for n, _ in fs]), 'rc': rc, 'verdict': verdict, 'crc': crc}


def differ(rc, verdict):
    """Inputs on which the one-scan and the multi-scan entry points do not say the same thing -> bool [files, PER_FILE].
    They agree when both refuse the headers, both decode (route 'device' and supported, the same decode code), or both
    leave the file to a library for the same reason - a 'host-entropy' file being 'progressive' or 'components' to the
    one-scan view."""
    ok1, ok2 = rc[..., 0] == 0, rc[..., 3] == 0
    sup1, sup2 = ok1 & (verdict[..., 0] == 1), ok2 & (verdict[..., 2] == 0)
    same_reason = (verdict[..., 1] == verdict[..., 3]) | ((verdict[..., 2] == 1) & ((verdict[..., 1] == 2) | (verdict[..., 1] == 6)))
    agree = np.where(sup1 | sup2, sup1 & sup2 & (rc[..., 1] == rc[..., 4]), (ok1 == ok2) & (~ok1 | same_reason))
    return ~agree


def save(path, arrays):
    """np.savez_compressed without the clock in it: the same answers give the same file, byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, value in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, value, allow_pickle=False)


def main():
    out = run()
    save(OUT, out)
    share = differ(out['rc'], out['verdict']).mean()
    print("wrote", OUT, out['crc'].size, "inputs of", len(out['names']), "files;", f"{100 * share:.1f} % differ;", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
