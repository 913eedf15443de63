// The host front end of the JPEG decode: ONE marker parser and ONE scan decoder behind every host entry point, in a file
// that compiles as plain C++ (tools/jpeg_host_fuzz.sh builds it so, under ASan + UBSan). The device half is jpeg.hip.
//
//   mpn_jpeg_info, mpn_jpeg_scan_prepare   walk(one_scan) up to the first scan: the verdict (supported / reason), and for
//                                          the second the header descriptor of the device's entropy stage (jpeg_entropy.hip)
//   mpn_jpeg_entropy_decode                walk(one_scan) + the one sequential interleaved scan -> raw int16 coefficients, 64
//                                          per 8x8 block in natural order, one plane of blocks per component; nothing behind
//                                          the scan is read
//   mpn_jpeg_scans_info                    walk(all_scans) up to the first scan: up to four components, route, reason
//   mpn_jpeg_scans_decode                  walk(all_scans) over ALL markers of the file -> the same coefficients. Tables
//                                          (DHT, DQT) and the restart interval (DRI) may change between scans; a component's
//                                          quantisation table is latched at its first scan (the library's rule). A scan is
//                                          one of five kinds - sequential, DC first, DC refinement, AC first, AC refinement
//                                          (T.81 annex G, the arithmetic of the library's jdphuff.c) - over interleaved MCUs
//                                          or, with one component, over the component's own ceil(w / 8) x ceil(h / 8) blocks.
//                                          `bits[c][k]` holds the successive-approximation position every coefficient has
//                                          reached (-1: not seen): a scan must continue it exactly, and the file must bring
//                                          every coefficient to position 0.
//
// The two policies read the same segments with the same readers and differ only in what they JUDGE (frame_reason,
// one_scan_reason against scan_script / first-scan rules) and in where they stop: DESIGN.md, "JPEG host front end", lists
// the inputs on which their verdicts part, and tests/golden/jpeg_host_verdicts.npz holds them fixed.
//
// No HIP call, no global, no allocation; every read is checked against `nbytes`, every block index is inside the padded
// planes by construction. Thread-safe and re-entrant.
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/mpn.h"
#include "jpeg_host.h"

void mpn_set_error(const char* fmt, ...);       // common.h (which needs the HIP headers; this file does not)

#define HOST_REQUIRE(cond, code, ...)      \
    do {                                   \
        if (!(cond)) {                     \
            mpn_set_error(__VA_ARGS__);    \
            return (code);                 \
        }                                  \
    } while (0)

namespace {

using namespace mpn_jpeg_host;

constexpr long long kMaxPixels = 1ll << 28;     // keeps every index of an image in 32 bits (the device checks the same bound)
constexpr int kMaxScans = 100;                  // a script longer than this is refused (Pillow's own limit)

enum Policy {
    one_scan,       // baseline, one interleaved scan of one or three components: stops at (decodes only) the first scan
    all_scans       // also progressive and four components: every scan of the file
};

struct Scan {
    int ns, id[4], comp[4], td[4], ta[4];       // id: as the header names a component; comp: its index in the frame
    int ss, se, ah, al;
};

struct Frame {
    int marker, precision, width, height, ncomp;
    bool progressive, sof, jfif, adobe, q16;
    int adobe_transform;
    int cid[4], hs[4], vs[4], tq[4];
    int bw[4], bh[4];           // padded block grid of each component (whole MCUs)
    int nw[4], nh[4];           // the component's own block grid: what a single-component scan walks
    long long base[5];
    int mcus_x, mcus_y;
    int restart;
    uint16_t q[4][64];          // by table id, natural order
    bool qset[4];
    uint16_t quant[4][64];      // by COMPONENT: its table as latched at its first decoded scan
    uint8_t hbits[2][4][17];
    uint8_t hvals[2][4][256];
    bool hset[2][4];
    Scan first;                 // the first scan and the position of its first entropy-coded byte (once it is accepted)
    size_t scan_pos;
};

// A frame header's fields -> false when the segment is damaged. What the frame is worth is frame_reason's business.
bool read_frame(int m, const uint8_t* s, size_t len, Frame& f) {
    if (f.sof || len < 6) return false;
    f.sof = true;
    f.marker = m;
    f.precision = s[0];
    f.height = (s[1] << 8) | s[2];
    f.width = (s[3] << 8) | s[4];
    const int nf = f.ncomp = s[5];
    if (nf < 1 || len != 6 + 3 * (size_t)nf) return false;
    for (int i = 0; i < nf && i < 4; ++i) {
        f.cid[i] = s[6 + 3 * i];
        f.hs[i] = s[7 + 3 * i] >> 4;
        f.vs[i] = s[7 + 3 * i] & 15;
        f.tq[i] = s[8 + 3 * i];
    }
    return true;
}

// The frame under a policy -> reason (MPN_JPEG_SUPPORTED: a frame the policy decodes, once the first scan is known; then
// the block grids are laid out). The ORDER of the checks is part of what the entry points answer.
int frame_reason(Frame& f, Policy policy) {
    const int m = f.marker, nf = f.ncomp;
    if (policy == one_scan && m == 0xC2) return MPN_JPEG_PROGRESSIVE;
    if (m >= 0xC9) return MPN_JPEG_ARITHMETIC;
    if (m != 0xC0 && m != 0xC1 && m != 0xC2) return MPN_JPEG_FRAME_TYPE;      // lossless, hierarchical
    f.progressive = m == 0xC2;
    if (f.precision != 8) return MPN_JPEG_PRECISION;
    if (f.width < 1 || f.height < 1) return MPN_JPEG_MALFORMED;               // (height 0 = a DNL marker follows: not handled)
    if (nf != 1 && nf != 3 && !(policy == all_scans && nf == 4)) return MPN_JPEG_COMPONENTS;
    for (int i = 0; i < nf; ++i) {
        if (f.hs[i] < 1 || f.hs[i] > 4 || f.vs[i] < 1 || f.vs[i] > 4 || f.tq[i] > 3) return MPN_JPEG_MALFORMED;
        for (int j = 0; j < i && policy == all_scans; ++j) {     // (a scan of this policy finds its components by id)
            if (f.cid[j] == f.cid[i]) return MPN_JPEG_MALFORMED;
        }
    }
    if (nf == 1) {
        f.hs[0] = f.vs[0] = 1;          // a single component is never interleaved: its factors do not matter
    } else {
        const bool first_ok = (f.hs[0] == 1 && f.vs[0] == 1) || (nf == 3 && f.hs[0] == 2 && (f.vs[0] == 1 || f.vs[0] == 2));
        if (!first_ok) return MPN_JPEG_SAMPLING;
        for (int i = 1; i < nf; ++i) {
            if (f.hs[i] != 1 || f.vs[i] != 1) return MPN_JPEG_SAMPLING;
        }
    }
    if ((long long)f.width * f.height > kMaxPixels) return MPN_JPEG_TOO_LARGE;
    f.mcus_x = (f.width + 8 * f.hs[0] - 1) / (8 * f.hs[0]);
    f.mcus_y = (f.height + 8 * f.vs[0] - 1) / (8 * f.vs[0]);
    long long at = 0;
    for (int c = 0; c < 4; ++c) {
        f.base[c] = at;
        if (c >= nf) continue;
        f.bw[c] = f.mcus_x * f.hs[c];
        f.bh[c] = f.mcus_y * f.vs[c];
        const int cw = (f.width * f.hs[c] + f.hs[0] - 1) / f.hs[0], ch = (f.height * f.vs[c] + f.vs[0] - 1) / f.vs[0];
        f.nw[c] = (cw + 7) / 8;
        f.nh[c] = (ch + 7) / 8;
        at += (long long)f.bw[c] * f.bh[c];
    }
    f.base[4] = at;
    return MPN_JPEG_SUPPORTED;
}

// DQT / DHT / DRI / APP0 / APP14 -> false when the segment is damaged
bool read_tables(int m, const uint8_t* s, size_t len, Frame& f) {
    if (m == 0xDB) {
        size_t i = 0;
        while (i < len) {
            const int pq = s[i] >> 4, tq = s[i] & 15;
            ++i;
            if (tq > 3 || pq > 1 || i + (pq ? 128u : 64u) > len) return false;
            if (pq) f.q16 = true;
            for (int k = 0; k < 64; ++k) f.q[tq][kNatural[k]] = pq ? (uint16_t)((s[i + 2 * k] << 8) | s[i + 2 * k + 1]) : s[i + k];
            f.qset[tq] = true;
            i += pq ? 128 : 64;
        }
    } else if (m == 0xC4) {
        size_t i = 0;
        while (i < len) {
            if (i + 17 > len) return false;
            const int tc = s[i] >> 4, th = s[i] & 15;
            if (tc > 1 || th > 3) return false;
            int count = 0;
            f.hbits[tc][th][0] = 0;
            for (int l = 1; l <= 16; ++l) {
                f.hbits[tc][th][l] = s[i + l];
                count += s[i + l];
            }
            i += 17;
            if (count > 256 || i + count > len) return false;
            memset(f.hvals[tc][th], 0, 256);
            memcpy(f.hvals[tc][th], s + i, count);
            f.hset[tc][th] = true;
            i += count;
        }
    } else if (m == 0xDD) {
        if (len != 2) return false;
        f.restart = (s[0] << 8) | s[1];
    } else if (m == 0xE0) {
        if (len >= 5 && memcmp(s, "JFIF", 5) == 0) f.jfif = true;
    } else if (m == 0xEE) {
        if (len >= 12 && memcmp(s, "Adobe", 5) == 0) {
            f.adobe = true;
            f.adobe_transform = s[11];
        }
    }
    return true;
}

// What is known at the first scan: the colour space the library would choose, 8-bit tables
int colour_reason(const Frame& f) {
    if (f.q16) return MPN_JPEG_DQT16;
    if (f.ncomp == 3) {
        if (f.adobe && f.adobe_transform != 1) return MPN_JPEG_COLORSPACE;
        if (!f.jfif && !f.adobe && f.cid[0] == 'R' && f.cid[1] == 'G' && f.cid[2] == 'B') return MPN_JPEG_COLORSPACE;
    }
    if (f.ncomp == 4 && !(f.adobe && f.adobe_transform == 0)) return MPN_JPEG_COLORSPACE;     // YCCK, or CMYK that is not inverted
    return MPN_JPEG_SUPPORTED;
}

// An SOS header's fields -> false when the segment does not have the shape of one
bool read_scan(const uint8_t* s, size_t len, Scan& sc) {
    if (len < 1) return false;
    sc.ns = s[0];
    if (sc.ns < 1 || sc.ns > 4 || len != 4 + 2 * (size_t)sc.ns) return false;
    for (int i = 0; i < sc.ns; ++i) {
        sc.id[i] = s[1 + 2 * i];
        sc.td[i] = s[2 + 2 * i] >> 4;
        sc.ta[i] = s[2 + 2 * i] & 15;
    }
    sc.ss = s[1 + 2 * sc.ns];
    sc.se = s[2 + 2 * sc.ns];
    sc.ah = s[3 + 2 * sc.ns] >> 4;
    sc.al = s[3 + 2 * sc.ns] & 15;
    return true;
}

// all_scans: the scan against the frame -> false when it names a script the standard does not allow
bool scan_script(const Frame& f, Scan& sc) {
    if (sc.ns > f.ncomp) return false;
    for (int i = 0; i < sc.ns; ++i) {
        int c = -1;
        for (int j = 0; j < f.ncomp; ++j) {
            if (f.cid[j] == sc.id[i]) c = j;
        }
        if (c < 0 || (i > 0 && c <= sc.comp[i - 1])) return false;         // components of a scan come in frame order
        sc.comp[i] = c;
        if (sc.td[i] > 3 || sc.ta[i] > 3) return false;
    }
    if (!f.progressive) return sc.ss == 0 && sc.se == 63 && sc.ah == 0 && sc.al == 0;
    if (sc.ss > sc.se || sc.se > 63 || sc.al > 13) return false;
    if (sc.ss == 0 ? sc.se != 0 : sc.ns != 1) return false;                  // DC alone, or a band of ONE component
    return sc.ah == 0 || sc.al == sc.ah - 1;
}

// one_scan: the first scan against the frame -> reason. It must be THE scan: every component, in the frame's order, with
// its tables in place. (Again the order is part of the answer; all_scans leaves a missing table to the decode.)
int one_scan_reason(const Frame& f, Scan& sc) {
    if (sc.ns != f.ncomp) return MPN_JPEG_MULTISCAN;
    for (int i = 0; i < sc.ns; ++i) {
        if (sc.id[i] != f.cid[i] || sc.td[i] > 3 || sc.ta[i] > 3) return MPN_JPEG_MALFORMED;
        if (!f.hset[0][sc.td[i]] || !f.hset[1][sc.ta[i]] || !f.qset[f.tq[i]]) return MPN_JPEG_MALFORMED;
        sc.comp[i] = i;
    }
    if (sc.ss != 0 || sc.se != 63 || sc.ah != 0 || sc.al != 0) return MPN_JPEG_MALFORMED;
    return colour_reason(f);
}

struct Coder {
    Bits b;
    unsigned eobrun;
    int pred[4];
};

inline void top_up(Bits& b) {
    if (b.n < 32) b.refill();
}

inline bool dc_first(Coder& k, const HuffTable& t, int c, int al, int16_t* blk) {
    top_up(k.b);
    const int s = k.b.decode(t);
    if (s < 0 || s > 11) return false;
    if (s) k.pred[c] = (int)((unsigned)k.pred[c] + (unsigned)extend(k.b.get(s), s));
    blk[0] = (int16_t)((unsigned)k.pred[c] << al);
    return true;
}

inline void dc_refine(Coder& k, int al, int16_t* blk) {
    top_up(k.b);
    if (k.b.get(1)) blk[0] = (int16_t)(blk[0] | (1 << al));
}

inline bool ac_first(Coder& k, const HuffTable& t, int ss, int se, int al, int16_t* blk) {
    if (k.eobrun > 0) {
        --k.eobrun;
        return true;
    }
    for (int i = ss; i <= se; ++i) {
        top_up(k.b);
        const int rs = k.b.decode(t);
        if (rs < 0) return false;
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            i += r;
            if (i > se) return false;
            blk[kNatural[i]] = (int16_t)((unsigned)extend(k.b.get(s), s) << al);
        } else if (r == 15) {
            i += 15;
        } else {                                    // an end-of-band run of 2^r + (r bits) blocks, this one included
            k.eobrun = 1u << r;
            if (r) {
                top_up(k.b);
                k.eobrun += k.b.get(r);
            }
            --k.eobrun;
            break;
        }
    }
    return true;
}

// one correction bit of a coefficient that is already non-zero
inline void correct(Coder& k, int16_t& v, int p1) {
    top_up(k.b);
    if (k.b.get(1) && (v & p1) == 0) v = (int16_t)(v >= 0 ? v + p1 : v - p1);
}

inline bool ac_refine(Coder& k, const HuffTable& t, int ss, int se, int al, int16_t* blk) {
    const int p1 = 1 << al;
    int i = ss;
    if (k.eobrun == 0) {
        for (; i <= se; ++i) {
            top_up(k.b);
            const int rs = k.b.decode(t);
            if (rs < 0) return false;
            int r = rs >> 4;
            int s = rs & 15;
            if (s) {
                if (s != 1) return false;           // a refinement scan adds coefficients of magnitude 1 only
                top_up(k.b);
                s = k.b.get(1) ? p1 : -p1;
            } else if (r != 15) {
                k.eobrun = 1u << r;
                if (r) {
                    top_up(k.b);
                    k.eobrun += k.b.get(r);
                }
                break;                              // the rest of the band below, as part of the run
            }
            // skip r zero coefficients (16 for ZRL), correcting every non-zero one on the way
            for (; i <= se; ++i) {
                int16_t& v = blk[kNatural[i]];
                if (v != 0) {
                    correct(k, v, p1);
                } else if (--r < 0) {
                    break;
                }
            }
            if (s) {
                if (i > se) return false;
                blk[kNatural[i]] = (int16_t)s;
            }
        }
    }
    if (k.eobrun > 0) {
        for (; i <= se; ++i) {
            int16_t& v = blk[kNatural[i]];
            if (v != 0) correct(k, v, p1);
        }
        --k.eobrun;
    }
    return true;
}

// One scan's entropy-coded data from `pos` on. Returns "" or what is wrong; `pos` becomes where the reader stopped.
template <bool sequential>
const char* decode_scan(const uint8_t* data, size_t n, size_t& pos, const Frame& f, const Scan& sc, int16_t* coefs) {
    HuffTable dc[4], ac[4];
    const bool need_dc = sequential || (sc.ss == 0 && sc.ah == 0), need_ac = sequential || sc.ss > 0;
    for (int i = 0; i < sc.ns; ++i) {
        if (need_dc && (!f.hset[0][sc.td[i]] || !build_table(f.hbits[0][sc.td[i]], f.hvals[0][sc.td[i]], dc[i]))) {
            return "a DC Huffman table is missing or not a prefix code";
        }
        if (need_ac && (!f.hset[1][sc.ta[i]] || !build_table(f.hbits[1][sc.ta[i]], f.hvals[1][sc.ta[i]], ac[i]))) {
            return "an AC Huffman table is missing or not a prefix code";
        }
    }
    Coder k;
    k.b = {data + pos, data + n, 0, 0, 0, false};
    k.eobrun = 0;
    memset(k.pred, 0, sizeof(k.pred));
    const bool interleaved = sc.ns > 1;
    const int c0 = sc.comp[0];
    const int units_x = interleaved ? f.mcus_x : f.nw[c0], units_y = interleaved ? f.mcus_y : f.nh[c0];
    const long long units = (long long)units_x * units_y;
    int ux = 0, uy = 0, until_restart = f.restart;
    for (long long u = 0; u < units; ++u) {
        if (f.restart && until_restart == 0) {
            // a restart: the coder was flushed to a byte boundary and an RSTn marker follows (the reader stops in front of it)
            if (k.b.overran()) return "a scan ends before its restart interval does";
            const uint8_t* q = k.b.p;
            while (q + 1 < k.b.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
            if (!(q + 1 < k.b.end && q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) return "restart marker missing";
            k.b = {q + 2, data + n, 0, 0, 0, false};
            k.eobrun = 0;
            memset(k.pred, 0, sizeof(k.pred));
            until_restart = f.restart;
        }
        for (int i = 0; i < sc.ns; ++i) {
            const int c = sc.comp[i];
            const int ch = interleaved ? f.hs[c] : 1, cv = interleaved ? f.vs[c] : 1;
            for (int v = 0; v < cv; ++v) {
                for (int h = 0; h < ch; ++h) {
                    // (uy * cv + v < bh[c] and ux * ch + h < bw[c]: nw <= bw, nh <= bh, whole MCUs)
                    int16_t* blk = coefs + (f.base[c] + (long long)(uy * cv + v) * f.bw[c] + (ux * ch + h)) * 64;
                    bool ok = true;
                    if (sequential) {
                        ok = decode_block(k.b, dc[i], ac[i], k.pred[c], blk);
                    } else if (sc.ss == 0) {
                        if (sc.ah == 0) {
                            ok = dc_first(k, dc[i], c, sc.al, blk);
                        } else {
                            dc_refine(k, sc.al, blk);
                        }
                    } else {
                        ok = sc.ah == 0 ? ac_first(k, ac[i], sc.ss, sc.se, sc.al, blk) : ac_refine(k, ac[i], sc.ss, sc.se, sc.al, blk);
                    }
                    if (!ok) return "damaged entropy-coded data";
                }
            }
        }
        --until_restart;
        if (++ux == units_x) {
            ux = 0;
            ++uy;
        }
    }
    if (k.b.overran()) return "a scan ends before the image does";
    if (k.eobrun > 0) return "an end-of-band run reaches past the scan";
    pos = (size_t)(k.b.p - data);
    return "";
}

// Walks the markers from the start under a policy. With coefs == nullptr it stops at the first scan (f.first, f.scan_pos);
// else it decodes the first scan (one_scan) or every scan (all_scans). reason: MPN_JPEG_* of the file; on
// MPN_JPEG_SUPPORTED with coefs the planes are complete and f.quant holds every component's table.
int walk(Policy policy, const uint8_t* data, size_t n, Frame& f, int& reason, int16_t* coefs, size_t coef_bytes, const char*& what) {
    memset(&f, 0, sizeof(f));
    reason = MPN_JPEG_MALFORMED;
    what = "not a JPEG stream, or its headers are damaged";
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return MPN_ERR_BAD_DATA;
    int8_t bits[4][64];                 // successive-approximation position reached; -1: not seen
    memset(bits, -1, sizeof(bits));
    bool latched[4] = {false, false, false, false};
    int scans = 0;
    size_t pos = 2;
    for (;;) {
        // the next marker: (after a scan) bytes that are not one are skipped, as the library does
        while (pos + 1 < n && !(data[pos] == 0xFF && data[pos + 1] != 0x00 && data[pos + 1] != 0xFF)) {
            if (scans == 0 && data[pos] != 0xFF) return MPN_ERR_BAD_DATA;      // in the headers a segment follows a segment
            ++pos;
        }
        if (pos + 1 >= n) break;
        const int m = data[pos + 1];
        pos += 2;
        if (m == 0xD9) break;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD8) return MPN_ERR_BAD_DATA;
        if (pos + 2 > n) return MPN_ERR_BAD_DATA;
        const size_t L = ((size_t)data[pos] << 8) | data[pos + 1];
        if (L < 2 || pos + L > n) return MPN_ERR_BAD_DATA;
        const uint8_t* s = data + pos + 2;
        const size_t len = L - 2;
        pos += L;
        if (m == 0xCC) {
            reason = MPN_JPEG_ARITHMETIC;
            return MPN_OK;
        }
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            const int r = read_frame(m, s, len, f) ? frame_reason(f, policy) : MPN_JPEG_MALFORMED;
            if (r == MPN_JPEG_MALFORMED) return MPN_ERR_BAD_DATA;
            if (r != MPN_JPEG_SUPPORTED) {
                reason = r;
                return MPN_OK;
            }
            continue;
        }
        if (m != 0xDA) {
            if (!read_tables(m, s, len, f)) return MPN_ERR_BAD_DATA;
            continue;
        }
        // ---- a scan
        Scan sc;
        if (!f.sof || !read_scan(s, len, sc)) return MPN_ERR_BAD_DATA;
        int r = MPN_JPEG_SUPPORTED;
        if (policy == one_scan) {
            r = one_scan_reason(f, sc);
        } else if (!scan_script(f, sc)) {
            what = "a scan header is damaged, or its script is not one the standard allows";
            r = MPN_JPEG_MALFORMED;
        } else if (scans == 0) {        // what is known at the first scan
            r = !f.progressive && sc.ns != f.ncomp ? MPN_JPEG_MULTISCAN : colour_reason(f);
        }
        if (r == MPN_JPEG_MALFORMED) return MPN_ERR_BAD_DATA;
        if (r != MPN_JPEG_SUPPORTED) {
            reason = r;
            return MPN_OK;
        }
        if (scans == 0) {
            f.first = sc;
            f.scan_pos = pos;
            if (!coefs) {
                reason = MPN_JPEG_SUPPORTED;
                return MPN_OK;
            }
            if (coef_bytes < (size_t)f.base[4] * 128) {
                what = "coef_bytes is smaller than total_blocks * 128";
                return MPN_ERR_WORKSPACE;
            }
            memset(coefs, 0, (size_t)f.base[4] * 128);
        }
        if (++scans > kMaxScans || f.q16) {
            what = "more scans than a decoder accepts, or a 16-bit quantisation table behind the first scan";
            return MPN_ERR_BAD_DATA;
        }
        for (int i = 0; i < sc.ns; ++i) {
            const int c = sc.comp[i];
            if (!latched[c]) {
                if (!f.qset[f.tq[c]]) {
                    what = "a quantisation table is missing";
                    return MPN_ERR_BAD_DATA;
                }
                memcpy(f.quant[c], f.q[f.tq[c]], sizeof(f.quant[c]));
                latched[c] = true;
            }
            // the script: this scan continues, coefficient by coefficient, what the scans before it left
            if (!f.progressive) {
                if (bits[c][0] >= 0) {
                    what = "a component is coded twice";
                    return MPN_ERR_BAD_DATA;
                }
                memset(bits[c], 0, 64);
                continue;
            }
            if (sc.ss > 0 && bits[c][0] < 0) {
                what = "a scan script codes a band before the component's DC";
                return MPN_ERR_BAD_DATA;
            }
            for (int k = sc.ss; k <= sc.se; ++k) {
                const int expected = bits[c][k] < 0 ? 0 : bits[c][k];
                if (sc.ah != expected || (sc.ah == 0 && bits[c][k] >= 0)) {
                    what = "a scan script refines a band that was never started, or starts one twice";
                    return MPN_ERR_BAD_DATA;
                }
                bits[c][k] = (int8_t)sc.al;
            }
        }
        const char* err = f.progressive ? decode_scan<false>(data, n, pos, f, sc, coefs) : decode_scan<true>(data, n, pos, f, sc, coefs);
        if (err[0]) {
            what = err;
            return MPN_ERR_BAD_DATA;
        }
        if (policy == one_scan) break;  // its whole image; what follows the scan is never read
    }
    if (scans == 0) return MPN_ERR_BAD_DATA;                    // no scan at all: damaged
    for (int c = 0; c < f.ncomp; ++c) {
        for (int k = 0; k < 64; ++k) {
            if (bits[c][k] != 0) {
                what = "the file ends before every coefficient has all its bits (scans are missing)";
                return MPN_ERR_BAD_DATA;
            }
        }
    }
    reason = MPN_JPEG_SUPPORTED;
    return MPN_OK;
}

// The geometry of a decoded frame and its (up to three) latched tables, for both decode entry points
void fill_desc(const Frame& f, mpn_jpeg_desc* desc) {
    memset(desc, 0, sizeof(*desc));
    desc->width = f.width;
    desc->height = f.height;
    desc->components = f.ncomp;
    desc->h_samp = f.hs[0];
    desc->v_samp = f.vs[0];
    desc->total_blocks = (int32_t)f.base[4];
    for (int c = 0; c < f.ncomp && c < 3; ++c) {
        desc->blocks_w[c] = f.bw[c];
        desc->blocks_h[c] = f.bh[c];
        memcpy(desc->quant[c], f.quant[c], sizeof(desc->quant[c]));
    }
}

}  // namespace

extern "C" int mpn_jpeg_info(const uint8_t* data, size_t nbytes, mpn_jpeg_header* out) {
    HOST_REQUIRE(data && out, MPN_ERR_BAD_ARG, "jpeg_info: null pointer");
    Frame f;
    int reason;
    const char* what;
    const int rc = walk(one_scan, data, nbytes, f, reason, nullptr, 0, what);
    memset(out, 0, sizeof(*out));
    out->width = f.width;
    out->height = f.height;
    out->components = f.ncomp;
    out->h_samp = f.hs[0];
    out->v_samp = f.vs[0];
    out->restart_interval = f.restart;
    out->supported = reason == MPN_JPEG_SUPPORTED;
    out->reason = reason;
    HOST_REQUIRE(rc == MPN_OK, rc, "jpeg_info: %s", what);
    if (out->supported) {
        for (int c = 0; c < f.ncomp; ++c) {
            out->blocks_w[c] = f.bw[c];
            out->blocks_h[c] = f.bh[c];
        }
        out->total_blocks = (int32_t)f.base[4];
        out->coef_bytes = f.base[4] * 128;
    }
    return MPN_OK;
}

extern "C" int mpn_jpeg_entropy_decode(const uint8_t* data, size_t nbytes, int16_t* coefs, size_t coef_bytes, mpn_jpeg_desc* desc) {
    HOST_REQUIRE(data && coefs && desc, MPN_ERR_BAD_ARG, "jpeg_entropy_decode: null pointer");
    Frame f;
    int reason;
    const char* what;
    const int rc = walk(one_scan, data, nbytes, f, reason, coefs, coef_bytes, what);
    HOST_REQUIRE(rc == MPN_OK, rc, "jpeg_entropy_decode: %s", what);
    HOST_REQUIRE(reason == MPN_JPEG_SUPPORTED, MPN_ERR_BAD_DATA, "jpeg_entropy_decode: stream not supported (reason %d, see MPN_JPEG_*)", reason);
    fill_desc(f, desc);
    return MPN_OK;
}

// The marker scan as a descriptor for the device's entropy stage (jpeg_entropy.hip): headers only, the scan's bytes untouched.
extern "C" size_t mpn_jpeg_scan_desc_bytes(void) { return sizeof(mpn_jpeg_scan_desc); }

extern "C" int mpn_jpeg_scan_prepare(const uint8_t* data, size_t nbytes, mpn_jpeg_scan_desc* out) {
    HOST_REQUIRE(data && out, MPN_ERR_BAD_ARG, "jpeg_scan_prepare: null pointer");
    Frame f;
    int reason;
    const char* what;
    const int rc = walk(one_scan, data, nbytes, f, reason, nullptr, 0, what);
    if (reason == MPN_JPEG_SUPPORTED && nbytes > (size_t)MPN_JPEG_MAX_FILE_BYTES) reason = MPN_JPEG_TOO_LARGE;
    memset(out, 0, sizeof(*out));
    out->nbytes = (int64_t)nbytes;
    out->width = f.width;
    out->height = f.height;
    out->components = f.ncomp;
    out->h_samp = f.hs[0];
    out->v_samp = f.vs[0];
    out->restart_interval = f.restart;
    out->supported = reason == MPN_JPEG_SUPPORTED;
    out->reason = reason;
    HOST_REQUIRE(rc == MPN_OK, rc, "jpeg_scan_prepare: %s", what);
    if (!out->supported) return MPN_OK;
    out->scan_offset = (int64_t)f.scan_pos;
    out->total_blocks = (int32_t)f.base[4];
    for (int c = 0; c < f.ncomp; ++c) {
        out->blocks_w[c] = f.bw[c];
        out->blocks_h[c] = f.bh[c];
        out->dc_table[c] = f.first.td[c];
        out->ac_table[c] = f.first.ta[c];
        memcpy(out->quant[c], f.q[f.tq[c]], sizeof(out->quant[c]));
    }
    for (int tc = 0; tc < 2; ++tc) {
        for (int th = 0; th < 4; ++th) {
            if (!f.hset[tc][th]) continue;
            memcpy(out->huff_bits[tc][th], f.hbits[tc][th] + 1, 16);
            memcpy(out->huff_vals[tc][th], f.hvals[tc][th], 256);
        }
    }
    return MPN_OK;
}

extern "C" int mpn_jpeg_scans_info(const uint8_t* data, size_t nbytes, mpn_jpeg_scans_header* out) {
    HOST_REQUIRE(data && out, MPN_ERR_BAD_ARG, "jpeg_scans_info: null pointer");
    Frame f;
    int reason;
    const char* what;
    const int rc = walk(all_scans, data, nbytes, f, reason, nullptr, 0, what);
    memset(out, 0, sizeof(*out));
    out->width = f.width;
    out->height = f.height;
    out->components = f.ncomp;
    out->h_samp = f.hs[0];
    out->v_samp = f.vs[0];
    out->progressive = f.progressive;
    out->reason = reason;
    out->route = reason != MPN_JPEG_SUPPORTED ? MPN_JPEG_ROUTE_LIBRARY
                 : !f.progressive && f.ncomp != 4 ? MPN_JPEG_ROUTE_DEVICE : MPN_JPEG_ROUTE_HOST_ENTROPY;
    HOST_REQUIRE(rc == MPN_OK, rc, "jpeg_scans_info: %s", what);
    if (reason == MPN_JPEG_SUPPORTED) {
        for (int c = 0; c < f.ncomp; ++c) {
            out->blocks_w[c] = f.bw[c];
            out->blocks_h[c] = f.bh[c];
        }
        out->total_blocks = (int32_t)f.base[4];
        out->coef_bytes = f.base[4] * 128;
    }
    return MPN_OK;
}

extern "C" int mpn_jpeg_scans_decode(const uint8_t* data, size_t nbytes, int16_t* coefs, size_t coef_bytes, mpn_jpeg_desc* desc) {
    HOST_REQUIRE(data && coefs && desc, MPN_ERR_BAD_ARG, "jpeg_scans_decode: null pointer");
    Frame f;
    int reason;
    const char* what;
    const int rc = walk(all_scans, data, nbytes, f, reason, coefs, coef_bytes, what);
    HOST_REQUIRE(rc == MPN_OK, rc, "jpeg_scans_decode: %s", what);
    HOST_REQUIRE(reason == MPN_JPEG_SUPPORTED, MPN_ERR_BAD_DATA, "jpeg_scans_decode: stream not supported (reason %d, see MPN_JPEG_*)", reason);
    fill_desc(f, desc);
    if (f.ncomp == 4) {
        // the descriptor holds three tables: the fourth component names the one of them it shares (Pillow and the usual
        // writers give all four one table)
        desc->blocks_w3 = f.bw[3];
        desc->blocks_h3 = f.bh[3];
        desc->quant3 = -1;
        for (int c = 2; c >= 0; --c) {
            if (memcmp(f.quant[3], f.quant[c], sizeof(f.quant[3])) == 0) desc->quant3 = c;
        }
        HOST_REQUIRE(desc->quant3 >= 0, MPN_ERR_BAD_DATA,
                     "jpeg_scans_decode: stream not supported (the fourth component has a quantisation table of its own)");
    }
    return MPN_OK;
}
