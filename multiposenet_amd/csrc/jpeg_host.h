// What the JPEG host front end (jpeg_host.hip) decodes with: the zigzag table, Huffman tables with a 9-bit lookahead, the
// bit reader and one sequential block. Plain C++ (no HIP): a host-only program can include it.
#ifndef MPN_JPEG_HOST_H_
#define MPN_JPEG_HOST_H_
#include <stdint.h>
#include <stddef.h>
#include <string.h>

namespace mpn_jpeg_host {

// zigzag position -> natural (row-major) position
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLook = 9;

struct HuffTable {
    uint16_t look[1 << kLook];      // (code length << 8) | symbol of the code that starts these 9 bits; 0 = longer than 9
    int32_t maxcode[18];            // largest code of each length (-1: none)
    int32_t valoff[17];             // index of a length's first symbol minus its first code
    uint8_t vals[256];
};

inline bool build_table(const uint8_t* bits, const uint8_t* vals, HuffTable& t) {
    memset(t.look, 0, sizeof(t.look));
    memcpy(t.vals, vals, 256);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
            if (l <= kLook) {
                const int first = code << (kLook - l), count = 1 << (kLook - l);
                if (first + count > (1 << kLook)) return false;
                for (int j = 0; j < count; ++j) t.look[first + j] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        if (code > (1 << l)) return false;          // more codes than the length has
        t.maxcode[l] = bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    return true;
}

// The entropy-coded segment as a bit stream: a 64-bit buffer holding `n` unread bits in its low end. Byte stuffing (FF 00) is
// removed on the way in; a marker or the end of the data stops the input and zero bits follow, counted in `fake`.
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf;
    int n, fake;
    bool stopped;

    inline void refill() {
        while (n <= 56) {
            if (!stopped && n <= 32 && end - p >= 4) {           // four plain bytes at once
                uint32_t v;
                memcpy(&v, p, 4);
                if (((~v - 0x01010101u) & v & 0x80808080u) == 0) {   // no byte is FF
                    buf = (buf << 32) | __builtin_bswap32(v);
                    n += 32;
                    p += 4;
                    continue;
                }
            }
            if (!stopped && p < end) {
                const unsigned c = *p;
                if (c == 0xFF) {
                    if (p + 1 >= end || p[1] != 0) {
                        stopped = true;
                        continue;
                    }
                    p += 2;
                } else {
                    ++p;
                }
                buf = (buf << 8) | c;
                n += 8;
            } else {
                stopped = true;
                buf <<= 8;
                n += 8;
                fake += 8;
            }
        }
    }
    inline unsigned get(int s) {                    // 1 <= s <= 16, n >= s
        n -= s;
        return (unsigned)(buf >> n) & ((1u << s) - 1u);
    }
    inline int decode(const HuffTable& t) {         // n >= 16
        const unsigned e = t.look[(unsigned)(buf >> (n - kLook)) & ((1u << kLook) - 1u)];
        if (e) {
            n -= (int)(e >> 8);
            return (int)(e & 255u);
        }
        int l = kLook + 1;
        int32_t code = (int32_t)((buf >> (n - l)) & ((1u << l) - 1u));
        while (l <= 16 && code > t.maxcode[l]) {
            ++l;
            code = (int32_t)((buf >> (n - l)) & ((1u << l) - 1u));
        }
        if (l > 16) return -1;
        n -= l;
        return t.vals[(code + t.valoff[l]) & 255];
    }
    inline bool overran() const { return n < fake; }     // zero bits that are not in the stream were consumed
};

inline int extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

inline bool decode_block(Bits& b, const HuffTable& dc, const HuffTable& ac, int& pred, int16_t* out) {
    if (b.n < 32) b.refill();
    int s = b.decode(dc);
    if (s < 0 || s > 11) return false;
    if (s) pred = (int)((unsigned)pred + (unsigned)extend(b.get(s), s));
    out[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        if (b.n < 32) b.refill();
        const int rs = b.decode(ac);
        if (rs < 0) return false;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return false;
            out[kNatural[k]] = (int16_t)extend(b.get(s), s);
            ++k;
        } else {
            if (r != 15) break;             // end of block
            k += 16;
        }
    }
    return true;
}

}  // namespace mpn_jpeg_host
#endif
