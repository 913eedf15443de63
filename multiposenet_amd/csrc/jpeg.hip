// Baseline JPEG decode split in two ("hybrid"): the serial part on the host, the parallel part on the device, the result equal
// byte for byte to what libjpeg(-turbo) - and so Pillow - returns for the same bytes.
//
//   HOST   mpn_jpeg_info            marker scan: geometry, sampling, restart interval, supported / reason
//          mpn_jpeg_entropy_decode  Huffman decode of the one interleaved scan -> raw int16 coefficients, 64 per 8x8 block in
//                                   natural order, one plane of blocks per component + a fixed-size descriptor
//          (no HIP call, no globals: thread-safe and re-entrant; every read is checked against `nbytes`; Huffman tables
//          and the bit reader live in jpeg_host.h, shared with the multi-scan stage of jpeg_scans.hip)
//   DEVICE mpn_jpeg_decode          jpeg_idct_kernel    dequantise + 8x8 inverse DCT -> uint8 component planes in `work`
//                                   jpeg_colour_kernel  "fancy" chroma upsampling + YCbCr->RGB -> packed HWC uint8 at src_offset
//                                   (four components - Adobe CMYK, coefficients from jpeg_scans.hip - : four planes, and
//                                   Pillow's inversion and CMYK->RGB in place of YCbCr->RGB)
//
// The arithmetic is libjpeg's, all integer:
//   - inverse DCT: the "slow integer" method (13-bit constants, 2 extra bits after pass 1, COLUMNS first, then rows),
//     descale = (x + 2^(n-1)) >> n, +128 and the range limit through the 10-bit index of the library's table;
//   - chroma: the triangle filter of h2v1 / h2v2 "fancy" upsampling with its alternating rounding constants, edges taken at
//     the component's TRUE down-sampled size; a component of width <= 2 is replicated (the library's own rule);
//   - colour: the 16-bit fixed-point YCbCr->RGB tables with their rounding terms.
#include "common.h"
#include "jpeg_host.h"
#include <string.h>

namespace {

typedef mpn_jpeg_desc Desc;
static_assert(sizeof(Desc) == MPN_JPEG_DESC_BYTES, "descriptor layout is part of the ABI");

constexpr long long kMaxPixels = 1ll << 28;    // keeps every index of an image in 32 bits

using namespace mpn_jpeg_host;

// ------------------------------------------------------------------------------------------------ host: markers
struct Parsed {
    int width, height, ncomp;
    int cid[3], hs[3], vs[3], tq[3], td[3], ta[3];
    int restart;
    bool jfif, adobe, sof, q16;
    int adobe_transform;
    uint16_t q[4][64];                  // natural order
    bool qset[4];
    uint8_t hbits[2][4][17];            // [class][id]: codes per length 1..16
    uint8_t hvals[2][4][256];
    bool hset[2][4];
    size_t scan_pos;                    // first entropy-coded byte
};

// Scans the markers up to the first scan. Returns the reason code (MPN_JPEG_SUPPORTED = 0: a stream the device path decodes).
int parse(const uint8_t* data, size_t n, Parsed& p) {
    memset(&p, 0, sizeof(p));
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return MPN_JPEG_MALFORMED;
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n || data[pos] != 0xFF) return MPN_JPEG_MALFORMED;
        while (pos < n && data[pos] == 0xFF) ++pos;          // fill bytes
        if (pos >= n) return MPN_JPEG_MALFORMED;
        const int m = data[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // stand-alone markers
        if (m == 0x00 || m == 0xD8 || m == 0xD9) return MPN_JPEG_MALFORMED;
        if (pos + 2 > n) return MPN_JPEG_MALFORMED;
        const size_t L = ((size_t)data[pos] << 8) | data[pos + 1];
        if (L < 2 || pos + L > n) return MPN_JPEG_MALFORMED;
        const uint8_t* s = data + pos + 2;
        const size_t len = L - 2;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {      // a frame header
            if (p.sof || len < 6) return MPN_JPEG_MALFORMED;
            p.sof = true;
            const int precision = s[0], nf = s[5];
            p.height = (s[1] << 8) | s[2];
            p.width = (s[3] << 8) | s[4];
            p.ncomp = nf;
            if (len != 6 + 3 * (size_t)nf || nf < 1) return MPN_JPEG_MALFORMED;
            for (int i = 0; i < nf && i < 3; ++i) {
                p.cid[i] = s[6 + 3 * i];
                p.hs[i] = s[7 + 3 * i] >> 4;
                p.vs[i] = s[7 + 3 * i] & 15;
                p.tq[i] = s[8 + 3 * i];
            }
            if (m == 0xC2) return MPN_JPEG_PROGRESSIVE;
            if (m >= 0xC9) return MPN_JPEG_ARITHMETIC;
            if (m != 0xC0 && m != 0xC1) return MPN_JPEG_FRAME_TYPE;      // lossless, hierarchical
            if (precision != 8) return MPN_JPEG_PRECISION;
            if (p.width < 1 || p.height < 1) return MPN_JPEG_MALFORMED;  // (height 0 = a DNL marker follows: not handled)
            if (nf != 1 && nf != 3) return MPN_JPEG_COMPONENTS;
            for (int i = 0; i < nf; ++i) {
                if (p.hs[i] < 1 || p.hs[i] > 4 || p.vs[i] < 1 || p.vs[i] > 4 || p.tq[i] > 3) return MPN_JPEG_MALFORMED;
            }
            if (nf == 3) {
                const bool luma_ok = (p.hs[0] == 1 && p.vs[0] == 1) || (p.hs[0] == 2 && p.vs[0] == 1) || (p.hs[0] == 2 && p.vs[0] == 2);
                if (!luma_ok || p.hs[1] != 1 || p.vs[1] != 1 || p.hs[2] != 1 || p.vs[2] != 1) return MPN_JPEG_SAMPLING;
            } else {
                p.hs[0] = p.vs[0] = 1;      // a single component is never interleaved: its factors do not matter
            }
            if ((long long)p.width * p.height > kMaxPixels) return MPN_JPEG_TOO_LARGE;
        } else if (m == 0xCC) {
            return MPN_JPEG_ARITHMETIC;
        } else if (m == 0xDB) {             // quantisation tables
            size_t i = 0;
            while (i < len) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                ++i;
                if (tq > 3 || pq > 1 || i + (pq ? 128u : 64u) > len) return MPN_JPEG_MALFORMED;
                if (pq) p.q16 = true;
                for (int k = 0; k < 64; ++k) {
                    p.q[tq][kNatural[k]] = pq ? (uint16_t)((s[i + 2 * k] << 8) | s[i + 2 * k + 1]) : s[i + k];
                }
                p.qset[tq] = true;
                i += pq ? 128 : 64;
            }
        } else if (m == 0xC4) {             // Huffman tables
            size_t i = 0;
            while (i < len) {
                if (i + 17 > len) return MPN_JPEG_MALFORMED;
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return MPN_JPEG_MALFORMED;
                int count = 0;
                p.hbits[tc][th][0] = 0;
                for (int l = 1; l <= 16; ++l) {
                    p.hbits[tc][th][l] = s[i + l];
                    count += s[i + l];
                }
                i += 17;
                if (count > 256 || i + count > len) return MPN_JPEG_MALFORMED;
                memset(p.hvals[tc][th], 0, 256);
                memcpy(p.hvals[tc][th], s + i, count);
                p.hset[tc][th] = true;
                i += count;
            }
        } else if (m == 0xDD) {
            if (len != 2) return MPN_JPEG_MALFORMED;
            p.restart = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {
            if (len >= 5 && memcmp(s, "JFIF", 5) == 0) p.jfif = true;
        } else if (m == 0xEE) {
            if (len >= 12 && memcmp(s, "Adobe", 5) == 0) {
                p.adobe = true;
                p.adobe_transform = s[11];
            }
        } else if (m == 0xDA) {             // the scan
            if (!p.sof || len < 1) return MPN_JPEG_MALFORMED;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || len != 4 + 2 * (size_t)ns) return MPN_JPEG_MALFORMED;
            if (ns != p.ncomp) return MPN_JPEG_MULTISCAN;
            for (int i = 0; i < ns; ++i) {
                if (s[1 + 2 * i] != p.cid[i]) return MPN_JPEG_MALFORMED;
                p.td[i] = s[2 + 2 * i] >> 4;
                p.ta[i] = s[2 + 2 * i] & 15;
                if (p.td[i] > 3 || p.ta[i] > 3 || !p.hset[0][p.td[i]] || !p.hset[1][p.ta[i]] || !p.qset[p.tq[i]]) return MPN_JPEG_MALFORMED;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return MPN_JPEG_MALFORMED;
            if (p.q16) return MPN_JPEG_DQT16;
            if (p.ncomp == 3) {
                // libjpeg's colour-space guess: anything but YCbCr is left to the library
                if (p.adobe && p.adobe_transform != 1) return MPN_JPEG_COLORSPACE;
                if (!p.jfif && !p.adobe && p.cid[0] == 'R' && p.cid[1] == 'G' && p.cid[2] == 'B') return MPN_JPEG_COLORSPACE;
            }
            p.scan_pos = pos + L;
            return MPN_JPEG_SUPPORTED;
        }
        pos += L;
    }
}

struct Geometry {
    int ncomp, hs, vs;
    int bw[3], bh[3];       // padded block grid of each component
    long long base[4];      // first block of each component's plane; base[ncomp] = all blocks
};

void geometry_of(const Parsed& p, Geometry& g) {
    g.ncomp = p.ncomp;
    g.hs = p.hs[0];
    g.vs = p.vs[0];
    const int mx = (p.width + 8 * g.hs - 1) / (8 * g.hs), my = (p.height + 8 * g.vs - 1) / (8 * g.vs);
    long long at = 0;
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = g.bh[c] = 0;
        g.base[c] = at;
        if (c < g.ncomp) {
            g.bw[c] = mx * (c == 0 ? g.hs : 1);
            g.bh[c] = my * (c == 0 ? g.vs : 1);
            at += (long long)g.bw[c] * g.bh[c];
        }
    }
    g.base[3] = at;
    if (g.ncomp == 1) g.base[1] = g.base[2] = at;
}

void fill_info(const Parsed& p, int reason, mpn_jpeg_header* out) {
    memset(out, 0, sizeof(*out));
    out->width = p.width;
    out->height = p.height;
    out->components = p.ncomp;
    out->h_samp = p.hs[0];
    out->v_samp = p.vs[0];
    out->restart_interval = p.restart;
    out->supported = reason == MPN_JPEG_SUPPORTED;
    out->reason = reason;
    if (reason == MPN_JPEG_SUPPORTED) {
        Geometry g;
        geometry_of(p, g);
        for (int c = 0; c < 3; ++c) {
            out->blocks_w[c] = g.bw[c];
            out->blocks_h[c] = g.bh[c];
        }
        out->total_blocks = g.base[3];
        out->coef_bytes = g.base[3] * 128;
    }
}

// ------------------------------------------------------------------------------------------------ device
struct DevGeometry {
    int ncomp, hs, vs, total;
    int bw[4], bh[4], base[4];  // (base[c] = total for a component the image does not have)
    int cw, ch;                 // true size of a chroma component
};

// The geometry of a descriptor, recomputed from (width, height, components, sampling) alone, and every range it makes the
// kernels touch: false = the image is skipped.
__device__ __forceinline__ bool dev_geometry(const Desc& d, DevGeometry& g, size_t coef_bytes, size_t work_bytes, size_t sources_bytes) {
    if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535 || (long long)d.width * d.height > kMaxPixels) return false;
    if (d.components != 1 && d.components != 3 && d.components != 4) return false;
    const bool samp_ok = (d.h_samp == 1 && d.v_samp == 1) || (d.components == 3 && d.h_samp == 2 && (d.v_samp == 1 || d.v_samp == 2));
    if (!samp_ok) return false;
    if (d.components == 4 && (d.quant3 < 0 || d.quant3 > 2)) return false;      // the table the fourth component shares
    g.ncomp = d.components;
    g.hs = d.h_samp;
    g.vs = d.v_samp;
    const int mx = (d.width + 8 * g.hs - 1) / (8 * g.hs), my = (d.height + 8 * g.vs - 1) / (8 * g.vs);
    g.bw[0] = mx * g.hs;
    g.bh[0] = my * g.vs;
    g.base[0] = 0;
    g.base[1] = g.bw[0] * g.bh[0];
    g.bw[1] = g.bw[2] = g.ncomp >= 3 ? mx : 0;
    g.bh[1] = g.bh[2] = g.ncomp >= 3 ? my : 0;
    g.bw[3] = g.ncomp == 4 ? mx : 0;
    g.bh[3] = g.ncomp == 4 ? my : 0;
    g.base[2] = g.base[1] + g.bw[1] * g.bh[1];
    g.base[3] = g.base[2] + g.bw[2] * g.bh[2];
    g.total = g.base[3] + g.bw[3] * g.bh[3];
    g.cw = (d.width + g.hs - 1) / g.hs;
    g.ch = (d.height + g.vs - 1) / g.vs;
    if (d.src_offset < 0 || d.coef_offset < 0 || d.work_offset < 0 || ((d.src_offset | d.coef_offset | d.work_offset) & 15)) return false;
    if ((unsigned long long)d.coef_offset + (unsigned long long)g.total * 128ull > coef_bytes) return false;
    if ((unsigned long long)d.work_offset + (unsigned long long)g.total * 64ull > work_bytes) return false;
    return (unsigned long long)d.src_offset + (unsigned long long)d.width * d.height * 3ull <= sources_bytes;
}

// One pass of the slow-integer inverse DCT over 8 values (jidctint.c): CONST_BITS = 13.
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8], int shift) {
    const int round = 1 << (shift - 1);
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * (-15137);
    int tmp3 = z1 + z2 * 6270;
    z2 = in[0];
    z3 = in[4];
    int tmp0 = (z2 + z3) * 8192;
    int tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 *= -16069;
    z4 *= -3196;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    out[0] = (tmp10 + tmp3 + round) >> shift;
    out[7] = (tmp10 - tmp3 + round) >> shift;
    out[1] = (tmp11 + tmp2 + round) >> shift;
    out[6] = (tmp11 - tmp2 + round) >> shift;
    out[2] = (tmp12 + tmp1 + round) >> shift;
    out[5] = (tmp12 - tmp1 + round) >> shift;
    out[3] = (tmp13 + tmp0 + round) >> shift;
    out[4] = (tmp13 - tmp0 + round) >> shift;
}

// +128 and the library's range-limit table, which is indexed with the low 10 bits: a sign-extended 10-bit value, clamped
__device__ __forceinline__ unsigned range_limit(int v) {
    const int s = ((v & 1023) ^ 512) - 512;
    return (unsigned)min(max(s + 128, 0), 255);
}

constexpr int kThreads = 256;
constexpr int kSlots = kThreads / 8;        // 8x8 blocks of a workgroup: eight lanes each
constexpr int kIdctGroups = 128;            // workgroups per image (grid-stride over the image's blocks)
constexpr int kColourGroups = 256;

// Eight lanes per 8x8 block: lane r loads coefficient row r (16 bytes) and dequantises it; rows meet columns through LDS
// (lane c runs pass 1 on column c and writes it back in place), then lane r runs pass 2 on row r and stores 8 bytes.
__global__ void __launch_bounds__(kThreads) jpeg_idct_kernel(const int16_t* __restrict__ coefs, size_t coef_bytes,
                                                             const Desc* __restrict__ descs, uint8_t* __restrict__ work,
                                                             size_t work_bytes, size_t sources_bytes) {
    __shared__ int tile[kSlots][8][9];
    const Desc& d = descs[blockIdx.y];
    DevGeometry g;
    if (!dev_geometry(d, g, coef_bytes, work_bytes, sources_bytes)) return;      // (uniform over the workgroup)
    const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int16_t* src = coefs + d.coef_offset / 2;
    uint8_t* planes = work + d.work_offset;
    for (int first = blockIdx.x * kSlots; first < g.total; first += gridDim.x * kSlots) {       // (uniform trip count)
        const int blk = first + slot;
        const bool on = blk < g.total;
        const int c = !on ? 0 : blk >= g.base[3] ? 3 : blk >= g.base[2] ? 2 : blk >= g.base[1] ? 1 : 0;     // (a missing component's base = total)
        const int qc = c == 3 ? d.quant3 : c;
        int v[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0;
        if (on) {
            const uint4 cq = *reinterpret_cast<const uint4*>(src + (size_t)blk * 64 + lane * 8);
            const uint4 qq = *reinterpret_cast<const uint4*>(&d.quant[qc][lane * 8]);
            const unsigned cu[4] = {cq.x, cq.y, cq.z, cq.w}, qu[4] = {qq.x, qq.y, qq.z, qq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = (int)(short)(cu[i] & 0xffffu) * (int)(qu[i] & 0xffffu);
                v[2 * i + 1] = (int)(short)(cu[i] >> 16) * (int)(qu[i] >> 16);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[slot][lane][i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[slot][i][lane];
        idct8(v, o, 11);                                        // CONST_BITS - PASS1_BITS
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[slot][i][lane] = o[i];  // (the elements this lane read: no hazard)
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[slot][lane][i];
        idct8(v, o, 18);                                        // CONST_BITS + PASS1_BITS + 3
        if (on) {
            const int bi = blk - g.base[c], by = bi / g.bw[c], bx = bi - by * g.bw[c];
            uint2 px;
            px.x = range_limit(o[0]) | (range_limit(o[1]) << 8) | (range_limit(o[2]) << 16) | (range_limit(o[3]) << 24);
            px.y = range_limit(o[4]) | (range_limit(o[5]) << 8) | (range_limit(o[6]) << 16) | (range_limit(o[7]) << 24);
            // plane c: rows of bw*8 bytes at block base[c] * 64 (work_offset is a multiple of 16: the store is aligned)
            *reinterpret_cast<uint2*>(planes + (size_t)g.base[c] * 64 + ((size_t)(by * 8 + lane) * g.bw[c] + bx) * 8) = px;
        }
        // the next iteration writes row `lane`, which only this lane reads above: no barrier needed here
    }
}

// chroma sample of pixel (x, y): libjpeg's fancy upsampling of one component plane (stride in bytes)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ plane, int stride, const DevGeometry& g, int x, int y) {
    if (g.hs == 1) return plane[(size_t)y * stride + x];
    const int i = x >> 1;
    if (g.cw <= 2) return plane[(size_t)(g.vs == 2 ? y >> 1 : y) * stride + i];       // replicated (the library's rule)
    const int left = max(i - 1, 0), right = min(i + 1, g.cw - 1);
    const int nb = (x & 1) ? right : left;
    if (g.vs == 1) {
        const uint8_t* row = plane + (size_t)y * stride;
        return nb == i ? row[i] : (3 * row[i] + row[nb] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int r = y >> 1;
    const int rn = (y & 1) ? min(r + 1, g.ch - 1) : max(r - 1, 0);
    const uint8_t* row0 = plane + (size_t)r * stride;
    const uint8_t* row1 = plane + (size_t)rn * stride;
    const int here = 3 * row0[i] + row1[i], there = 3 * row0[nb] + row1[nb];
    return (3 * here + there + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ unsigned clip255(int v) { return (unsigned)min(max(v, 0), 255); }

// Pillow's MULDIV255: a * b / 255, rounded, for a, b in 0..255
__device__ __forceinline__ int muldiv255(int a, int b) {
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

// One thread per 4 consecutive pixels of the packed image = 12 bytes = three aligned dword stores (src_offset is a multiple
// of 16); the last, partial group of an image is stored byte by byte so that nothing behind the image is touched.
__global__ void __launch_bounds__(kThreads) jpeg_colour_kernel(const Desc* __restrict__ descs, const uint8_t* __restrict__ work,
                                                               size_t coef_bytes, size_t work_bytes,
                                                               uint8_t* __restrict__ sources, size_t sources_bytes) {
    const Desc& d = descs[blockIdx.y];
    DevGeometry g;
    if (!dev_geometry(d, g, coef_bytes, work_bytes, sources_bytes)) return;
    const int w = d.width;
    const unsigned npix = (unsigned)w * (unsigned)d.height, groups = (npix + 3u) >> 2;
    const uint8_t* yp = work + d.work_offset;
    const uint8_t* cbp = yp + (size_t)g.base[1] * 64;
    const uint8_t* crp = yp + (size_t)g.base[2] * 64;
    const uint8_t* kp = yp + (size_t)g.base[3] * 64;            // (read only when the image has four components)
    const int ys = g.bw[0] * 8, cs = g.bw[1] * 8;
    uint8_t* dst = sources + d.src_offset;
    for (unsigned it = blockIdx.x * kThreads + threadIdx.x; it < groups; it += gridDim.x * kThreads) {
        const unsigned p0 = it * 4u;
        int y = (int)(p0 / (unsigned)w), x = (int)(p0 - (unsigned)y * (unsigned)w);
        unsigned bytes[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned r = 0, gg = 0, b = 0;
            if (p0 + i < npix) {
                const int lum = yp[(size_t)y * ys + x];
                if (g.ncomp == 1) {
                    r = gg = b = (unsigned)lum;
                } else if (g.ncomp == 4) {
                    // Adobe CMYK, stored inverted: the library passes the four samples through, Pillow inverts them on load
                    // (C = 255 - sample) and converts with nk = 255 - K = the fourth sample
                    const size_t at = (size_t)y * ys + x;       // (four planes of one size)
                    const int nk = kp[at];
                    r = clip255(nk - muldiv255(255 - lum, nk));
                    gg = clip255(nk - muldiv255(255 - (int)cbp[at], nk));
                    b = clip255(nk - muldiv255(255 - (int)crp[at], nk));
                } else {
                    const int cb = chroma_at(cbp, cs, g, x, y) - 128, cr = chroma_at(crp, cs, g, x, y) - 128;
                    r = clip255(lum + ((91881 * cr + 32768) >> 16));
                    gg = clip255(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                    b = clip255(lum + ((116130 * cb + 32768) >> 16));
                }
            }
            bytes[3 * i] = r;
            bytes[3 * i + 1] = gg;
            bytes[3 * i + 2] = b;
            if (++x == w) {
                x = 0;
                ++y;
            }
        }
        if (p0 + 4u <= npix) {
            unsigned* q = reinterpret_cast<unsigned*>(dst + (size_t)it * 12);
#pragma unroll
            for (int j = 0; j < 3; ++j) q[j] = bytes[4 * j] | (bytes[4 * j + 1] << 8) | (bytes[4 * j + 2] << 16) | (bytes[4 * j + 3] << 24);
        } else {
            const int valid = (int)(npix - p0) * 3;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (j < valid) dst[(size_t)it * 12 + j] = (uint8_t)bytes[j];
            }
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ entry points
extern "C" size_t mpn_jpeg_desc_bytes(void) { return sizeof(Desc); }

extern "C" int mpn_jpeg_info(const uint8_t* data, size_t nbytes, mpn_jpeg_header* out) {
    MPN_REQUIRE(data && out, MPN_ERR_BAD_ARG, "jpeg_info: null pointer");
    Parsed p;
    const int reason = parse(data, nbytes, p);
    fill_info(p, reason, out);
    MPN_REQUIRE(reason != MPN_JPEG_MALFORMED, MPN_ERR_BAD_DATA, "jpeg_info: not a JPEG stream, or its headers are damaged");
    return MPN_OK;
}

extern "C" int mpn_jpeg_entropy_decode(const uint8_t* data, size_t nbytes, int16_t* coefs, size_t coef_bytes, mpn_jpeg_desc* desc) {
    MPN_REQUIRE(data && coefs && desc, MPN_ERR_BAD_ARG, "jpeg_entropy_decode: null pointer");
    Parsed p;
    const int reason = parse(data, nbytes, p);
    MPN_REQUIRE(reason == MPN_JPEG_SUPPORTED, MPN_ERR_BAD_DATA, "jpeg_entropy_decode: stream not supported (reason %d, see MPN_JPEG_*)", reason);
    Geometry g;
    geometry_of(p, g);
    const size_t need = (size_t)g.base[3] * 128;
    MPN_REQUIRE(coef_bytes >= need, MPN_ERR_WORKSPACE, "jpeg_entropy_decode: coef_bytes %zu < %zu", coef_bytes, need);
    HuffTable dc[3], ac[3];
    for (int c = 0; c < g.ncomp; ++c) {
        MPN_REQUIRE(build_table(p.hbits[0][p.td[c]], p.hvals[0][p.td[c]], dc[c]) && build_table(p.hbits[1][p.ta[c]], p.hvals[1][p.ta[c]], ac[c]),
                    MPN_ERR_BAD_DATA, "jpeg_entropy_decode: a Huffman table is not a prefix code");
    }
    memset(coefs, 0, need);
    Bits b = {data + p.scan_pos, data + nbytes, 0, 0, 0, false};
    int pred[3] = {0, 0, 0};
    const int mcus_x = g.bw[0] / g.hs;
    const long long mcus = (long long)mcus_x * (g.bh[0] / g.vs);
    int mx = 0, my = 0, until_restart = p.restart;
    for (long long m = 0; m < mcus; ++m) {
        if (p.restart && until_restart == 0) {
            // a restart: the coder was flushed to a byte boundary and an RSTn marker follows (the reader stops in front of it)
            MPN_REQUIRE(!b.overran(), MPN_ERR_BAD_DATA, "jpeg_entropy_decode: the scan ends before its restart interval does");
            const uint8_t* q = b.p;
            while (q + 1 < b.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
            MPN_REQUIRE(q + 1 < b.end && q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7, MPN_ERR_BAD_DATA,
                        "jpeg_entropy_decode: restart marker missing");
            b.p = q + 2;
            b.buf = 0;
            b.n = b.fake = 0;
            b.stopped = false;
            pred[0] = pred[1] = pred[2] = 0;
            until_restart = p.restart;
        }
        for (int c = 0; c < g.ncomp; ++c) {
            const int ch = c == 0 ? g.hs : 1, cv = c == 0 ? g.vs : 1;
            for (int v = 0; v < cv; ++v) {
                for (int h = 0; h < ch; ++h) {
                    int16_t* out = coefs + (g.base[c] + (long long)(my * cv + v) * g.bw[c] + (mx * ch + h)) * 64;
                    MPN_REQUIRE(decode_block(b, dc[c], ac[c], pred[c], out), MPN_ERR_BAD_DATA, "jpeg_entropy_decode: damaged entropy-coded data");
                }
            }
        }
        --until_restart;
        if (++mx == mcus_x) {
            mx = 0;
            ++my;
        }
    }
    MPN_REQUIRE(!b.overran(), MPN_ERR_BAD_DATA, "jpeg_entropy_decode: the scan ends before the image does");
    memset(desc, 0, sizeof(*desc));
    desc->width = p.width;
    desc->height = p.height;
    desc->components = g.ncomp;
    desc->h_samp = g.hs;
    desc->v_samp = g.vs;
    desc->total_blocks = (int32_t)g.base[3];
    for (int c = 0; c < g.ncomp; ++c) {
        desc->blocks_w[c] = g.bw[c];
        desc->blocks_h[c] = g.bh[c];
        memcpy(desc->quant[c], p.q[p.tq[c]], sizeof(desc->quant[c]));
    }
    return MPN_OK;
}

// The marker scan as a descriptor for the device's entropy stage (jpeg_entropy.hip): headers only, the scan's bytes untouched.
extern "C" size_t mpn_jpeg_scan_desc_bytes(void) { return sizeof(mpn_jpeg_scan_desc); }

extern "C" int mpn_jpeg_scan_prepare(const uint8_t* data, size_t nbytes, mpn_jpeg_scan_desc* out) {
    MPN_REQUIRE(data && out, MPN_ERR_BAD_ARG, "jpeg_scan_prepare: null pointer");
    Parsed p;
    int reason = parse(data, nbytes, p);
    if (reason == MPN_JPEG_SUPPORTED && nbytes > (size_t)MPN_JPEG_MAX_FILE_BYTES) reason = MPN_JPEG_TOO_LARGE;
    memset(out, 0, sizeof(*out));
    out->nbytes = (int64_t)nbytes;
    out->width = p.width;
    out->height = p.height;
    out->components = p.ncomp;
    out->h_samp = p.hs[0];
    out->v_samp = p.vs[0];
    out->restart_interval = p.restart;
    out->supported = reason == MPN_JPEG_SUPPORTED;
    out->reason = reason;
    MPN_REQUIRE(reason != MPN_JPEG_MALFORMED, MPN_ERR_BAD_DATA, "jpeg_scan_prepare: not a JPEG stream, or its headers are damaged");
    if (reason != MPN_JPEG_SUPPORTED) return MPN_OK;
    Geometry g;
    geometry_of(p, g);
    out->scan_offset = (int64_t)p.scan_pos;
    out->total_blocks = (int32_t)g.base[3];
    for (int c = 0; c < g.ncomp; ++c) {
        out->blocks_w[c] = g.bw[c];
        out->blocks_h[c] = g.bh[c];
        out->dc_table[c] = p.td[c];
        out->ac_table[c] = p.ta[c];
        memcpy(out->quant[c], p.q[p.tq[c]], sizeof(out->quant[c]));
    }
    for (int tc = 0; tc < 2; ++tc) {
        for (int th = 0; th < 4; ++th) {
            if (!p.hset[tc][th]) continue;
            memcpy(out->huff_bits[tc][th], p.hbits[tc][th] + 1, 16);
            memcpy(out->huff_vals[tc][th], p.hvals[tc][th], 256);
        }
    }
    return MPN_OK;
}

extern "C" size_t mpn_jpeg_decode_workspace_bytes(int B, long long total_blocks) {
    if (B < 1 || total_blocks < B) return 0;
    return (size_t)total_blocks * 64;
}

extern "C" int mpn_jpeg_decode(const int16_t* coefs, size_t coef_bytes, const void* descs, int B, uint8_t* sources_out,
                               size_t sources_bytes, void* work, size_t work_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(coefs && descs && sources_out && work, MPN_ERR_BAD_ARG, "jpeg_decode: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "jpeg_decode: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(mpn_aligned16(coefs) && mpn_aligned16(descs) && mpn_aligned16(sources_out) && mpn_aligned16(work), MPN_ERR_BAD_ALIGN,
                "jpeg_decode: coefs, descs, sources_out and work must be 16-byte aligned");
    MPN_REQUIRE(coef_bytes >= 128 && work_bytes >= 64 && sources_bytes >= 3, MPN_ERR_WORKSPACE,
                "jpeg_decode: coefficients of %zu, workspace of %zu, sources of %zu bytes", coef_bytes, work_bytes, sources_bytes);
    const Desc* dd = reinterpret_cast<const Desc*>(descs);
    jpeg_idct_kernel<<<dim3(kIdctGroups, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        coefs, coef_bytes, dd, reinterpret_cast<uint8_t*>(work), work_bytes, sources_bytes);
    MPN_LAUNCH_CHECK();
    jpeg_colour_kernel<<<dim3(kColourGroups, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        dd, reinterpret_cast<const uint8_t*>(work), coef_bytes, work_bytes, sources_out, sources_bytes);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
