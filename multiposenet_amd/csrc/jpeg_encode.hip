// Baseline JPEG encode on the device (include/mpn.h, "JPEG encode"): the scan libjpeg(-turbo) - and so Pillow - writes for the
// same pixels, quantisation tables and sampling, byte for byte.
//
//   mpn_jpeg_forward         jpeg_forward_kernel      RGB(A) -> YCbCr, chroma down-sampling, 8x8 forward DCT, quantisation ->
//                                                     int16 coefficients in mpn_jpeg_entropy_decode's layout
//   mpn_jpeg_entropy_encode  jpeg_count_bits_kernel   bits of every block (scan order) + sums per chunk of 256 blocks
//                            jpeg_scan_bits_kernel    one workgroup per image: exclusive scan of the chunk sums, total bits
//                            jpeg_zero_words_kernel   zeroes the words the stream will take
//                            jpeg_emit_kernel         every block ORs its codes into the big-endian word buffer (atomicOr)
//                            jpeg_count_ff_kernel     0xFF bytes per chunk of 256 words (the last byte padded with 1-bits)
//                            jpeg_finish_kernel       one workgroup per image: scan of those counts, fit test, the record
//                            jpeg_scatter_kernel      bytes to their stuffed positions, 0x00 behind every 0xFF, then FF D9
//
// All integer arithmetic, libjpeg's: jccolor.c (16-bit fixed point), jcsample.c (h2v1 / h2v2 with alternating bias),
// jcprepct.c (edge replication), jfdctint.c (slow integer DCT), jcdctmgr.c (quantisation), jccoefct.c (dummy blocks),
// jchuff.c with the Annex K tables. Nothing synchronises with the host or allocates: every size a later kernel needs is read
// from the image's workspace header.
#include "common.h"

namespace {

typedef mpn_jpeg_enc_desc Desc;
static_assert(sizeof(Desc) == MPN_JPEG_ENC_DESC_BYTES, "descriptor layout is part of the ABI");

// Annex K.3 - K.6 as (code length << 16) | code, indexed by symbol (0: the table has no such symbol)
__device__ const uint32_t kDcLuma[12] = {
    0x20000, 0x30002, 0x30003, 0x30004, 0x30005, 0x30006, 0x4000e, 0x5001e, 0x6003e, 0x7007e, 0x800fe, 0x901fe,
};
__device__ const uint32_t kAcLuma[256] = {
    0x4000a, 0x20000, 0x20001, 0x30004, 0x4000b, 0x5001a, 0x70078, 0x800f8, 0xa03f6, 0x10ff82, 0x10ff83, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0x4000c, 0x5001b, 0x70079, 0x901f6, 0xb07f6, 0x10ff84, 0x10ff85,
    0x10ff86, 0x10ff87, 0x10ff88, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x5001c, 0x800f9, 0xa03f7,
    0xc0ff4, 0x10ff89, 0x10ff8a, 0x10ff8b, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x0, 0x0, 0x0, 0x0, 0x0,
    0x0, 0x6003a, 0x901f7, 0xc0ff5, 0x10ff8f, 0x10ff90, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0x6003b, 0xa03f8, 0x10ff96, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a,
    0x10ff9b, 0x10ff9c, 0x10ff9d, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x7007a, 0xb07f7, 0x10ff9e,
    0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x0, 0x0, 0x0, 0x0, 0x0,
    0x0, 0x7007b, 0xc0ff6, 0x10ffa6, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0x800fa, 0xc0ff7, 0x10ffae, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2,
    0x10ffb3, 0x10ffb4, 0x10ffb5, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x901f8, 0xf7fc0, 0x10ffb6,
    0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x0, 0x0, 0x0, 0x0, 0x0,
    0x0, 0x901f9, 0x10ffbe, 0x10ffbf, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0x901fa, 0x10ffc7, 0x10ffc8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc,
    0x10ffcd, 0x10ffce, 0x10ffcf, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0xa03f9, 0x10ffd0, 0x10ffd1,
    0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x0, 0x0, 0x0, 0x0, 0x0,
    0x0, 0xa03fa, 0x10ffd9, 0x10ffda, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0xb07f8, 0x10ffe2, 0x10ffe3, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7,
    0x10ffe8, 0x10ffe9, 0x10ffea, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x10ffeb, 0x10ffec, 0x10ffed,
    0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x0, 0x0, 0x0, 0x0, 0x0,
    0xb07f9, 0x10fff5, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0x0,
    0x0, 0x0, 0x0, 0x0,
};
__device__ const uint32_t kDcChroma[12] = {
    0x20000, 0x20001, 0x20002, 0x30006, 0x4000e, 0x5001e, 0x6003e, 0x7007e, 0x800fe, 0x901fe, 0xa03fe, 0xb07fe,
};
__device__ const uint32_t kAcChroma[256] = {
    0x20000, 0x20001, 0x30004, 0x4000a, 0x50018, 0x50019, 0x60038, 0x70078, 0x901f4, 0xa03f6, 0xc0ff4, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0x4000b, 0x60039, 0x800f6, 0x901f5, 0xb07f6, 0xc0ff5, 0x10ff88,
    0x10ff89, 0x10ff8a, 0x10ff8b, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x5001a, 0x800f7, 0xa03f7,
    0xc0ff6, 0xf7fc2, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x10ff8f, 0x10ff90, 0x0, 0x0, 0x0, 0x0, 0x0,
    0x0, 0x5001b, 0x800f8, 0xa03f8, 0xc0ff7, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x10ff96, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0x6003a, 0x901f6, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b,
    0x10ff9c, 0x10ff9d, 0x10ff9e, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x6003b, 0xa03f9, 0x10ff9f,
    0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x10ffa6, 0x0, 0x0, 0x0, 0x0, 0x0,
    0x0, 0x70079, 0xb07f7, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x10ffae, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0x7007a, 0xb07f8, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3,
    0x10ffb4, 0x10ffb5, 0x10ffb6, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x800f9, 0x10ffb7, 0x10ffb8,
    0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x10ffbe, 0x10ffbf, 0x0, 0x0, 0x0, 0x0, 0x0,
    0x0, 0x901f7, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x10ffc7, 0x10ffc8, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0x901f8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce,
    0x10ffcf, 0x10ffd0, 0x10ffd1, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x901f9, 0x10ffd2, 0x10ffd3,
    0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x10ffd9, 0x10ffda, 0x0, 0x0, 0x0, 0x0, 0x0,
    0x0, 0x901fa, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x10ffe2, 0x10ffe3, 0x0,
    0x0, 0x0, 0x0, 0x0, 0x0, 0xb07f9, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9,
    0x10ffea, 0x10ffeb, 0x10ffec, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0xe3fe0, 0x10ffed, 0x10ffee,
    0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x10fff5, 0x0, 0x0, 0x0, 0x0, 0x0,
    0xa03fa, 0xf7fc3, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0x0,
    0x0, 0x0, 0x0, 0x0,
};

// zigzag position -> natural (row-major) position
__device__ const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kThreads = 256;
constexpr int kSlots = kThreads / 8;        // 8x8 blocks of a workgroup in the forward kernel: eight lanes each
constexpr int kForwardGroups = 256;         // workgroups per image (grid-stride)
constexpr int kEntropyGroups = 128;
constexpr long long kMaxCapacity = 1ll << 30;

__host__ __device__ inline unsigned long long round16(unsigned long long n) { return (n + 15ull) & ~15ull; }

// An image's share of the entropy workspace, in bytes from its work_offset. Sizes in 32-bit words:
//   nbits  [T]            bits of every block, in scan order
//   sums_a [ceil(T/256)]  bits per chunk of 256 blocks, then (in place) their exclusive scan
//   words  [W]            the unstuffed bit stream, big-endian inside a word; W = capacity / 4 + 4
//   sums_b [ceil(W/256)]  0xFF bytes per chunk of 256 words, then their exclusive scan
//   head   [4]            total bits, total 0xFF bytes, 1 = the raw stream exceeds the capacity, 1 = the stuffed stream fits
struct WorkLayout {
    unsigned long long nbits, sums_a, words, sums_b, head, bytes;
    unsigned n_words;
};

__host__ __device__ inline WorkLayout work_layout(long long total_blocks, long long capacity) {
    WorkLayout l;
    const unsigned long long T = (unsigned long long)total_blocks, W = (unsigned long long)capacity / 4 + 4;
    l.n_words = (unsigned)W;
    l.nbits = 0;
    l.sums_a = l.nbits + round16(4 * T);
    l.words = l.sums_a + round16(4 * ((T + 255) / 256));
    l.sums_b = l.words + round16(4 * W);
    l.head = l.sums_b + round16(4 * ((W + 255) / 256));
    l.bytes = l.head + 16;
    return l;
}

struct Geometry {
    int hs, vs, mx, my, total;
    int bw[3], bh[3], base[3];
    int rbw, rbh;               // luma's own block grid: blocks beyond it are dummy blocks
    int ch;                     // rows of a down-sampled chroma component
};

__device__ __forceinline__ bool geometry_of(const Desc& d, Geometry& g) {
    if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535) return false;
    if (d.channels != 3 && d.channels != 4) return false;
    if (!((d.h_samp == 1 && d.v_samp == 1) || (d.h_samp == 2 && (d.v_samp == 1 || d.v_samp == 2)))) return false;
    g.hs = d.h_samp;
    g.vs = d.v_samp;
    g.mx = (d.width + 8 * g.hs - 1) / (8 * g.hs);
    g.my = (d.height + 8 * g.vs - 1) / (8 * g.vs);
    const long long total = (long long)g.mx * g.my * (g.hs * g.vs + 2);
    if (total > MPN_JPEG_ENC_MAX_BLOCKS) return false;
    g.total = (int)total;
    g.bw[0] = g.mx * g.hs;
    g.bh[0] = g.my * g.vs;
    g.bw[1] = g.bw[2] = g.mx;
    g.bh[1] = g.bh[2] = g.my;
    g.base[0] = 0;
    g.base[1] = g.bw[0] * g.bh[0];
    g.base[2] = g.base[1] + g.mx * g.my;
    g.rbw = (d.width + 7) / 8;
    g.rbh = (d.height + 7) / 8;
    g.ch = (d.height + g.vs - 1) / g.vs;
    return true;
}

__device__ __forceinline__ bool coefs_ok(const Desc& d, const Geometry& g, size_t coef_bytes) {
    return d.coef_offset >= 0 && (d.coef_offset & 15) == 0 &&
           (unsigned long long)d.coef_offset + (unsigned long long)g.total * 128ull <= coef_bytes;
}

__device__ __forceinline__ bool forward_ok(const Desc& d, Geometry& g, size_t sources_bytes, size_t coef_bytes) {
    if (!geometry_of(d, g) || !coefs_ok(d, g, coef_bytes)) return false;
    return d.src_offset >= 0 && (d.src_offset & 15) == 0 &&
           (unsigned long long)d.src_offset + (unsigned long long)d.width * d.height * d.channels <= sources_bytes;
}

__device__ __forceinline__ bool entropy_ok(const Desc& d, Geometry& g, WorkLayout& l, size_t coef_bytes, size_t out_bytes, size_t work_bytes) {
    if (!geometry_of(d, g) || !coefs_ok(d, g, coef_bytes)) return false;
    if (d.capacity < 16 || d.capacity > kMaxCapacity) return false;
    if (d.out_offset < 0 || (d.out_offset & 15) || (unsigned long long)d.out_offset + (unsigned long long)d.capacity > out_bytes) return false;
    l = work_layout(g.total, d.capacity);
    return d.work_offset >= 0 && (d.work_offset & 15) == 0 && (unsigned long long)d.work_offset + l.bytes <= work_bytes;
}

// ------------------------------------------------------------------------------------------------ forward
constexpr int fix16(double x) { return (int)(x * 65536.0 + 0.5); }

// component c of pixel (x, y), both inside the image (jccolor.c)
__device__ __forceinline__ int component_at(const uint8_t* __restrict__ img, int channels, int w, int c, int x, int y) {
    int r, g, b;
    const size_t at = (size_t)y * w + x;
    if (channels == 4) {
        const unsigned p = *reinterpret_cast<const unsigned*>(img + at * 4);       // (the image starts on a multiple of 16)
        r = p & 255u;
        g = (p >> 8) & 255u;
        b = (p >> 16) & 255u;
    } else {
        r = img[at * 3];
        g = img[at * 3 + 1];
        b = img[at * 3 + 2];
    }
    if (c == 0) return (fix16(0.299) * r + fix16(0.587) * g + fix16(0.114) * b + 32768) >> 16;
    if (c == 1) return (-fix16(0.16874) * r - fix16(0.33126) * g + fix16(0.5) * b + (128 << 16) + 32767) >> 16;
    return (fix16(0.5) * r - fix16(0.41869) * g - fix16(0.08131) * b + (128 << 16) + 32767) >> 16;
}

// One pass of the slow-integer forward DCT over 8 values (jfdctint.c): CONST_BITS = 13, PASS1_BITS = 2.
template <bool kRows>
__device__ __forceinline__ void fdct8(const int (&d)[8], int (&out)[8]) {
    constexpr int n = kRows ? 11 : 15, round = 1 << (n - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (kRows) {
        out[0] = (t10 + t11) * 4;
        out[4] = (t10 - t11) * 4;
    } else {
        out[0] = (t10 + t11 + 2) >> 2;
        out[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    out[2] = (z1 + t13 * 6270 + round) >> n;
    out[6] = (z1 - t12 * 15137 + round) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    out[7] = (a4 + z1 + z3 + round) >> n;
    out[5] = (a5 + z2 + z4 + round) >> n;
    out[3] = (a6 + z2 + z3 + round) >> n;
    out[1] = (a7 + z1 + z4 + round) >> n;
}

// Eight lanes per 8x8 block: lane r converts and (for chroma) down-samples sample row r and runs the row pass; rows meet
// columns through LDS (lane c runs the column pass on column c), and again on the way back, so that lane r quantises and
// stores coefficient row r as 16 bytes. A dummy block runs on the pixels of the block whose DC it repeats.
__global__ void __launch_bounds__(kThreads) jpeg_forward_kernel(const uint8_t* __restrict__ sources, size_t sources_bytes,
                                                                const Desc* __restrict__ descs, int16_t* __restrict__ coefs,
                                                                size_t coef_bytes) {
    __shared__ int tile[kSlots][8][9];
    const Desc& d = descs[blockIdx.y];
    Geometry g;
    if (!forward_ok(d, g, sources_bytes, coef_bytes)) return;                    // (uniform over the workgroup)
    const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const uint8_t* img = sources + d.src_offset;
    int16_t* dst = coefs + d.coef_offset / 2;
    const int w = d.width, h = d.height, channels = d.channels;
    for (int first = blockIdx.x * kSlots; first < g.total; first += gridDim.x * kSlots) {       // (uniform trip count)
        const int blk = first + slot;
        const bool on = blk < g.total;
        const int c = !on ? 0 : blk >= g.base[2] ? 2 : blk >= g.base[1] ? 1 : 0;
        const int bi = blk - g.base[c], by = bi / g.bw[c], bx = bi - by * g.bw[c];
        bool dummy = false;
        int v[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0;
        if (on) {
            int sy = by, sx = bx;
            if (c == 0 && (by >= g.rbh || bx >= g.rbw)) {       // the preceding block in MCU order (jccoefct.c)
                dummy = true;
                if (by >= g.rbh) {
                    sy = by - 1;
                    sx = bx | (g.hs - 1);
                }
                if (sx >= g.rbw) sx -= 1;
            }
            if (c == 0 || g.hs == 1) {
                const int y = min(sy * 8 + lane, h - 1);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = component_at(img, channels, w, c, min(sx * 8 + i, w - 1), y) - 128;
            } else {
                const int yc = min(sy * 8 + lane, g.ch - 1);    // the last DOWN-SAMPLED row is replicated
                const int y0 = min(yc * g.vs, h - 1), y1 = min(yc * g.vs + g.vs - 1, h - 1);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int x0 = min((sx * 8 + i) * 2, w - 1), x1 = min((sx * 8 + i) * 2 + 1, w - 1);
                    int s = component_at(img, channels, w, c, x0, y0) + component_at(img, channels, w, c, x1, y0);
                    if (g.vs == 2) {
                        s += component_at(img, channels, w, c, x0, y1) + component_at(img, channels, w, c, x1, y1);
                        v[i] = ((s + 1 + (i & 1)) >> 2) - 128;
                    } else {
                        v[i] = ((s + (i & 1)) >> 1) - 128;
                    }
                }
            }
        }
        fdct8<true>(v, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[slot][lane][i] = o[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[slot][i][lane];
        fdct8<false>(v, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[slot][i][lane] = o[i];  // (the elements this lane read: no hazard)
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[slot][lane][i];
        if (on) {
            const uint4 qq = *reinterpret_cast<const uint4*>(&d.quant[c][lane * 8]);
            const unsigned qu[4] = {qq.x, qq.y, qq.z, qq.w};
            unsigned packed[4];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int q8 = 8 * max((int)((qu[i >> 1] >> (16 * (i & 1))) & 0xffffu), 1);
                const int mag = (abs(v[i]) + (q8 >> 1)) / q8;
                int val = v[i] < 0 ? -mag : mag;
                if (dummy && (lane | i) != 0) val = 0;
                if (i & 1) packed[i >> 1] |= (unsigned)(val & 0xffff) << 16;
                else packed[i >> 1] = (unsigned)(val & 0xffff);
            }
            *reinterpret_cast<uint4*>(dst + (size_t)blk * 64 + lane * 8) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
        }
        // the next iteration writes row `lane`, which only this lane reads above: no barrier needed here
    }
}

// ------------------------------------------------------------------------------------------------ entropy coding
// exclusive scan of one value per thread over the workgroup; `total` = the sum. All threads call it.
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* lds, unsigned& total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const unsigned add = t >= off ? lds[t - off] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const unsigned incl = lds[t];
    total = lds[kThreads - 1];
    __syncthreads();
    return incl - v;
}

// block `k` of MCU `m` in the coefficient planes; c = its component
__device__ __forceinline__ int block_of(const Geometry& g, int m, int k, int& c) {
    const int my = m / g.mx, mx = m - my * g.mx, nl = g.hs * g.vs;
    if (k < nl) {
        const int v = k / g.hs, hh = k - v * g.hs;
        c = 0;
        return (my * g.vs + v) * g.bw[0] + mx * g.hs + hh;
    }
    c = k - nl + 1;
    return g.base[c] + my * g.mx + mx;
}

__device__ __forceinline__ int magnitude_bits(int v) { return 32 - __clz(abs(v)); }      // (0 for 0)

// Walks block s (scan order) of an image as the Huffman coder does and hands every (code, length) pair to `put`.
template <typename Put>
__device__ __forceinline__ void code_block(const int16_t* __restrict__ src, const Geometry& g, int s, Put put) {
    const int per = g.hs * g.vs + 2, m = s / per, k = s - m * per;
    int c, pc;
    const int16_t* blk = src + (size_t)block_of(g, m, k, c) * 64;
    int pred = 0;                                               // the previous block of this component in scan order
    if (c == 0 && k > 0) pred = src[(size_t)block_of(g, m, k - 1, pc) * 64];
    else if (m > 0) pred = src[(size_t)block_of(g, m - 1, c == 0 ? g.hs * g.vs - 1 : k, pc) * 64];
    const uint32_t* dc = c == 0 ? kDcLuma : kDcChroma;
    const uint32_t* ac = c == 0 ? kAcLuma : kAcChroma;
    const int diff = (int)blk[0] - pred;
    int size = min(magnitude_bits(diff), 11);
    put(dc[size] & 0xffffu, dc[size] >> 16);
    if (size) put((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1u), size);
    int run = 0;
    for (int z = 1; z < 64; ++z) {
        const int val = blk[kZigzag[z]];
        if (val == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            put(ac[0xF0] & 0xffffu, ac[0xF0] >> 16);
            run -= 16;
        }
        size = magnitude_bits(val);
        const uint32_t e = ac[((run << 4) | min(size, 15)) & 255];
        put(e & 0xffffu, e >> 16);
        put((unsigned)(val < 0 ? val - 1 : val) & ((1u << size) - 1u), size);
        run = 0;
    }
    if (run) put(ac[0] & 0xffffu, ac[0] >> 16);
}

__global__ void __launch_bounds__(kThreads) jpeg_count_bits_kernel(const int16_t* __restrict__ coefs, size_t coef_bytes,
                                                                   const Desc* __restrict__ descs, size_t out_bytes,
                                                                   uint8_t* __restrict__ work, size_t work_bytes) {
    __shared__ unsigned lds[kThreads];
    const Desc& d = descs[blockIdx.y];
    Geometry g;
    WorkLayout l;
    if (!entropy_ok(d, g, l, coef_bytes, out_bytes, work_bytes)) return;
    const int16_t* src = coefs + d.coef_offset / 2;
    unsigned* nbits = reinterpret_cast<unsigned*>(work + d.work_offset + l.nbits);
    unsigned* sums = reinterpret_cast<unsigned*>(work + d.work_offset + l.sums_a);
    const int chunks = (g.total + kThreads - 1) / kThreads;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int s = chunk * kThreads + threadIdx.x;
        unsigned n = 0;
        if (s < g.total) {
            code_block(src, g, s, [&](unsigned, unsigned len) { n += len; });
            nbits[s] = n;
        }
        unsigned total;
        block_scan(n, lds, total);
        if (threadIdx.x == 0) sums[chunk] = total;
    }
}

// One workgroup per image: the exclusive scan of `count` chunk sums in place, chunk after chunk; returns the grand total.
__device__ __forceinline__ unsigned scan_sums(unsigned* sums, int count, unsigned* lds) {
    unsigned carry = 0;
    for (int first = 0; first < count; first += kThreads) {
        const int i = first + threadIdx.x;
        const unsigned v = i < count ? sums[i] : 0u;
        unsigned total;
        const unsigned before = block_scan(v, lds, total);
        if (i < count) sums[i] = carry + before;
        carry += total;
    }
    return carry;
}

__global__ void __launch_bounds__(kThreads) jpeg_scan_bits_kernel(const Desc* __restrict__ descs, size_t coef_bytes, size_t out_bytes,
                                                                  uint8_t* __restrict__ work, size_t work_bytes) {
    __shared__ unsigned lds[kThreads];
    const Desc& d = descs[blockIdx.x];
    Geometry g;
    WorkLayout l;
    if (!entropy_ok(d, g, l, coef_bytes, out_bytes, work_bytes)) return;
    unsigned* sums = reinterpret_cast<unsigned*>(work + d.work_offset + l.sums_a);
    unsigned* head = reinterpret_cast<unsigned*>(work + d.work_offset + l.head);
    const unsigned bits = scan_sums(sums, (g.total + kThreads - 1) / kThreads, lds);
    if (threadIdx.x == 0) {
        head[0] = bits;
        head[1] = 0;
        head[2] = (unsigned long long)((bits + 7u) >> 3) > (unsigned long long)d.capacity ? 1u : 0u;
        head[3] = 0;
    }
}

// words the emit pass may touch: those of the stream and one more (a block that ends on a word boundary adds nothing to it)
__device__ __forceinline__ unsigned used_words(unsigned bits) { return (bits >> 5) + 2u; }

__global__ void __launch_bounds__(kThreads) jpeg_zero_words_kernel(const Desc* __restrict__ descs, size_t coef_bytes, size_t out_bytes,
                                                                   uint8_t* __restrict__ work, size_t work_bytes) {
    const Desc& d = descs[blockIdx.y];
    Geometry g;
    WorkLayout l;
    if (!entropy_ok(d, g, l, coef_bytes, out_bytes, work_bytes)) return;
    const unsigned* head = reinterpret_cast<const unsigned*>(work + d.work_offset + l.head);
    if (head[2] != 0) return;
    unsigned* words = reinterpret_cast<unsigned*>(work + d.work_offset + l.words);
    const unsigned n = min(used_words(head[0]), l.n_words);
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) words[i] = 0u;
}

__global__ void __launch_bounds__(kThreads) jpeg_emit_kernel(const int16_t* __restrict__ coefs, size_t coef_bytes,
                                                             const Desc* __restrict__ descs, size_t out_bytes,
                                                             uint8_t* __restrict__ work, size_t work_bytes) {
    __shared__ unsigned lds[kThreads];
    const Desc& d = descs[blockIdx.y];
    Geometry g;
    WorkLayout l;
    if (!entropy_ok(d, g, l, coef_bytes, out_bytes, work_bytes)) return;
    const unsigned* head = reinterpret_cast<const unsigned*>(work + d.work_offset + l.head);
    if (head[2] != 0) return;                                   // (uniform)
    const int16_t* src = coefs + d.coef_offset / 2;
    const unsigned* nbits = reinterpret_cast<const unsigned*>(work + d.work_offset + l.nbits);
    const unsigned* sums = reinterpret_cast<const unsigned*>(work + d.work_offset + l.sums_a);
    unsigned* words = reinterpret_cast<unsigned*>(work + d.work_offset + l.words);
    const unsigned limit = min(used_words(head[0]), l.n_words);
    const int chunks = (g.total + kThreads - 1) / kThreads;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int s = chunk * kThreads + threadIdx.x;
        unsigned total;
        const unsigned at = sums[chunk] + block_scan(s < g.total ? nbits[s] : 0u, lds, total);
        if (s >= g.total) continue;                             // (after the scan: every thread took part in it)
        unsigned long long acc = 0;
        unsigned wi = at >> 5;
        int have = (int)(at & 31u);                             // the bits in front of this block: zeros here, ORed in by others
        code_block(src, g, s, [&](unsigned code, unsigned len) {
            acc = (acc << len) | code;
            have += (int)len;
            if (have >= 32) {
                have -= 32;
                if (wi < limit) atomicOr(&words[wi], (unsigned)(acc >> have));
                ++wi;
            }
        });
        if (have > 0 && wi < limit) atomicOr(&words[wi], (unsigned)(acc << (32 - have)));
    }
}

// word i of the finished raw stream: the last partial byte is padded with 1-bits
__device__ __forceinline__ unsigned raw_word(const unsigned* __restrict__ words, unsigned i, unsigned bits) {
    unsigned v = words[i];
    const unsigned tail = bits & 31u;
    if (i == (bits >> 5) && (tail & 7u)) {
        const unsigned upto = (tail + 7u) & ~7u;
        v |= ((1u << (upto - tail)) - 1u) << (32u - upto);
    }
    return v;
}

// 0xFF bytes among the first `valid` bytes (in stream order: from the top) of a word
__device__ __forceinline__ unsigned count_ff(unsigned v, unsigned valid) {
    unsigned n = 0;
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) n += (j < valid && ((v >> (24 - 8 * j)) & 255u) == 255u) ? 1u : 0u;
    return n;
}

__global__ void __launch_bounds__(kThreads) jpeg_count_ff_kernel(const Desc* __restrict__ descs, size_t coef_bytes, size_t out_bytes,
                                                                 uint8_t* __restrict__ work, size_t work_bytes) {
    __shared__ unsigned lds[kThreads];
    const Desc& d = descs[blockIdx.y];
    Geometry g;
    WorkLayout l;
    if (!entropy_ok(d, g, l, coef_bytes, out_bytes, work_bytes)) return;
    const unsigned* head = reinterpret_cast<const unsigned*>(work + d.work_offset + l.head);
    if (head[2] != 0) return;
    const unsigned* words = reinterpret_cast<const unsigned*>(work + d.work_offset + l.words);
    unsigned* sums = reinterpret_cast<unsigned*>(work + d.work_offset + l.sums_b);
    const unsigned bits = head[0], raw = (bits + 7u) >> 3, n = (raw + 3u) >> 2;
    const unsigned chunks = (n + kThreads - 1) / kThreads;
    for (unsigned chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const unsigned i = chunk * kThreads + threadIdx.x;
        const unsigned c = i < n ? count_ff(raw_word(words, i, bits), min(raw - 4u * i, 4u)) : 0u;
        unsigned total;
        block_scan(c, lds, total);
        if (threadIdx.x == 0) sums[chunk] = total;
    }
}

// One workgroup per image: scans the 0xFF counts, decides whether the stream fits, writes the record.
__global__ void __launch_bounds__(kThreads) jpeg_finish_kernel(const Desc* __restrict__ descs, size_t coef_bytes, size_t out_bytes,
                                                               uint8_t* __restrict__ work, size_t work_bytes,
                                                               mpn_jpeg_stream_record* __restrict__ records) {
    __shared__ unsigned lds[kThreads];
    const Desc& d = descs[blockIdx.x];
    mpn_jpeg_stream_record rec = {d.out_offset, 0, MPN_JPEG_ENC_SKIPPED, {0, 0, 0}};
    Geometry g;
    WorkLayout l;
    if (entropy_ok(d, g, l, coef_bytes, out_bytes, work_bytes)) {               // (uniform)
        unsigned* head = reinterpret_cast<unsigned*>(work + d.work_offset + l.head);
        const unsigned raw = (head[0] + 7u) >> 3;
        if (head[2] != 0) {
            rec.size = (long long)raw + 2;
            rec.status = MPN_JPEG_ENC_NO_FIT_RAW;
        } else {
            unsigned* sums = reinterpret_cast<unsigned*>(work + d.work_offset + l.sums_b);
            const unsigned n = (raw + 3u) >> 2;
            const unsigned ff = scan_sums(sums, (int)((n + kThreads - 1) / kThreads), lds);
            rec.size = (long long)raw + ff + 2;
            rec.status = rec.size <= d.capacity ? MPN_JPEG_ENC_OK : MPN_JPEG_ENC_NO_FIT;
            if (threadIdx.x == 0) {
                head[1] = ff;
                head[3] = rec.status == MPN_JPEG_ENC_OK ? 1u : 0u;       // the scatter writes only then
            }
        }
    }
    if (threadIdx.x == 0) records[blockIdx.x] = rec;
}

__global__ void __launch_bounds__(kThreads) jpeg_scatter_kernel(const Desc* __restrict__ descs, size_t coef_bytes,
                                                                uint8_t* __restrict__ out, size_t out_bytes,
                                                                const uint8_t* __restrict__ work, size_t work_bytes) {
    __shared__ unsigned lds[kThreads];
    const Desc& d = descs[blockIdx.y];
    Geometry g;
    WorkLayout l;
    if (!entropy_ok(d, g, l, coef_bytes, out_bytes, work_bytes)) return;
    const unsigned* head = reinterpret_cast<const unsigned*>(work + d.work_offset + l.head);
    if (head[2] != 0 || head[3] != 1u) return;                  // the stream does not fit: nothing is written
    const unsigned* words = reinterpret_cast<const unsigned*>(work + d.work_offset + l.words);
    const unsigned* sums = reinterpret_cast<const unsigned*>(work + d.work_offset + l.sums_b);
    const unsigned bits = head[0], raw = (bits + 7u) >> 3, n = (raw + 3u) >> 2, ff = head[1];
    uint8_t* dst = out + d.out_offset;                          // raw + ff + 2 <= capacity was checked by jpeg_finish_kernel
    const unsigned chunks = (n + kThreads - 1) / kThreads;
    for (unsigned chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const unsigned i = chunk * kThreads + threadIdx.x;
        unsigned v = 0, valid = 0;
        if (i < n) {
            v = raw_word(words, i, bits);
            valid = min(raw - 4u * i, 4u);
        }
        unsigned total;
        unsigned at = 4u * i + sums[chunk] + block_scan(count_ff(v, valid), lds, total);
        for (unsigned j = 0; j < valid; ++j) {
            const unsigned byte = (v >> (24 - 8 * j)) & 255u;
            dst[at++] = (uint8_t)byte;
            if (byte == 255u) dst[at++] = 0;
        }
        if (i + 1 == n) {                                       // behind the last byte: EOI
            dst[raw + ff] = 0xFF;
            dst[raw + ff + 1] = 0xD9;
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ entry points
extern "C" size_t mpn_jpeg_enc_desc_bytes(void) { return sizeof(Desc); }

extern "C" int mpn_jpeg_forward(const uint8_t* sources, size_t sources_bytes, const void* descs, int B, int16_t* coefs,
                                size_t coef_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(sources && descs && coefs, MPN_ERR_BAD_ARG, "jpeg_forward: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "jpeg_forward: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(mpn_aligned16(sources) && mpn_aligned16(descs) && mpn_aligned16(coefs), MPN_ERR_BAD_ALIGN,
                "jpeg_forward: sources, descs and coefs must be 16-byte aligned");
    MPN_REQUIRE(sources_bytes >= 3 && coef_bytes >= 128, MPN_ERR_WORKSPACE, "jpeg_forward: sources of %zu, coefficients of %zu bytes",
                sources_bytes, coef_bytes);
    jpeg_forward_kernel<<<dim3(kForwardGroups, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        sources, sources_bytes, reinterpret_cast<const Desc*>(descs), coefs, coef_bytes);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}

extern "C" size_t mpn_jpeg_entropy_encode_workspace_bytes(long long total_blocks, long long capacity) {
    if (total_blocks < 1 || total_blocks > MPN_JPEG_ENC_MAX_BLOCKS || capacity < 16 || capacity > kMaxCapacity) return 0;
    return (size_t)work_layout(total_blocks, capacity).bytes;
}

extern "C" int mpn_jpeg_entropy_encode(const int16_t* coefs, size_t coef_bytes, const void* descs, int B, uint8_t* out,
                                       size_t out_bytes, void* records, void* work, size_t work_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(coefs && descs && out && records && work, MPN_ERR_BAD_ARG, "jpeg_entropy_encode: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "jpeg_entropy_encode: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(mpn_aligned16(coefs) && mpn_aligned16(descs) && mpn_aligned16(out) && mpn_aligned16(records) && mpn_aligned16(work),
                MPN_ERR_BAD_ALIGN, "jpeg_entropy_encode: coefs, descs, out, records and work must be 16-byte aligned");
    MPN_REQUIRE(coef_bytes >= 128 && out_bytes >= 16 && work_bytes >= 16, MPN_ERR_WORKSPACE,
                "jpeg_entropy_encode: coefficients of %zu, output of %zu, workspace of %zu bytes", coef_bytes, out_bytes, work_bytes);
    const Desc* dd = reinterpret_cast<const Desc*>(descs);
    uint8_t* wk = reinterpret_cast<uint8_t*>(work);
    hipStream_t st = (hipStream_t)stream;
    const dim3 wide(kEntropyGroups, (unsigned)B);
    jpeg_count_bits_kernel<<<wide, kThreads, 0, st>>>(coefs, coef_bytes, dd, out_bytes, wk, work_bytes);
    MPN_LAUNCH_CHECK();
    jpeg_scan_bits_kernel<<<dim3((unsigned)B), kThreads, 0, st>>>(dd, coef_bytes, out_bytes, wk, work_bytes);
    MPN_LAUNCH_CHECK();
    jpeg_zero_words_kernel<<<wide, kThreads, 0, st>>>(dd, coef_bytes, out_bytes, wk, work_bytes);
    MPN_LAUNCH_CHECK();
    jpeg_emit_kernel<<<wide, kThreads, 0, st>>>(coefs, coef_bytes, dd, out_bytes, wk, work_bytes);
    MPN_LAUNCH_CHECK();
    jpeg_count_ff_kernel<<<wide, kThreads, 0, st>>>(dd, coef_bytes, out_bytes, wk, work_bytes);
    MPN_LAUNCH_CHECK();
    jpeg_finish_kernel<<<dim3((unsigned)B), kThreads, 0, st>>>(dd, coef_bytes, out_bytes, wk, work_bytes,
                                                               reinterpret_cast<mpn_jpeg_stream_record*>(records));
    MPN_LAUNCH_CHECK();
    jpeg_scatter_kernel<<<wide, kThreads, 0, st>>>(dd, coef_bytes, out, out_bytes, wk, work_bytes);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
